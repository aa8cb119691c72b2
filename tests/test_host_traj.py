"""Host entries of the trajectory evaluation, none of which needs a device: dpgo_graph_grid3d_truth against the
oracle's ground truth, dpgo_hip_align_moments against the np.longdouble restatement of tests/_traj.py, and
dpgo_g2o_read_vertices on small files written here."""
import ctypes as C

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _traj as TJ

_L = np.longdouble


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    H.lib()
    return H


# ---------------------------------------------------------------------------------------- grid truth
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("seed", [0, 12345])
def test_grid3d_truth_is_bitwise_the_oracles(hip, k, seed):
    want = O.grid3d(k, seed).extra["ground_truth"]
    got = hip.grid3d_truth(k, seed)
    assert got.shape == want.shape == (3, 4 * k ** 3)
    assert np.array_equal(got, want)


def test_grid3d_truth_refusals(hip):
    buf = np.full(12 * 8, 7.0)
    for k in (1, 201, -3):
        assert hip.lib().dpgo_graph_grid3d_truth(k, 0, buf.ctypes.data_as(hip._dp)) != 0
    assert hip.lib().dpgo_graph_grid3d_truth(2, 0, None) != 0
    assert np.all(buf == 7.0)


# ---------------------------------------------------------------------------------------- alignment from moments
def _cases():
    for d in (2, 3):
        for n in (127, 200, 1000):
            for masked in (False, True):
                yield d, n, masked


@pytest.mark.parametrize("d,n,masked", list(_cases()))
def test_align_moments_against_the_restatement(hip, d, n, masked):
    """From the restatement's own moments (rounded to float64), about the float64 means: |A - A_ref| <= 1e-12 and
    |a - a_ref| <= 1e-12 (1 + |mu^| + |mu|), the project's bar for host linear algebra against a longdouble
    restatement; A orthogonal to 1e-14 with det > 0; sigma descending; the rank."""
    F = TJ.fixture(d, n)
    use = F["use"] if masked else None
    m0, _ = TJ.moments(F["That"], F["T"], d, use)
    shift = np.asarray(m0[3:3 + 2 * d] / m0[0], dtype=np.float64)
    m1, _ = TJ.moments(F["That"], F["T"], d, use, shift)
    mom = m1.astype(np.float64)
    ref, rinfo = TJ.align_moments(d, mom, shift)
    Aa, info = hip.align_moments(d, mom, shift)
    dA = float(np.max(np.abs(Aa[:, :d].astype(_L) - ref[:, :d])))
    da = float(np.max(np.abs(Aa[:, d].astype(_L) - ref[:, d])))
    scale = 1.0 + float(np.linalg.norm(rinfo["mu_hat"].astype(np.float64)) + np.linalg.norm(rinfo["mu"].astype(np.float64)))
    print(f"align_moments d={d} n={n} masked={masked}: |A - ref| = {dA:.2e}, |a - ref| = {da:.2e} (scale {scale:.0f})")
    assert dA <= 1e-12
    assert da <= 1e-12 * scale
    A = Aa[:, :d]
    assert np.max(np.abs(A @ A.T - np.eye(d))) <= 1e-14
    assert np.linalg.det(A) > 0
    assert info["count"] == rinfo["count"] == (np.count_nonzero(use) if masked else n)
    sig = info["sigma"]
    assert np.all(np.diff(np.abs(sig)) <= 0) and np.all(sig[:-1] > 0)
    assert np.max(np.abs(sig - rinfo["sigma"].astype(np.float64))) <= 1e-12 * sig[0]
    assert info["rank"] == rinfo["rank"] == d
    # the zero-shift moments give the same map up to what their cancellation costs: far looser, the reason the
    # driver centres first
    Aa0, _ = hip.align_moments(d, m0.astype(np.float64))
    assert np.max(np.abs(Aa0[:, :d] - A)) <= 1e-6


@pytest.mark.parametrize("d", [2, 3])
def test_align_moments_mirrored_and_degenerate(hip, d):
    F = TJ.fixture(d, 200)
    Rh, th = TJ.split(F["That"], d)
    th = th.copy()
    th[:, 0] = -th[:, 0]
    mom, _ = TJ.moments(TJ.join(Rh, th), F["T"], d)
    Aa, info = hip.align_moments(d, mom.astype(np.float64))
    assert np.linalg.det(Aa[:, :d]) > 0 and info["sigma"][-1] < 0
    # one pose: C = 0, A = I, a = t - t^, rank 0
    G = TJ.fixture(d, 1)
    mom, _ = TJ.moments(G["That"], G["T"], d)
    Aa, info = hip.align_moments(d, mom.astype(np.float64))
    assert np.array_equal(Aa[:, :d], np.eye(d)) and info["rank"] == 0 and info["count"] == 1
    assert np.array_equal(Aa[:, d], TJ.split(G["T"], d)[1][0] - TJ.split(G["That"], d)[1][0])
    # collinear translations: rank 1; A is a rotation all the same, and unique for d = 2 only
    n = 50
    R = np.stack([np.eye(d)] * n)
    line = np.outer(np.arange(n, dtype=np.float64), np.ones(d))
    Q = TJ.random_rotations(np.random.default_rng(3), d, 1)[0]
    mom, _ = TJ.moments(TJ.join(R, line), TJ.join(R, line @ Q.T), d)
    Aa, info = hip.align_moments(d, mom.astype(np.float64))
    A = Aa[:, :d]
    assert info["rank"] == 1
    assert np.max(np.abs(A @ A.T - np.eye(d))) <= 1e-14 and np.linalg.det(A) > 0
    assert np.max(np.abs(A @ np.ones(d) - Q @ np.ones(d))) <= 1e-12
    if d == 2:
        assert np.max(np.abs(A - Q)) <= 1e-12
    # a rank tolerance above sigma_d / sigma_1 lowers the rank
    mom, _ = TJ.moments(F["That"], F["T"], d)
    assert hip.align_moments(d, mom.astype(np.float64), rank_tol=0.999)[1]["rank"] < d


def test_align_moments_refusals(hip):
    L = hip.lib()
    F = TJ.fixture(3, 200)
    mom = TJ.moments(F["That"], F["T"], 3)[0].astype(np.float64)
    Aa = np.full(12, 7.0)
    info = hip.AlignInfo()
    info.rank = -7
    dp = hip._dp

    def call(d, m, out, shift=None):
        return L.dpgo_hip_align_moments(d, None if shift is None else shift.ctypes.data_as(dp),
                                        None if m is None else m.ctypes.data_as(dp), 1e-12,
                                        None if out is None else out.ctypes.data_as(dp), C.byref(info))
    assert call(4, mom, Aa) != 0 and call(1, mom, Aa) != 0
    assert call(3, None, Aa) != 0 and call(3, mom, None) != 0
    empty = np.zeros_like(mom)
    assert call(3, empty, Aa) != 0  # count = 0
    bad = mom.copy()
    bad[5] = np.nan
    assert call(3, bad, Aa) != 0
    both = np.concatenate([mom, np.full(12, 7.0)])
    assert L.dpgo_hip_align_moments(3, None, both.ctypes.data_as(dp), 1e-12, both[10:].ctypes.data_as(dp),
                                    C.byref(info)) != 0  # Aa overlaps mom
    assert np.all(Aa == 7.0) and info.rank == -7 and np.array_equal(both[:len(mom)], mom)
    assert call(3, mom, Aa) == 0 and info.rank == 3


# ---------------------------------------------------------------------------------------- g2o vertices
def test_read_vertices_se2(hip, tmp_path):
    p = tmp_path / "a.g2o"
    p.write_text("VERTEX_SE2 0 1.5 -2.0 0.25\n"
                 "EDGE_SE2 0 1 1 0 0 1 0 0 1 0 1\n"
                 "\n"
                 "VERTEX_SE2 2 3.0 4.0 -1.0\n"
                 "VERTEX_SE2 1\n")  # truncated: skipped
    T, present = hip.g2o_read_vertices(p, 2, 4)
    assert present.tolist() == [1, 0, 1, 0]
    R, t = TJ.split(T, 2)
    for j, (x, y, th) in {0: (1.5, -2.0, 0.25), 2: (3.0, 4.0, -1.0)}.items():
        assert np.array_equal(R[j], np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]))
        assert t[j].tolist() == [x, y]
    assert np.all(np.isnan(T[:, 3:6])) and np.all(np.isnan(T[:, 9:12]))


def test_read_vertices_se3_normalises_the_quaternion(hip, tmp_path):
    from scipy.spatial.transform import Rotation
    q = np.array([0.3, -0.2, 0.5, 0.7])  # (qx, qy, qz, qw), norm != 1
    p = tmp_path / "b.g2o"
    p.write_text(f"VERTEX_SE3:QUAT 1 1 2 3 {q[0]} {q[1]} {q[2]} {q[3]}\n"
                 f"VERTEX_SE3:QUAT 0 -1 0 4 {3 * q[0]} {3 * q[1]} {3 * q[2]} {3 * q[3]}\n"
                 "VERTEX_SE3:QUAT 2 0 0 0 0 0 0 1\n")
    T, present = hip.g2o_read_vertices(p, 3, 3)
    assert present.tolist() == [1, 1, 1]
    R, t = TJ.split(T, 3)
    want = Rotation.from_quat(q).as_matrix()
    for j in (0, 1):  # the scale of the quaternion does not matter
        assert np.max(np.abs(R[j] - want)) <= 4e-16
        assert np.max(np.abs(R[j] @ R[j].T - np.eye(3))) <= 1e-15 and np.linalg.det(R[j]) > 0
    assert np.array_equal(R[2], np.eye(3))
    assert t.tolist() == [[-1, 0, 4], [1, 2, 3], [0, 0, 0]]


def test_read_vertices_refusals(hip, tmp_path):
    L = hip.lib()
    p = tmp_path / "c.g2o"
    p.write_text("VERTEX_SE2 0 0 0 0\nVERTEX_SE2 5 1 1 1\n")
    T = np.full(6 * 4, 7.0)
    pres = np.full(4, 7, np.int32)

    def call(path, d, n):
        return L.dpgo_g2o_read_vertices(str(path).encode(), d, n, T.ctypes.data_as(hip._dp),
                                        pres.ctypes.data_as(hip._ip))
    assert call(p, 2, 4) != 0            # id 5 >= n
    assert call(p, 3, 2) != 0            # SE2 vertices, d = 3
    assert call(p, 4, 4) != 0 and call(p, 2, 0) != 0
    assert call(tmp_path / "missing.g2o", 2, 4) != 0
    z = tmp_path / "z.g2o"
    z.write_text("VERTEX_SE3:QUAT 0 0 0 0 0 0 0 0\n")
    assert call(z, 3, 2) != 0            # a zero quaternion is no rotation
    assert np.all(T == 7.0) and np.all(pres == 7)
    with pytest.raises(hip.DPGOHipError):
        hip.g2o_read_vertices(p, 2, 4)
    T6, pr6 = hip.g2o_read_vertices(p, 2, 6)
    assert pr6.tolist() == [1, 0, 0, 0, 0, 1]


def test_graph_truth_is_the_grid_truth(hip):
    g = hip.Graph.grid3d(3, seed=4)
    assert np.array_equal(g.truth(), hip.grid3d_truth(3, 4))
    A = g.arrays()
    h = hip.Graph.from_arrays(3, g.n, **A)
    with pytest.raises(hip.DPGOHipError):
        h.truth()


def test_python_helpers(hip):
    """hip.rot_angle is the restated formula and inverts the chordal distance of a known rotation; hip.merge_traj_sums
    adds entries 0-2 and takes the maximum of 3-4."""
    for d in (2, 3):
        for ang in (0.0, 1e-3, 0.7, 3.0):
            Rm = TJ.exp_so(d, ang if d == 2 else np.array([0.0, 0.0, ang]))
            rot_sq = np.sum((Rm - np.eye(d)) ** 2)
            assert hip.rot_angle(rot_sq) == TJ.rot_angle(rot_sq) and abs(hip.rot_angle(rot_sq) - ang) <= 1e-7
    assert hip.rot_angle(9.0) == np.pi  # clamped
    parts = [[3.0, 1.5, 0.25, 0.9, 0.2], [2.0, 0.5, 0.75, 0.4, 0.6], [0.0, 0.0, 0.0, 0.0, 0.0]]
    assert hip.merge_traj_sums(parts).tolist() == [5.0, 2.0, 1.0, 0.9, 0.6]
    assert hip.traj_moments_len(2) == TJ.moments_len(2) == 11 and hip.traj_moments_len(3) == 18
