"""The ground the trajectory-evaluation GPU tests stand on (tests/_traj.py), checked on the CPU: the restated
alignment against scipy and the d = 2 closed form, its stationarity, the noise-free fixtures, a mirrored estimate, the
fixtures' conditioning, and the gauge freedom of the RPE."""
import numpy as np
import pytest

from tests import _edges as EE
from tests import _traj as TJ

_L = np.longdouble
N = 200


def _cost(That, T, d, Aa, use=None):
    e = TJ.errors(That, T, d, Aa, use)
    return np.nansum(e["tra"])


@pytest.mark.parametrize("masked", [False, True])
def test_alignment_d3_equals_scipy_align_vectors(masked):
    from scipy.spatial.transform import Rotation
    F = TJ.fixture(3, N)
    use = F["use"] if masked else None
    Aa, info = TJ.align(F["That"], F["T"], 3, use)
    u = TJ._used(N, use)
    _, th = TJ.split(F["That"], 3)
    _, tt = TJ.split(F["T"], 3)
    a = th[u] - th[u].mean(axis=0)
    b = tt[u] - tt[u].mean(axis=0)
    rot, _ = Rotation.align_vectors(b, a)  # the rotation that takes a to b
    dA = float(np.max(np.abs(Aa[:, :3].astype(np.float64) - rot.as_matrix())))
    print(f"|A - scipy| = {dA:.2e}")
    assert dA <= 1e-12
    assert info["count"] == np.count_nonzero(u)


@pytest.mark.parametrize("masked", [False, True])
def test_alignment_d2_equals_closed_form(masked):
    F = TJ.fixture(2, N)
    use = F["use"] if masked else None
    Aa, _ = TJ.align(F["That"], F["T"], 2, use)
    u = TJ._used(N, use)
    _, th = TJ.split(F["That"].astype(_L), 2)
    _, tt = TJ.split(F["T"].astype(_L), 2)
    a = th[u] - th[u].mean(axis=0)
    b = tt[u] - tt[u].mean(axis=0)
    Cm = np.einsum("ji,jc->ic", b, a)  # tr(A^T C) = cos (C00 + C11) + sin (C10 - C01)
    th_opt = np.arctan2(Cm[1, 0] - Cm[0, 1], Cm[0, 0] + Cm[1, 1])
    A = np.array([[np.cos(th_opt), -np.sin(th_opt)], [np.sin(th_opt), np.cos(th_opt)]])
    assert float(np.max(np.abs(Aa[:, :2] - A))) <= 1e-15
    mu_h, mu = th[u].mean(axis=0), tt[u].mean(axis=0)
    assert float(np.max(np.abs(Aa[:, 2] - (mu - A @ mu_h)))) <= 1e-13


@pytest.mark.parametrize("d", [2, 3])
def test_alignment_is_a_stationary_point(d):
    """Moving A along each so(d) generator by +-1e-6 (a re-fitted to the means) does not lower the cost."""
    F = TJ.fixture(d, N)
    Aa, info = TJ.align(F["That"], F["T"], d)
    c0 = _cost(F["That"], F["T"], d, Aa)
    gens = [1.0] if d == 2 else [np.array(v) for v in ([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0])]
    for g in gens:
        for sgn in (1e-6, -1e-6):
            A = TJ.exp_so(d, sgn * g).astype(_L) @ Aa[:, :d]
            a = info["mu"] - A @ info["mu_hat"]
            c = _cost(F["That"], F["T"], d, np.concatenate([A, a[:, None]], axis=1))
            assert c >= c0 * (1 - _L(1e-15)), (float(c), float(c0))
    # and a alone: any shift away from mu - A mu^ raises the cost
    for i in range(d):
        for sgn in (1e-6, -1e-6):
            B = Aa.copy()
            B[i, d] += sgn
            assert _cost(F["That"], F["T"], d, B) > c0


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("masked", [False, True])
def test_noise_free_fixture_returns_the_known_transform(d, masked):
    F = TJ.fixture(d, N, noise=False)
    use = F["use"] if masked else None
    Aa, info = TJ.align(F["That"], F["T"], d, use)
    assert float(np.max(np.abs(Aa[:, :d] - F["A0"]))) <= 1e-13
    assert float(np.max(np.abs(Aa[:, d] - F["a0"]))) <= 1e-13 * 3000  # |a0| is of the offset's order
    e = TJ.errors(F["That"], F["T"], d, Aa, use)
    assert float(np.nanmax(e["tra"])) <= (1e-12) ** 2 * 3000 ** 2
    assert float(np.nanmax(e["rot"])) <= (1e-14) ** 2
    assert info["rank"] == d


@pytest.mark.parametrize("d", [2, 3])
def test_mirrored_estimate_still_gives_a_rotation(d):
    F = TJ.fixture(d, N)
    Rh, th = TJ.split(F["That"], d)
    th = th.copy()
    th[:, 0] = -th[:, 0]
    Aa, info = TJ.align(TJ.join(Rh, th), F["T"], d)
    A = Aa[:, :d]
    assert float(TJ._det(A)) > 0
    assert float(np.max(np.abs(A @ A.T - np.eye(d)))) <= 1e-17
    assert info["sigma"][-1] < 0 and np.all(np.diff(np.abs(info["sigma"])) <= 0)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [n for n in TJ.POSE_SIZES if n > 3] + [N])
def test_fixtures_are_well_conditioned(d, n):
    for use in (None, TJ.fixture(d, n)["use"]):
        F = TJ.fixture(d, n)
        _, info = TJ.align(F["That"], F["T"], d, use)
        ratio = float(abs(info["sigma"][-1]) / info["sigma"][0])
        assert ratio >= 0.1, ratio


@pytest.mark.parametrize("d", [2, 3])
def test_rpe_of_a_rigidly_moved_truth_is_at_rounding_level(d):
    """The truth moved by any rigid map has the truth's relative poses: edge errors at r = d, with those as the
    measurements, are at rounding level -- no alignment enters the RPE."""
    F = TJ.fixture(d, N, noise=False)
    p1, p2 = TJ.edges(N, 500)
    R, t, _, _ = TJ.relative_poses(F["T"], d, p1, p2)
    one = np.ones(len(p1))
    e = EE.edge_errors(F["That"], d, p1, p2, R.astype(np.float64), t.astype(np.float64), one, one)
    assert float(np.max(e["rot"])) <= (1e-14) ** 2
    assert float(np.max(e["tra"])) <= (1e-14 * 3000) ** 2
    # and with noise it is not
    G = TJ.fixture(d, N)
    e = EE.edge_errors(G["That"], d, p1, p2, R.astype(np.float64), t.astype(np.float64), one, one)
    assert float(np.min(e["tra"])) > 1e-8


def test_tree_depth_stays_below_the_span_bound():
    """m <= d + 8 + ceil(n / 64), the most any summation order over 64-pose spans needs."""
    for d in (2, 3):
        for n in list(range(1, 1500)) + [10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7]:
            assert TJ.moments_depth(d, n) <= d + 8 + -(-n // 64), n


def test_rot_angle_of_a_known_rotation():
    for d in (2, 3):
        for ang in (0.0, 1e-3, 0.7, 3.0, np.pi):
            Rm = TJ.exp_so(d, ang if d == 2 else np.array([0.0, 0.0, ang]))
            rot_sq = np.sum((Rm - np.eye(d)) ** 2)
            assert abs(TJ.rot_angle(rot_sq) - ang) <= 1e-7 + 1e-12
