"""Host entry points of the robust multi-robot initialisation (no GPU; use_gpu = 0): dpgo_robust_rotation_average
against the longdouble restatement of tests/_frames.py, and dpgo_graph_distributed_init_ex (odometry local
trajectories, GNC-TLS two-stage alignment against the single breadth-first parent) on the two corrupted fixtures whose
ground tests/test_frames_reference.py asserts.

Distance of every non-root agent's frame on the corrupted 3D fixture from the frame computed on the uncorrupted
graph (chordal for the rotation, Euclidean for the translation), robust two-stage / plain L2:
  agent 1  0.0289, 0.0547 / 0.123, 0.725;  agent 2  0.0250, 0.0671 / 0.159, 1.36;  agent 3  0.0286, 0.0908 / 0.168, 2.21
(the robust frames' remainder is the trace converged outliers leave in the pre-final-reweighting estimate)."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _frames as F


@pytest.fixture(scope="module")
def H():
    from dpgo_amd import hip
    return hip


def _rotations(d, n, nin, noise, rng):
    """nin rotations within `noise` rad of one truth, then n - nin at more than 1.2 x the threshold from it."""
    Rt = F._random_rotation(rng, d)
    out = []
    while len(out) < n:
        if len(out) < nin:
            if d == 2:
                a = rng.uniform(-noise, noise)
                dR = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            else:
                v = rng.standard_normal(3)
                v *= rng.uniform(0, noise) / np.linalg.norm(v)
                K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
                th = np.linalg.norm(v)
                dR = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * K @ K if th > 0 else np.eye(3)
            out.append(Rt @ dR)
        else:
            Rr = F._random_rotation(rng, d)
            if np.linalg.norm(Rr - Rt) > 1.2 * F.THRESHOLD:
                out.append(Rr)
    return np.array(out)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("weighted", [False, True])
def test_rotation_average_matches_restatement(H, d, weighted):
    rng = np.random.default_rng(100 * d + weighted)
    ran_gnc = 0
    for n, nin, noise in [(1, 1, 0.0), (5, 5, 0.01), (8, 5, 0.02), (20, 12, 0.02), (50, 10, 0.0), (50, 30, 0.02),
                          (33, 20, 0.01)]:
        Rs = _rotations(d, n, nin, noise, rng)
        kappa = rng.uniform(0.5, 2.0, n) if weighted else None
        Ropt, w, iters = H.robust_rotation_average(Rs, kappa, F.THRESHOLD)
        Rr, wr, ir = F.rotation_average(Rs, kappa, F.THRESHOLD)
        assert np.abs(Ropt - Rr.astype(np.float64)).max() <= 1e-12, (n, nin)
        assert np.abs(w - wr.astype(np.float64)).max() <= 1e-12, (n, nin)
        assert np.array_equal(w == 0.0, wr == 0) and np.array_equal(w == 1.0, wr == 1), (n, nin)
        assert iters == ir, (n, nin, iters, ir)
        if nin < n and n - nin <= 0.45 * n:  # the fixtures' condition; beyond it (d = 2, 80 %) outliers may cluster
            assert list(np.nonzero(w > 1 - 1e-8)[0]) == list(range(nin))
        ran_gnc += iters > 0
    assert ran_gnc >= 4  # the sets with outliers went through the GNC loop; the clean ones skipped it


def test_rotation_average_known_answers_and_errors(H):
    rng = np.random.default_rng(5)
    Rt = F._random_rotation(rng, 3)
    Ropt, w, iters = H.robust_rotation_average(Rt[None])
    assert np.linalg.norm(Ropt - Rt) <= 1e-8 and list(w) == [1.0] and iters == 0
    with pytest.raises(H.DPGOHipError):
        H.robust_rotation_average(np.zeros((0, 3, 3)))
    bad = np.array([Rt, Rt * (1 + 1e-6)])
    with pytest.raises(H.DPGOHipError, match="not a rotation"):
        H.robust_rotation_average(bad)
    refl = np.array([Rt, Rt @ np.diag([1.0, 1.0, -1.0])])
    with pytest.raises(H.DPGOHipError, match="item 1 is not a rotation"):
        H.robust_rotation_average(refl)


@pytest.mark.parametrize("fixture", [F.fixture3d, F.fixture2d])
def test_odometry_robust_init_matches_restatement(H, fixture):
    fx = fixture()
    d, K, aop = fx["d"], fx["K"], fx["aop"]
    g = F.graph_of(H, fx)
    T, frames, info = g.distributed_init_ex(aop, local="odometry", align="robust")
    assert np.abs(T - fx["T_local"]).max() <= 1e-12  # O.odometry_initialization per agent
    rb = fx["robust"]
    assert np.abs(frames - rb["frames"]).max() <= 1e-10
    assert np.array_equal(info["parent"], rb["parent"])
    assert np.array_equal(info["candidates"], rb["candidates"])
    assert np.array_equal(info["inliers"], rb["inliers"])
    assert np.array_equal(info["edge_inlier"], rb["edge_inlier"])
    root = int(aop[0])
    assert np.array_equal(frames[root], np.hstack([np.eye(d), np.zeros((d, 1))]))
    assert info["iters"] == 0 and info["relres"] == 0.0


def test_robust_frames_beat_l2_on_the_corrupted_grid(H):
    fx = F.fixture3d()
    aop = fx["aop"]
    _, fr_clean, _ = F.graph_of(H, fx, clean=True).distributed_init_ex(aop, local="odometry", align="robust")
    g = F.graph_of(H, fx)
    _, fr_rob, _ = g.distributed_init_ex(aop, local="odometry", align="robust")
    _, fr_l2, _ = g.distributed_init_ex(aop, local="odometry", align="l2")
    for a in range(fx["K"]):
        if a == aop[0]:
            continue
        rr, rt = F.frame_distance(fr_rob[a], fr_clean[a])
        lr, lt = F.frame_distance(fr_l2[a], fr_clean[a])
        print(f"agent {a}: robust {rr:.4g} {rt:.4g}  l2 {lr:.4g} {lt:.4g}")
        assert rr < lr and rt < lt, (a, rr, lr, rt, lt)


def _compose_lift(T, frames, aop, Y):
    """frame o local, then YLift, in float64 with the operation order of init.cpp / graph.cpp (sums from the first
    term on, no fused multiply-add): the products are exact float64 products and the sums round as the host's."""
    d = T.shape[0]
    b = d + 1
    n = T.shape[1] // b
    P = T.reshape(d, n, b)  # [row, pose, col]
    Fp = frames[np.asarray(aop)]  # n x d x b
    W = np.zeros((d, n, b))
    for u in range(d):
        for c in range(b):
            s = Fp[:, u, d].copy() if c == d else np.zeros(n)
            for w in range(d):
                s = s + Fp[:, u, w] * P[w, :, c]
            W[u, :, c] = s
    X = np.zeros((Y.shape[0], n, b))
    for a in range(Y.shape[0]):
        acc = np.zeros((n, b))
        for u in range(d):
            acc = acc + Y[a, u] * W[u]
        X[a] = acc
    return X.reshape(Y.shape[0], n * b)


def test_defaults_reproduce_distributed_init_bitwise(H):
    g = H.Graph.grid3d(6, seed=3)
    aop = g.grid_partition(2)
    Y = O.lifting_matrix(3, 5)
    X, _, _ = g.distributed_init(aop, 5, Y, gpu=False)
    T, frames, info = g.distributed_init_ex(aop)
    assert np.array_equal(_compose_lift(T, frames, aop, Y), X)
    assert info["parent"][aop[0]] == -1 and (np.delete(info["parent"], aop[0]) >= 0).all()
    assert np.array_equal(info["candidates"], info["inliers"])


def test_odometry_needs_an_unbroken_chain(H):
    """An agent whose consecutive poses (local indices l, l + 1) are not joined by an edge has no odometry to compose:
    EINVAL naming the agent.  Interleaved agents break every chain.  The grid's sub-cubes do not: the snake order
    restricted to a sub-cube is again a path of lattice neighbours, so grid_partition(2) initialises like contiguous
    ranges (checked against the oracle's odometry_initialization through the restatement's helper)."""
    g = H.Graph.grid3d(6, seed=3)
    with pytest.raises(H.DPGOHipError, match=r"odometry of agent 0 stops at its pose 0"):
        g.distributed_init_ex((np.arange(g.n) % 4).astype(np.int32), local="odometry", align="robust")
    aop = g.grid_partition(2)
    a = g.arrays()
    T, _, info = g.distributed_init_ex(aop, local="odometry", align="robust")
    To = F.odometry_local(3, a["p1"].astype(np.int64), a["p2"].astype(np.int64), a["R"], a["t"], aop, 8)
    assert np.abs(T - To).max() <= 1e-12
    assert (info["parent"] >= 0).sum() == 7


def test_agent_with_only_outlier_closures_is_refused(H):
    """The last agent keeps two shared closures, both outliers.  Two candidate frames further apart than twice the
    threshold angle tie at their chordal midpoint, both residuals stay above the threshold, the GNC ends with both
    weights 0, the pair is skipped and the agent is never aligned.  (With many outliers the GNC locks on to whichever
    few agree by chance: nothing can tell those from inliers.)  The restatement decides that the inlier set is empty;
    the library must then refuse."""
    fx = F.fixture3d()
    aop, p1, p2 = fx["aop"], fx["p1"], fx["p2"]
    A = fx["K"] - 1
    mine = np.nonzero((aop[p1] == A) != (aop[p2] == A))[0]
    keep = np.ones(len(p1), bool)
    keep[mine[2:]] = False
    R, t = fx["R_clean"].copy(), fx["t_clean"].copy()
    rng = np.random.default_rng(3)
    for e in mine[:2]:
        R[e] = F._random_rotation(rng, 3)
        t[e] += rng.normal(0.0, 5.0, size=3)
    assert np.linalg.norm(R[mine[0]] - R[mine[1]]) > 2.0  # far more than twice 30 degrees apart
    p1, p2, R, t = p1[keep], p2[keep], R[keep], t[keep]
    rb = F.two_stage_alignment(3, p1, p2, R, t, aop, fx["K"], fx["T_local"])
    assert not rb["aligned"][A] and rb["aligned"][:A].all()
    assert list(rb["edge_inlier"][rb["edge_inlier"] != 255][-2:]) == [0, 0]
    g = H.Graph.from_arrays(3, fx["n"], p1, p2, R, t, fx["kappa"][keep], fx["tau"][keep])
    with pytest.raises(H.DPGOHipError, match=f"agent {A} was never aligned"):
        g.distributed_init_ex(aop, local="odometry", align="robust")
    # the averaging alone: both weights exactly 0, as the restatement's
    two = np.array([np.eye(3), np.diag([-1.0, -1.0, 1.0]) @ np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])])
    _, w, iters = H.robust_rotation_average(two)
    _, wr, ir = F.rotation_average(two)
    assert list(w) == [0.0, 0.0] and list(wr) == [0, 0] and iters == ir
