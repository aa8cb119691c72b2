"""GPU parity of the multi-agent RBCD engine (include/dpgo_rbcd.h) against the PGOAgent
restatement in the oracle, under the same colour-class schedule."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests._common import load_meas, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _graph_from_meas(H, meas):
    return H.Graph.from_arrays(meas.d, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t,
                               meas.kappa, meas.tau)


def _run_engine(H, g, agent_of_pose, num_agents, X0, iters, accel, r, **kw):
    e = H.Rbcd(g, agent_of_pose, np.zeros(num_agents, np.int32), 0, 1,
               H.rbcd_params(r=r, acceleration=int(accel), **kw))
    e.set_X(X0)
    for it in range(iters):
        c = it % e.num_colors
        e.pre_exchange(c)
        e.update(c, None)
    out = np.zeros(X0.size)
    e.get_X_into(out)
    return H.from_dev_layout(out, r), e


@pytest.mark.parametrize("accel", [False, True])
def test_grid_cubes_match_oracle(hip, accel):
    k, A, r = 6, 2, 5  # 216 poses, 8 cube agents
    g = hip.Graph.grid3d(k, seed=3)
    a = g.arrays()
    meas = O.Measurements(3, np.zeros(g.m, np.int64), np.zeros(g.m, np.int64), a["p1"].astype(np.int64),
                          a["p2"].astype(np.int64), a["R"], a["t"], a["kappa"], a["tau"], np.ones(g.m), g.n)
    aop = g.grid_partition(A)
    X0 = g.chain_init(r, O.lifting_matrix(3, r))
    iters = 6
    Xh, e = _run_engine(hip, g, aop, A ** 3, X0, iters, accel, r)
    assert e.num_colors == 2
    Xo, colors = O.colour_rbcd(meas, aop, A ** 3, X0, iters, r, acceleration=accel)
    assert list(e.color_of_agent) == colors
    assert rel(Xh, Xo) <= 1e-9
    f0 = O.central_cost(meas, X0)
    assert O.central_cost(meas, Xh) < f0


def test_contiguous_partition_smallgrid(hip):
    """C1 data (smallGrid3D, 5 robots, contiguous ranges as examples/MultiRobotExample.cpp:73-90)."""
    meas = load_meas("smallGrid3D")
    r = 5
    n = meas.num_poses
    aop = np.minimum(np.arange(n) // (n // 5), 4).astype(np.int32)
    X0 = O.lifting_matrix(3, r) @ O.chordal_initialization(3, n, meas)
    g = _graph_from_meas(hip, meas)
    Xh, e = _run_engine(hip, g, aop, 5, X0, 8, True, r)
    Xo, _ = O.colour_rbcd(meas, aop, 5, X0, 8, r, acceleration=True)
    assert rel(Xh, Xo) <= 1e-9


def test_laplacian_and_reader(hip):
    import os
    meas = load_meas("smallGrid3D")
    g = _graph_from_meas(hip, meas)
    rp, col, blk = g.laplacian_bsr()
    import scipy.sparse as sp
    Q = O.connection_laplacian(meas, meas.num_poses)
    Qb = sp.bsr_matrix((blk.reshape(-1, 4, 4).transpose(0, 2, 1), col, rp), shape=Q.shape)
    assert abs(Qb - Q).max() <= 1e-12 * abs(Q).max()


@pytest.mark.parametrize("qfmt", ["edges", "bsr"])
def test_grid_cubes_exact_precon(hip, qfmt):
    """The engine with the reference's exact preconditioner (per-agent factor of Q + 0.1 I), Nesterov,
    both device forms of Q, against the oracle's colour schedule with the exact preconditioner."""
    k, A, r = 6, 2, 5
    g = hip.Graph.grid3d(k, seed=3)
    a = g.arrays()
    meas = O.Measurements(3, np.zeros(g.m, np.int64), np.zeros(g.m, np.int64), a["p1"].astype(np.int64),
                          a["p2"].astype(np.int64), a["R"], a["t"], a["kappa"], a["tau"], np.ones(g.m), g.n)
    aop = g.grid_partition(A)
    X0 = g.chain_init(r, O.lifting_matrix(3, r))
    Xh, e = _run_engine(hip, g, aop, A ** 3, X0, 6, True, r, precon=hip.PRECON_EXACT,
                        q_format=hip.QFMT_EDGES if qfmt == "edges" else hip.QFMT_BSR)
    Xo, _ = O.colour_rbcd(meas, aop, A ** 3, X0, 6, r, acceleration=True, precon=O.PRECON_EXACT)
    assert rel(Xh, Xo) <= 1e-9


def _grid_with_outliers(hip, k, seed, frac, rng_seed):
    """grid3d edges with a fraction of the loop closures (non-consecutive poses) corrupted."""
    g0 = hip.Graph.grid3d(k, seed=seed)
    a = g0.arrays()
    p1, p2 = a["p1"].astype(np.int64), a["p2"].astype(np.int64)
    R, t = a["R"].copy(), a["t"].copy()
    rng = np.random.default_rng(rng_seed)
    lc = np.nonzero(np.abs(p2 - p1) != 1)[0]
    bad = rng.choice(lc, size=max(1, int(frac * len(lc))), replace=False)
    t[bad] += rng.normal(0.0, 5.0, size=(len(bad), 3))
    g = hip.Graph.from_arrays(3, g0.n, p1, p2, R, t, a["kappa"], a["tau"])
    meas = O.Measurements(3, np.zeros(len(p1), np.int64), np.zeros(len(p1), np.int64), p1, p2, R, t,
                          a["kappa"], a["tau"], np.ones(len(p1)), g0.n)
    return g, g0, meas


@pytest.mark.parametrize("accel", [False, True])
@pytest.mark.parametrize("robust", ["GNC_TLS", "TLS", "Huber", "GM", "L1"])
def test_robust_reweighting_matches_oracle(hip, accel, robust):
    """Robust costs (GNC_TLS is the reference default) through two reweightings
    (robust_opt_inner_iters = 3: iterations 2 and 5; src/PGOAgent.cpp:642-718, 1174-1244;
    src/DPGO_robust.cpp): on-device residuals / weights / Q and G rebuild vs the oracle's PGOAgent
    colour schedule, with 10 % corrupted loop closures.  (Long runs on outlier-heavy data drift apart
    through discontinuous RTR/tCG branch decisions, for L2 as well, so the reweighting is exercised
    early.)"""
    k, A, r = 6, 2, 5
    g, g0, meas = _grid_with_outliers(hip, k, 3, 0.1, 7)
    aop = g0.grid_partition(A)
    X0 = g0.chain_init(r, O.lifting_matrix(3, r))  # odometry edges are uncorrupted
    iters = 6
    Xh, e = _run_engine(hip, g, aop, A ** 3, X0, iters, accel, r, robust_cost=hip.ROBUST[robust],
                        robust_opt_inner_iters=3)
    Xo, _ = O.colour_rbcd(meas, aop, A ** 3, X0, iters, r, acceleration=accel, robust=robust,
                          robust_opt_inner_iters=3)
    assert rel(Xh, Xo) <= 1e-9
    # the reweighting changed the solution (it is not the L2 trajectory)
    Xl, _ = O.colour_rbcd(meas, aop, A ** 3, X0, iters, r, acceleration=accel, robust="L2")
    assert rel(Xo, Xl) > 1e-6


@pytest.mark.parametrize("name", ["city10000", "kitti_00"])
def test_contiguous_partition_2d_eight_agents(hip, name):
    """BASELINE configs[2]: city10000 / kitti_00 partitioned into 8 agents (contiguous ranges,
    examples/MultiRobotExample.cpp:73-90), Nesterov on, 2D (d = 2), r = 5, from the chordal
    initialisation; the engine against the oracle's PGOAgent colour schedule."""
    meas = load_meas(name)
    r, K, iters = 5, 8, 6
    n = meas.num_poses
    aop = np.minimum(np.arange(n) // (n // K), K - 1).astype(np.int32)
    X0 = O.lifting_matrix(2, r) @ O.chordal_initialization(2, n, meas)
    g = _graph_from_meas(hip, meas)
    Xh, e = _run_engine(hip, g, aop, K, X0, iters, True, r)
    Xo, colors = O.colour_rbcd(meas, aop, K, X0, iters, r, acceleration=True)
    assert list(e.color_of_agent) == colors
    assert rel(Xh, Xo) <= 1e-9
    # measured: X agrees to ~1e-14 relative; the central cost is ill-conditioned in X on kitti_00
    # (translations ~2e3 against f ~ 80: a 2e-11 absolute X difference moves f by ~1e-9 relative)
    assert abs(O.central_cost(meas, Xh) - O.central_cost(meas, Xo)) <= 1e-8 * O.central_cost(meas, Xo)


@pytest.mark.parametrize("accel,robust", [(False, "L2"), (True, "L2"), (False, "GNC_TLS"), (True, "GNC_TLS")])
def test_greedy_selection_matches_example(hip, accel, robust):
    """The example's greedy schedule (examples/MultiRobotExample.cpp:243-256) driven through the engine: each round
    one agent is optimised (dpgo_rbcd_set_selected; every other agent runs iterate(false)), and the next one is the
    argmax of the per-agent |RieGrad| from dpgo_rbcd_central_eval.  The selected robots, the gradient norms and the
    final X equal the oracle's serialized restatement of the example (smallGrid3D, 5 contiguous robots,
    block-Jacobi).  GNC_TLS (reweighting every 3 iterations): only the selected robot receives its neighbours'
    poses, so every other robot's reweighting of a shared loop closure reads the pose it received when it was last
    selected (PGOAgent::updateLoopClosuresWeights, src/PGOAgent.cpp:1201-1235) -- the engine's neighbour
    dictionaries."""
    meas = load_meas("smallGrid3D")
    r, R, iters = 5, 5, 20
    n = meas.num_poses
    X0 = O.lifting_matrix(3, r) @ O.chordal_initialization(3, n, meas)
    log, Xo = O.multi_robot_example(meas, R, r=r, num_iters=iters, acceleration=accel, robust=robust,
                                    precon=O.PRECON_BLOCK_JACOBI, X_init=X0, robust_opt_inner_iters=3)
    _, robot_of, _, _ = O.partition_contiguous(meas, n, R)
    g = _graph_from_meas(hip, meas)
    e = hip.Rbcd(g, robot_of.astype(np.int32), np.zeros(R, np.int32), 0, 1,
                 hip.rbcd_params(r=r, acceleration=int(accel), precon=hip.PRECON_BLOCK_JACOBI,
                                 robust_cost=hip.ROBUST[robust], robust_opt_inner_iters=3))
    e.set_X(X0)
    sel, got = 0, []
    for it in range(len(log)):
        mask = np.zeros(R, np.int32)
        mask[sel] = 1
        e.set_selected(mask)
        c = int(e.color_of_agent[sel])
        e.pre_exchange(c)
        e.update(c, None)
        _, gn2 = e.central_eval()
        got.append((sel, float(np.sqrt(gn2.sum()))))
        sel = int(np.argmax(gn2))
    assert [s for s, _ in got] == [s for _, s, _, _ in log]
    for (_, gg), (_, _, _, go) in zip(got, log):
        assert abs(gg - go) <= 1e-8 * max(go, 1.0), (gg, go)
    Xd = np.zeros(X0.size)
    e.get_X_into(Xd)
    assert rel(hip.from_dev_layout(Xd, r), Xo) <= 1e-9
