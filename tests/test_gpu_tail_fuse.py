"""Last tCG step folded into the retraction (tuning key TUNE_TAIL_FUSE = 14).  With the key on, the merged tCG's last
k_tcg_updir is not launched: k_retract applies eta = fma(step, delta, eta_old) from registers for the agents with a
step pending, writes their <eta_old, Hdelta> partial where k_tcg_updir would have, and does not store eta.  The same
fma sequences on the same operands, so iterates, counters, traces and the agent status are bitwise those of value 0 on
every launch path: the iterations queued at once (unsplit, and in the agent groups of TUNE_SPLIT_STREAMS), one
iteration queued ahead of a published status, the candidates of the explicit agents after a first-step prediction,
multi-Run calls and radius-shrink retries."""
import functools

import numpy as np
import pytest

from tests._common import load_meas

pytestmark = pytest.mark.gpu

TAIL_FUSE, SPLIT_STREAMS, TILE_ORDER, LOOKAHEAD, STATUS_PASS = 14, 10, 13, 7, 9
# dpgo_hip_stats columns (hip.STATS_FIELDS)
NEGCURV, EXCREGION, LCON, SCON, MAXITER, CG_STEPS, IMPLICIT = 4, 5, 6, 7, 8, 10, 11


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _partition2(g, k):
    """Two agents per axis over grid3d(k), cut after the first ceil(k / 2) planes (uneven agents for odd k), from the
    generator's pose order: plane by plane, rows and planes traversed boustrophedon."""
    i = np.arange(k ** 3)
    z, idx = i // (k * k), i % (k * k)
    idx = np.where(z & 1, k * k - 1 - idx, idx)
    y, x = idx // k, idx % k
    x = np.where(y & 1, k - 1 - x, x)
    s = (k + 1) // 2
    return (x // s + 2 * (y // s + 2 * (z // s))).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _data(k, r):
    """Graph, partition, the distributed initial guess (CG regime) and the odometry chain (boundary regime), once per
    shape; never modified."""
    from dpgo_amd import hip as H
    g = H.Graph.grid3d(k, seed=5)
    aop = _partition2(g, k)
    Y = H.lifting_matrix(3, r)
    X0, _, _ = g.distributed_init(aop, r, Y, gpu=True, rtol=1e-12, dev_layout=True)
    Xc = g.chain_init_dev_layout(r, Y)
    for a in (X0, Xc):
        a.setflags(write=False)
    return g, aop, X0, Xc


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _engine_run(hip, k, r=5, start="init", iters=40, batch_stats=None, **params):
    g, aop, X0, Xc = _data(k, r)
    e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=r, **params))
    e.set_trace(2048)
    e.set_X(Xc if start == "chain" else X0)
    status = []
    for it in range(iters):
        e.pre_exchange(it % e.num_colors)
        e.update(it % e.num_colors, None)
        if batch_stats is not None:  # cumulative counters after every batch (one colour's update)
            batch_stats.append(e.stats().sum(axis=0))
        if it % 8 == 7 or it + 1 == iters:
            rc, rd = e.status()
            status.append((rc.copy(), rd.copy()))
    X = np.zeros(X0.size)
    e.get_X_into(X)
    tr = [np.array([[rec[f] for f in hip.TRACE_FIELDS] for rec in e.get_trace(a)]) for a in range(8)]
    return X, e.stats().copy(), tr, status


def _engine_ab(hip, k, tunings=(), **kw):
    """The same engine run with TUNE_TAIL_FUSE 0 and 1 under the given process tuning keys; asserts bitwise equality
    and returns the counters."""
    keys = [TAIL_FUSE] + [key for key, _ in tunings]
    saved = {key: hip.get_tuning(key) for key in keys}
    out = []
    try:
        for key, v in tunings:
            hip.set_tuning(key, v)
        for v in (0, 1):
            hip.set_tuning(TAIL_FUSE, v)
            out.append(_engine_run(hip, k, **kw))
    finally:
        for key, v in saved.items():
            hip.set_tuning(key, v)
    (X, stats, tr, status), (X1, stats1, tr1, status1) = out
    assert sum(len(t) for t in tr) > 0  # the trace is on and recorded something
    assert np.array_equal(_bits(X), _bits(X1))
    assert np.array_equal(stats, stats1)
    for a in range(8):
        assert tr[a].shape == tr1[a].shape, a
        assert np.array_equal(_bits(tr[a]), _bits(tr1[a])), a
    assert len(status) == len(status1)
    for (rc, rd), (rc1, rd1) in zip(status, status1):
        assert np.array_equal(_bits(rc), _bits(rc1))
        assert np.array_equal(rd, rd1)
    print("stats sum", dict(zip(hip.STATS_FIELDS, stats.sum(axis=0).tolist())))
    return stats


# k = 7: colour launches of fewer than 8 tiles and agents smaller than two tiles; 11: uneven agents and partial last
# tiles.  split 0: the unsplit queued-ahead path the 1M-pose flagship takes (these batches are split by default).
# inner: the engine's default of 10, which these small grids' tCG rarely reaches (it stops by the residual test after
# about 7: every agent takes today's path through the fused kernel), and 4, where most tCGs end at the last iteration
# with a step pending.
@pytest.mark.parametrize("inner", [None, 4])
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("split", [None, 0])
@pytest.mark.parametrize("k", [7, 11])
def test_tail_fuse_engine_bitwise(hip, k, split, order, inner):
    tunings = [(TILE_ORDER, order)] + ([(SPLIT_STREAMS, split)] if split is not None else [])
    kw = {} if inner is None else {"max_inner": inner}
    stats = _engine_ab(hip, k, tunings, acceleration=1, **kw)
    if inner is not None:
        assert stats[:, MAXITER].sum() > 0  # some tCG reached its last iteration: the fused tail ran


def test_tail_fuse_no_acceleration(hip):
    stats = _engine_ab(hip, 11, acceleration=0, max_inner=4)
    assert stats[:, MAXITER].sum() > 0


def test_tail_fuse_one_ahead(hip):
    """One iteration queued ahead of the status the host waits for (TUNE_TCG_LOOKAHEAD = 1)."""
    stats = _engine_ab(hip, 11, [(LOOKAHEAD, 1)], acceleration=1, max_inner=4)
    assert stats[:, MAXITER].sum() > 0
    _engine_ab(hip, 11, [(LOOKAHEAD, 1)], acceleration=1)


def test_tail_fuse_mixed_exit_kinds(hip):
    """From the odometry chain the first iterations end every tCG at its first step on the boundary (eta implicit);
    about 80 to 160 iterations on (max_inner = 6) the agents pass into the CG regime one by one, and one colour's
    batch holds agents that exit at the first step (implicit), agents that stop at a later step before the last
    iteration (a boundary step after CG steps, or the residual test; no step pending at the tail) and agents that run to
    MAXITER (a step pending).  The counters show that at least one batch held all three kinds."""
    per_batch = []
    stats = _engine_ab(hip, 11, start="chain", iters=160, acceleration=1, max_inner=6, batch_stats=per_batch)
    tot = stats.sum(axis=0)
    assert tot[IMPLICIT] > 0
    assert tot[MAXITER] > 0
    assert tot[LCON] + tot[SCON] + tot[NEGCURV] + tot[EXCREGION] - tot[IMPLICIT] > 0
    per_batch = np.array(per_batch[:160], np.int64)  # value 0's run (value 1's counters are asserted equal)
    d = np.diff(per_batch, axis=0, prepend=0)
    early = d[:, LCON] + d[:, SCON] + d[:, NEGCURV] + d[:, EXCREGION] - d[:, IMPLICIT]  # stopped with eta explicit
    mixed = (d[:, IMPLICIT] > 0) & (d[:, MAXITER] > 0) & (early > 0)
    print("batches with all three exit kinds:", int(mixed.sum()), "of", len(d))
    assert mixed.any()


@pytest.mark.parametrize("split", [None, 0])
@pytest.mark.parametrize("inner", [1, 2])
def test_tail_fuse_iteration_limits(hip, inner, split):
    """max_inner = 1: the first iteration is also the last (eta_old = 0, not read); 2: one ordinary iteration."""
    tunings = [(SPLIT_STREAMS, split)] if split is not None else []
    stats = _engine_ab(hip, 11, tunings, acceleration=1, max_inner=inner)
    assert stats[:, MAXITER].sum() > 0
    _engine_ab(hip, 11, tunings, start="chain", iters=16, acceleration=1, max_inner=inner)


def test_tail_fuse_status_pass(hip):
    """The agent status by its own pass (TUNE_STATUS_PASS = 1) instead of folded into the retraction."""
    stats = _engine_ab(hip, 11, [(STATUS_PASS, 1)], acceleration=1, max_inner=4)
    assert stats[:, MAXITER].sum() > 0


@pytest.mark.parametrize("fmt", ["edges", "bsr"])
def test_tail_fuse_engine_r3(hip, fmt):
    stats = _engine_ab(hip, 7, r=3, acceleration=1, max_inner=4,
                       q_format=hip.QFMT_EDGES if fmt == "edges" else hip.QFMT_BSR)
    assert stats[:, MAXITER].sum() > 0


def test_tail_fuse_engine_bsr(hip):
    stats = _engine_ab(hip, 11, acceleration=1, max_inner=4, q_format=hip.QFMT_BSR)
    assert stats[:, MAXITER].sum() > 0


@pytest.mark.parametrize("fmt", ["edges", "bsr"])
@pytest.mark.parametrize("r", [3, 5])
def test_tail_fuse_single_robot(hip, r, fmt):
    """dpgo_hip_optimize on smallGrid3D, 10 outer and 50 inner iterations: a multi-iteration Run (x1 moves, accepted
    candidates are copied) with radius-shrink retries, one agent."""
    from oracle import dpgo_oracle as O
    meas = load_meas("smallGrid3D")
    d, n = meas.d, meas.num_poses
    Q = O.connection_laplacian(meas, n)
    X0 = O.lifting_matrix(d, r) @ O.chordal_initialization(d, n, meas)
    out = []
    for inner in (50, 3):  # 3: every tCG ends at its last iteration
        for v in (0, 1):
            H = hip.Problem(n, d, r)
            H.set_tuning(TAIL_FUSE, v)
            if fmt == "edges":
                H.set_Q_edges(0, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau, meas.weight)
            else:
                H.set_Q_scipy(0, Q)
            H.set_trace(4096)
            p = hip.default_params(tr_iterations=10, tr_tolerance=1e-1, tr_initial_radius=10.0, tr_max_inner=inner,
                                   precon=hip.PRECON_BLOCK_JACOBI)
            Xh, rh = H.optimize(X0, p)
            tr = np.array([[rec[f] for f in hip.TRACE_FIELDS] for rec in H.get_trace(0)])
            out.append((Xh, rh, tr, H.stats()))
        (X, res, tr, st), (X1, res1, tr1, st1) = out[-2:]
        print("inner", inner, st[0])
        assert len(tr) > 3
        assert np.array_equal(_bits(X), _bits(X1))
        assert tr.shape == tr1.shape and np.array_equal(_bits(tr), _bits(tr1))
        assert st == st1
        for key in res[0]:
            if key != "elapsedMs":
                assert np.array_equal(_bits(res[0][key]), _bits(res1[0][key])), key
    assert out[2][3][0]["MAXITER"] > 0
