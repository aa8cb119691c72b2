"""Measurement weights and known inliers set into the RBCD engine (dpgo_rbcd_set_weights / _dev, k_set_weights, the
fixed-edge rule of k_gnc_weights and k_conv_ratio, dpgo_rbcd_central_eval_ex) on the 650-pose robust case
(tests/_robust.robust_case) with the weights W(d) of tests/_weights.py, whose references tests/test_weights_reference.py
checks on the CPU.

1  round trip and refusals;
2  the weighted evaluation against Graph.edge_errors and against the oracle's connection Laplacian, all 13 (d, r);
3  the trajectory against the oracle's Agents run on Measurements carrying W(d);
4  known inliers against the np.longdouble model of tests/_weights.py, ready against its ratios, release of the flags;
5  the exact preconditioner follows the weights (against a fresh engine on a graph with kappa, tau scaled on the host);
6  the device-pointer entry against the host one;
7  two ranks against one;
8  PCM's mask handed over as weights and flags.

Bars: evaluations 1e-12 relative (VALUE_BAR); weights as test_gpu_robust.check_weights; X against the oracle
max(1e-9, 2 x twin) with twin (the oracle against its own run started 1e-16 away) asserted <= 1e-8.

Measured on an MI355X: (2) f against edge_errors and against 1/2 <Q_W, X^T X> <= 7.3e-16, |RieGrad|^2 agent by agent
<= 1.1e-14 (6.8e-16 as a vector) over the 13 shapes, L2 and GNC_TLS alike.  (3) X 1.6e-13 .. 9.8e-13 at (3, 4)
(twin 8.8e-15 .. 5.9e-14) and 7.1e-12 .. 2.8e-10 at (2, 4) (twin 2.4e-11 .. 3.3e-10); weights <= 9.4e-11, under L2
identical; the weighted oracle ends 0.10 .. 0.19 from the unit-weight one.  (4) device against np.longdouble <= 2.7e-14
(float64 numpy's own <= 2.3e-14), 227 reweighted and 434 fixed at the first reweighting; ratios NaN, 0.8652, NaN, 0.7619,
0.8026, 0.6481, 0.5023, NaN at d = 3 (agent 0's single loop closure is st.lc[0], which the [::3] rule fixes); 242 / 228 released weights rewritten.
(5) bitwise equal with both preconditioners, tw 2.1e-14.  (8) 71 rejected closures held at 0, 17 of 49 accepted and
115 of 208 private ones moved off 1; the weighted cost falls from 430 to 9.
"""
import math
import os
import socket

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _pcm as P
from tests import _robust as RB
from tests import _weights as WT
from tests._common import rel
from tests.test_gpu_robust import (FIRST, K, PARITY, PARITY_ITERS, SCHEDULE, SHAPES, VALUE_BAR, _engine, _model_params,
                                    _oracle_counters, _oracle_params, _step, _structure, _weights, _X, check_weights)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1, "no gfx950 device"
    return H


def _flat(e, g, r):
    out = np.full(g.n * (g.d + 1) * r, np.nan)
    e.get_X_into(out)
    assert not np.isnan(out).any()
    return out


def _same_eval(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("kind", ["L2", "GNC_TLS"])
def test_round_trip_and_refusals(hip, kind):
    """get_weights returns what set_weights set, bit for bit, odometry included; a NaN, an infinite or a negative entry
    raises and leaves the weights and both evaluations as they were; so does an engine that stores Q as BSR."""
    d, r = 3, 5
    meas, aop, T = RB.robust_case(d)
    st, _ = _structure(d)
    e, g = _engine(hip, d, r, kind, acceleration=0)
    assert np.all(_weights(e, g) == 1.0)
    w = WT.W(d)
    assert np.any(w[st.owner < 0] != 1.0)
    e.set_weights(w)
    assert np.array_equal(_weights(e, g), w)
    unit, wtd = e.central_eval(), e.central_eval(weighted=True)
    assert unit[0] != wtd[0]
    odo, lc = int(np.nonzero(st.owner < 0)[0][3]), int(st.lc[7])
    for k in (odo, lc):
        for bad in (float("nan"), float("inf"), -1e-3):
            wb = np.array(w)
            wb[k] = bad
            with pytest.raises(hip.DPGOHipError):
                e.set_weights(wb, fixed=np.ones(g.m, np.uint8))
            assert np.array_equal(_weights(e, g), w)
            assert _same_eval(e.central_eval(), unit) and _same_eval(e.central_eval(weighted=True), wtd)
    with pytest.raises(ValueError):
        e.set_weights(w[:-1])
    # a second call replaces the first
    w2 = np.array(w[::-1])
    e.set_weights(w2)
    assert np.array_equal(_weights(e, g), w2)
    assert _same_eval(e.central_eval(), unit)
    if kind == "L2":
        b = hip.Rbcd(g, aop, np.zeros(K, np.int32), 0, 1, hip.rbcd_params(r=r, q_format=hip.QFMT_BSR))
        b.set_X(O.lifting_matrix(d, r) @ T)
        before = b.central_eval()
        with pytest.raises(hip.DPGOHipError):
            b.set_weights(w)
        assert np.all(_weights(b, g) == 1.0) and _same_eval(b.central_eval(), before)
        assert _same_eval(b.central_eval(weighted=True), before)


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("kind", ["L2", "GNC_TLS"])
@pytest.mark.parametrize("d,r", SHAPES)
def test_weighted_evaluation(hip, d, r, kind):
    """central_eval(weighted=True) after set_weights(W): f against Graph.edge_errors' weighted cost and against
    1/2 <Q_W, X^T X> of the oracle's connection Laplacian, the per-agent |RieGrad|^2 against the oracle's tangent
    projection of X Q_W, all at 1e-12 relative; the unit-weight evaluation is bitwise what it was before the call."""
    meas, aop, T = RB.robust_case(d)
    w = WT.W(d)
    e, g = _engine(hip, d, r, kind, acceleration=0)
    before = e.central_eval()
    assert _same_eval(e.central_eval(weighted=True), before)  # nothing set yet: the same problem
    e.set_weights(w)
    assert _same_eval(e.central_eval(), before)
    f, gn = e.central_eval(weighted=True)
    X = O.lifting_matrix(d, r) @ T
    cost = g.edge_errors(_flat(e, g, r), r, w=w)["cost"]
    Q = O.connection_laplacian(WT.weighted(meas, w), meas.num_poses)
    XQ = np.asarray((Q @ X.T).T)
    f_ref = 0.5 * float(np.sum(XQ * X))
    RG = O.tangent_project(X, XQ, d)
    b = d + 1
    g_ref = np.array([float(np.sum(RG[:, np.repeat(aop == a, b)] ** 2)) for a in range(K)])
    assert np.all(g_ref > 0.0)
    e_cost, e_q, e_g = abs(f - cost) / cost, abs(f - f_ref) / f_ref, float(np.max(np.abs(gn - g_ref) / g_ref))
    print(f"{kind} d={d} r={r}: f {f:.12g} (unit {before[0]:.12g}); against edge_errors {e_cost:.2e}, against "
          f"1/2<Q_W, X^T X> {e_q:.2e}, |RieGrad|^2 agent by agent {e_g:.2e} (as a vector {rel(gn, g_ref):.2e})")
    assert abs(f - before[0]) > 1e-3 * before[0]
    assert e_cost <= VALUE_BAR and e_q <= VALUE_BAR
    assert e_g <= VALUE_BAR  # every agent relative to its own value


# ------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("accel", [False, True])
@pytest.mark.parametrize("kind", ["L2", "GNC_TLS"])
@pytest.mark.parametrize("d,r", [(3, 4), (2, 4)])
def test_trajectory_matches_weighted_oracle(hip, d, r, kind, accel):
    """PARITY_ITERS iterations after set_weights(W(d)) against the oracle's Agents on Measurements whose weight is
    W(d): colours and solver counters equal, every reported weight within 1e-9, X within max(1e-9, 2 x twin)."""
    meas, aop, T = RB.robust_case(d)
    st, _ = _structure(d)
    w0 = WT.W(d)
    X0 = O.lifting_matrix(d, r) @ T
    kw = PARITY.get(kind, {})

    def oracle(X, ags=None, trace=None):
        return O.colour_rbcd(WT.weighted(meas, w0), aop, K, X, PARITY_ITERS[d], r, acceleration=accel, robust=kind,
                             robust_opt_inner_iters=3, agents_out=ags, trace=trace, **_oracle_params(kw))

    ags, trace = [], []
    Xo, colors = oracle(X0, ags, trace)
    noise = np.random.default_rng(3).standard_normal(X0.shape)
    twin = rel(oracle(X0 * (1.0 + 1e-16 * noise))[0], Xo)
    print(f"{kind} d={d} r={r} accel={accel}: weighted oracle vs its perturbed twin {twin:.2e}")
    assert twin <= 1e-8
    e, g = _engine(hip, d, r, kind, acceleration=int(accel), robust_opt_inner_iters=3, **kw)
    e.set_weights(w0)
    for it in range(PARITY_ITERS[d]):
        _step(e, it)
    assert list(e.color_of_agent) == colors
    err = rel(_X(hip, e, g, r), Xo)
    w, (wo, other) = _weights(e, g), WT.oracle_weights_both(ags, meas, aop)
    werr = float(np.max(np.abs(w - wo)))
    unit = rel(Xo, O.colour_rbcd(RB.fresh(meas), aop, K, X0, PARITY_ITERS[d], r, acceleration=accel, robust=kind,
                                 robust_opt_inner_iters=3, **_oracle_params(kw))[0])
    print(f"    engine vs oracle: X {err:.2e} (bar {max(1e-9, 2 * twin):.2e}), weights {werr:.2e}; the weighted "
          f"run is {unit:.2f} from the unit-weight one")
    assert unit >= 1e-3  # the oracle's two runs (CPU): the weights move X by orders of magnitude more than any bar here
    assert err <= max(1e-9, 2 * twin)
    assert werr <= 1e-9
    assert np.array_equal(w[st.owner < 0], w0[st.owner < 0]) and np.array_equal(other[st.shared], w0[st.shared])
    if kind == "L2":
        assert np.array_equal(w, w0)
    else:
        assert np.any(w[st.lc] != w0[st.lc])
    calls, runs, inner = _oracle_counters(trace, K)
    stats = e.stats()
    assert list(stats[:, 0]) == list(calls)
    assert list(stats[:, 2]) == list(runs)
    assert list(stats[:, 3]) == list(inner)


# ------------------------------------------------------------------------------------------ 4
_cache = {}
INLIER_RUN = dict(acceleration=0, robust_opt_inner_iters=1, rel_change_tol=1e300)


def _fixed(d):
    meas, _, _ = RB.robust_case(d)
    st, _ = _structure(d)
    return WT.mask(st, meas.m)


def _as_robust(w, w0, st):
    """w with the odometry at 1 once it is bitwise what was set: the form test_gpu_robust.check_weights takes."""
    odo = st.owner < 0
    assert np.array_equal(w[odo], w0[odo]), "odometry weights moved"
    out = np.array(w)
    out[odo] = 1.0
    return out


def _as_robust_rec(rec, st):
    out = dict(rec)
    out["w"] = np.array(rec["w"])
    out["w"][st.owner < 0] = 1.0
    return out


def _inlier_schedule(hip, d, r, threshold=None):
    """GNC_TLS from W(d) with the mask over 2 C + 1 iterations: X, weights and ready after every iteration."""
    meas, aop, T = RB.robust_case(d)
    kw = dict(INLIER_RUN, **SCHEDULE)
    if threshold is not None:
        kw["min_convergence_ratio"] = threshold
    e, g = _engine(hip, d, r, "GNC_TLS", **kw)
    e.set_weights(WT.W(d), _fixed(d))
    hist, ws, ready = [_X(hip, e, g, r)], [], []
    for it in range(2 * e.num_colors + 1):
        _step(e, it)
        hist.append(_X(hip, e, g, r))
        ws.append(_weights(e, g))
        ready.append(e.status()[1].copy())
    return e, g, hist, ws, ready


def _inlier_model(hip, d, r):
    if (d, r) not in _cache:
        meas, aop, _ = RB.robust_case(d)
        st, colors = _structure(d)
        e, g, hist, ws, ready = _inlier_schedule(hip, d, r)
        p = _model_params(SCHEDULE)
        args = (meas, aop, colors, "GNC_TLS", hist, 1, WT.W(d), _fixed(d), p)
        _cache[(d, r)] = (e, g, hist, ws, WT.run_model(*args), WT.run_model(*args, dtype=np.float64), p)
    return _cache[(d, r)]


@pytest.mark.parametrize("d,r", SHAPES)
def test_known_inliers_first_reweighting(hip, d, r):
    """robust_opt_inner_iters = 2: iteration 1 reweights at X0.  The fixed loop closures keep W(d) bitwise, the free
    ones take w(r(X0)) unless their owner has no neighbour pose yet (then W(d) too), odometry keeps what was set."""
    meas, aop, T = RB.robust_case(d)
    st, colors = _structure(d)
    w0, fixed = WT.W(d), _fixed(d)
    kw = FIRST["GNC_TLS"]
    p = _model_params(kw)
    e, g = _engine(hip, d, r, "GNC_TLS", acceleration=0, robust_opt_inner_iters=2, **kw)
    e.set_weights(w0, fixed)
    _step(e, 0)
    w = _weights(e, g)
    X0 = O.lifting_matrix(d, r) @ T
    ref = WT.run_model(meas, aop, colors, "GNC_TLS", [X0, X0], 2, w0, fixed, p)[0]
    twin = WT.run_model(meas, aop, colors, "GNC_TLS", [X0, X0], 2, w0, fixed, p, np.float64)[0]
    assert np.array_equal(w[fixed], w0[fixed])
    moved = ~np.isnan(ref["res"])
    assert moved.sum() >= 100 and not moved[fixed[st.lc]].any()
    assert np.any(w[st.lc][moved] != w0[st.lc][moved])
    worst, dist, near = check_weights("GNC_TLS", _as_robust(w, w0, st), _as_robust_rec(ref, st),
                                      _as_robust_rec(twin, st), st, p, f"d={d} r={r}")
    print(f"d={d} r={r}: max |w - w_longdouble| = {worst:.2e}, float64 numpy's own {dist:.2e}, {near} on a threshold, "
          f"{int(moved.sum())} reweighted, {int(fixed.sum())} fixed")


@pytest.mark.parametrize("d,r", [(3, 5), (2, 3)])
def test_known_inliers_along_the_schedule(hip, d, r):
    """Every iteration's weights against the model on the engine's own history; the fixed edges keep their set weight
    bitwise throughout; a later set_weights without flags releases them."""
    st, colors = _structure(d)
    w0, fixed = WT.W(d), _fixed(d)
    e, g, hist, ws, model, twin, p = _inlier_model(hip, d, r)
    for t, w in enumerate(ws):
        assert np.array_equal(w[fixed], w0[fixed]), f"iteration {t + 1}: a fixed edge was rewritten"
        worst, dist, near = check_weights("GNC_TLS", _as_robust(w, w0, st), _as_robust_rec(model[t], st),
                                          _as_robust_rec(twin[t], st), st, p, f"d={d} r={r} iteration {t + 1}")
        print(f"d={d} r={r} iteration {t + 1}: max |w - w_longdouble| = {worst:.2e}, float64 numpy's own {dist:.2e}, "
              f"{near} on a threshold")
    free = st.lc[~fixed[st.lc]]
    assert np.any(ws[-1][free] != w0[free])
    # release: the same weights without flags, one more iteration (it reweights: robust_opt_inner_iters = 1)
    held = st.lc[fixed[st.lc]]
    between = held[(w0[held] > 0.0) & (w0[held] < 1.0)]
    assert len(between) >= 50
    e.set_weights(ws[-1])
    assert np.array_equal(_weights(e, g), ws[-1])
    _step(e, len(ws))
    after = _weights(e, g)
    changed = int(np.sum(after[between] != w0[between]))
    print(f"    released: {changed} of {len(between)} formerly fixed weights inside (0, 1) rewritten")
    assert changed >= len(between) // 2


@pytest.mark.parametrize("d,r", [(3, 5), (2, 3)])
def test_ready_follows_the_ratio_of_the_free_copies(hip, d, r):
    """rel_change_tol = 1e300: ready[a] == not (ratio_a < threshold) with the model's ratios over the non-fixed copies,
    one engine per threshold; the agent whose every copy is fixed (0/0 = NaN) is ready at every threshold, like the
    agent without loop closures."""
    st, colors = _structure(d)
    _, _, _, _, model, _, _ = _inlier_model(hip, d, r)
    final = model[-1]["ratio"]
    assert math.isnan(final[WT.MASK_AGENT]) and math.isnan(final[RB.EXTRA_AGENT])
    thresholds = RB.thresholds_from(final)
    print(f"d={d} r={r}: ratios {['%.4f' % x for x in final]}, {len(thresholds)} thresholds")
    assert len(thresholds) >= 5
    for thr in thresholds:
        _, _, _, _, ready = _inlier_schedule(hip, d, r, thr)
        for t, rd in enumerate(ready):
            for a in range(K):
                if model[t]["selected"][a]:
                    want = RB.ready_from_ratio(model[t]["ratio"][a], thr)
                    assert bool(rd[a]) == want, (f"threshold {thr!r}, iteration {t + 1}, agent {a}: ready {rd[a]}, "
                                                 f"model ratio {model[t]['ratio'][a]!r}")
        assert bool(ready[-1][WT.MASK_AGENT]) and bool(ready[-1][RB.EXTRA_AGENT])


# ------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("precon", ["exact", "block_jacobi"])
def test_preconditioner_follows_the_weights(hip, precon):
    """d = 3, weights uniform(0.25, 1) on every edge.  Engine A: set_weights(w).  Engine B: a fresh engine on the graph
    with kappa and tau multiplied by w on the host.  After three colour steps X agrees to max(1e-9, 2 x tw), tw the
    distance between two engines of kind B started 1e-16 apart."""
    d, r = 3, 5
    meas, aop, T = RB.robust_case(d)
    w = np.random.default_rng(55).uniform(0.25, 1.0, meas.m)
    pc = hip.PRECON_EXACT if precon == "exact" else hip.PRECON_BLOCK_JACOBI
    X0 = O.lifting_matrix(d, r) @ T
    ranks = np.zeros(K, np.int32)

    def run(kappa, tau, X, weights=None):
        g = hip.Graph.from_arrays(d, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t, kappa, tau)
        e = hip.Rbcd(g, aop, ranks, 0, 1, hip.rbcd_params(r=r, precon=pc))
        e.set_X(X)
        if weights is not None:
            e.set_weights(weights)
        for it in range(3):
            _step(e, it)
        return _X(hip, e, g, r), e.stats()

    Xa, sa = run(meas.kappa, meas.tau, X0, w)
    Xb, sb = run(meas.kappa * w, meas.tau * w, X0)
    noise = np.random.default_rng(3).standard_normal(X0.shape)
    Xt, _ = run(meas.kappa * w, meas.tau * w, X0 * (1.0 + 1e-16 * noise))
    Xu, _ = run(meas.kappa, meas.tau, X0)
    tw, err = rel(Xt, Xb), rel(Xa, Xb)
    print(f"{precon}: set_weights vs host-scaled graph {err:.2e} (bitwise: {np.array_equal(Xa, Xb)}), twin {tw:.2e}, "
          f"unit-weight run {rel(Xu, Xb):.2e} away")
    assert tw <= 1e-8
    assert rel(Xu, Xb) > 1e-3  # the weights matter over three steps
    assert err <= max(1e-9, 2 * tw)
    assert np.array_equal(sa[:, 0], sb[:, 0])  # the same agents were updated the same number of times


# ------------------------------------------------------------------------------------------ 6
def test_device_entry_equals_host_entry(hip):
    """set_weights_dev on torch tensors -- and on a weight tensor offset by 8 bytes -- gives bitwise the host call's
    get_weights and the same X and weights after two reweighting steps."""
    import torch
    d, r = 3, 5
    w0, fixed = WT.W(d), _fixed(d)
    kw = dict(INLIER_RUN, **SCHEDULE)

    def finish(e, g):
        first = _weights(e, g)
        for it in range(2):
            _step(e, it)
        return first, _weights(e, g), _flat(e, g, r)

    e, g = _engine(hip, d, r, "GNC_TLS", **kw)
    e.set_weights(w0, fixed)
    host = finish(e, g)
    assert np.array_equal(host[0], w0) and np.any(host[1] != w0) and np.array_equal(host[1][fixed], w0[fixed])
    ft = torch.from_numpy(fixed.astype(np.uint8)).cuda()
    for offset in (0, 1):
        buf = torch.zeros(len(w0) + offset, dtype=torch.float64, device="cuda")
        buf[offset:] = torch.from_numpy(np.array(w0)).cuda()
        torch.cuda.synchronize()
        assert buf[offset:].data_ptr() == buf.data_ptr() + 8 * offset
        e, g = _engine(hip, d, r, "GNC_TLS", **kw)
        e.set_weights_dev(buf[offset:].data_ptr(), ft.data_ptr())
        dev = finish(e, g)
        for a, b in zip(host, dev):
            assert np.array_equal(a, b), offset
    # without flags
    e, g = _engine(hip, d, r, "GNC_TLS", **kw)
    e.set_weights(w0)
    host = finish(e, g)
    e, g = _engine(hip, d, r, "GNC_TLS", **kw)
    e.set_weights_dev(buf[1:].data_ptr())
    for a, b in zip(host, finish(e, g)):
        assert np.array_equal(a, b)
    assert np.any(host[1][fixed] != w0[fixed])


def test_kernel_timing_entry_leaves_the_engine_alone(hip):
    """dpgo_rbcd_bench_set_weights repeats the gather of the last host-form call: weights and evaluation stay bitwise
    what they were; once a reweighting has run (the staged values are no longer the engine's) it refuses."""
    d, r = 3, 5
    w0, fixed = WT.W(d), _fixed(d)
    e, g = _engine(hip, d, r, "GNC_TLS", **dict(INLIER_RUN, **SCHEDULE))
    with pytest.raises(hip.DPGOHipError):
        e.bench_set_weights(0)
    e.set_weights(w0, fixed)
    before = e.central_eval(weighted=True)
    for c in range(e.num_colors):
        assert e.bench_set_weights(c, 2) > 0.0
    assert np.array_equal(_weights(e, g), w0) and _same_eval(e.central_eval(weighted=True), before)
    _step(e, 0)
    w1 = _weights(e, g)
    assert np.any(w1 != w0)
    with pytest.raises(hip.DPGOHipError):
        e.bench_set_weights(0)
    assert np.array_equal(_weights(e, g), w1)


# ------------------------------------------------------------------------------------------ 7
GK, GA, GR, GD, GITERS = 6, 2, 5, 3, 6


def _grid_case(H):
    g = H.Graph.grid3d(GK, seed=5)
    aop = g.grid_partition(GA)
    owner = H.weight_owner(g, aop, GA ** 3)
    rng = np.random.default_rng(17)
    u = rng.random(g.m)
    w = np.where(u < 0.15, 0.0, np.where(u < 0.4, 1.0, rng.uniform(0.05, 1.0, g.m)))
    w[owner < 0] = rng.uniform(0.25, 1.0, int((owner < 0).sum()))
    fixed = ((owner >= 0) & (np.arange(g.m) % 3 == 0)).astype(np.uint8)
    params = H.rbcd_params(r=GR, acceleration=1, robust_cost=H.ROBUST["GNC_TLS"], robust_opt_inner_iters=2, gnc_barc=0.6,
                           gnc_init_mu=0.05, gnc_mu_step=3.0)
    return g, aop, owner, w, fixed, params


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dpgo_amd import hip as H
        g, aop, owner, w, fixed, params = _grid_case(H)
        ranks = (np.arange(GA ** 3) * world // GA ** 3).astype(np.int32)
        e = H.Rbcd(g, aop, ranks, rank, world, params)
        e.set_X(g.chain_init(GR, O.lifting_matrix(GD, GR)))
        dev = torch.device("cuda", 0)
        s = torch.cuda.Stream(dev)
        e.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            e.set_weights(w, fixed)
            send = torch.zeros(max(int(e.send_counts.sum()), 1), dtype=torch.float64, device=dev)
            recv = torch.zeros(max(int(e.recv_counts.sum()), 1), dtype=torch.float64, device=dev)
            rsplit = [int(x) for x in e.recv_counts]
            ssplit = [int(x) for x in e.send_counts]
            for it in range(GITERS):
                c = it % e.num_colors
                e.pre_exchange(c)
                e.pack(send.data_ptr())
                hs = send.cpu()
                hr = torch.empty_like(recv, device="cpu")
                dist.all_to_all_single(hr, hs, rsplit, ssplit)
                recv.copy_(hr)
                e.update(c, recv.data_ptr())
            wout = np.full(g.m, np.nan)
            e.weights_into(wout)
            X = np.full(g.n * (GD + 1) * GR, np.nan)
            e.get_X_into(X)
        q.put((rank, wout, X))
    finally:
        dist.destroy_process_group()


def test_two_ranks_bitwise_one_rank():
    """GNC_TLS with a mask, set_weights on both ranks (each the full arrays), the colour schedule over gloo: the merged
    get_weights and get_X are bitwise the one-rank engine's."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(rk, 2, port, q)) for rk in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=240) for _ in range(2)], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=60)
    from dpgo_amd import hip as H
    g, aop, owner, w, fixed, params = _grid_case(H)
    e1 = H.Rbcd(g, aop, np.zeros(GA ** 3, np.int32), 0, 1, params)
    e1.set_X(g.chain_init(GR, O.lifting_matrix(GD, GR)))
    e1.set_weights(w, fixed)
    for it in range(GITERS):
        _step(e1, it)
    w1 = np.full(g.m, np.nan)
    e1.weights_into(w1)
    X1 = np.full(g.n * (GD + 1) * GR, np.nan)
    e1.get_X_into(X1)
    for which, one in ((1, w1), (2, X1)):
        parts = [o[which] for o in outs]
        wr = [~np.isnan(x) for x in parts]
        assert np.all(wr[0].astype(int) + wr[1].astype(int) == 1) and wr[0].any() and wr[1].any()
        assert np.array_equal(np.where(wr[0], parts[0], parts[1]), one), which
    fx = fixed.astype(bool)
    assert np.array_equal(w1[fx], w[fx]) and np.array_equal(w1[owner < 0], w[owner < 0])
    free = (owner >= 0) & ~fx
    assert np.any(w1[free] != w[free])  # the reweighting ran
    p1, p2 = g.arrays()["p1"].astype(np.int64), g.arrays()["p2"].astype(np.int64)
    ranks = np.arange(GA ** 3) * 2 // GA ** 3
    assert np.any(ranks[aop[p1]] != ranks[aop[p2]])  # edges across the ranks


# ------------------------------------------------------------------------------------------ 8
def test_pcm_hand_over(hip):
    """tests/_pcm.fixture3d: PCM's mask through hip.pcm_weights under GNC_TLS.  The rejected closures stay exactly 0
    through the reweightings, the accepted ones and the private ones are reweighted, and the weighted evaluation is
    Graph.edge_errors' weighted cost."""
    fx = P.fixture3d()
    d, r, Kp = fx["d"], 5, fx["K"]
    g = P.graph_of(hip, fx)
    T, frames, _ = g.distributed_init_ex(fx["aop"], local="odometry", align="pcm", max_translation_error=fx["c_t"],
                                         gpu=True)
    ei, _ = g.pcm(fx["aop"], T, max_translation_error=fx["c_t"], gpu=True)
    assert np.array_equal(ei, fx["labels"]) and (ei == 0).sum() >= 5 and (ei == 1).sum() >= 5
    w, fixed = hip.pcm_weights(ei)
    assert np.array_equal(w, np.where(ei == 0, 0.0, 1.0)) and np.array_equal(fixed != 0, ei == 0)
    assert np.all(w[ei == 255] == 1.0) and not fixed[ei == 255].any()
    e = hip.Rbcd(g, fx["aop"], np.zeros(Kp, np.int32), 0, 1,
                 hip.rbcd_params(r=r, acceleration=0, robust_cost=hip.ROBUST["GNC_TLS"], robust_opt_inner_iters=1,
                                 **SCHEDULE))
    e.set_trajectory(T, O.lifting_matrix(d, r), frames)
    e.set_weights(w, fixed)
    assert np.array_equal(_weights(e, g), w)
    f0 = e.central_eval(weighted=True)[0]
    c0 = g.edge_errors(_flat(e, g, r), r, w=w)["cost"]
    assert abs(f0 - c0) <= VALUE_BAR * c0
    for it in range(2 * e.num_colors):  # every agent is selected twice: at least two reweightings of every closure
        _step(e, it)
    wn = _weights(e, g)
    assert np.all(wn[ei == 0] == 0.0), "a rejected closure was reweighted"
    owner = hip.weight_owner(g, fx["aop"], Kp)
    assert np.all(wn[owner < 0] == 1.0)
    accepted, private = wn[ei == 1], wn[(ei == 255) & (owner >= 0)]
    print(f"rejected {int((ei == 0).sum())} held at 0; accepted: {int((accepted != 1.0).sum())} of {len(accepted)} "
          f"moved off 1; private closures: {int((private != 1.0).sum())} of {len(private)}")
    assert np.any(accepted != 1.0), "no accepted closure was reweighted: are they free?"
    f = e.central_eval(weighted=True)[0]
    print(f"hand-over: f {f0:.12g} against edge_errors {abs(f0 - c0) / c0:.2e}; the weighted cost after the run "
          f"{f:.6g}")
    assert f < f0  # the run descended on the problem it was handed
