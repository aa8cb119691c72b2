"""The on-device robust reweighting (k_gnc_weights, k_gnc_snapshot, k_conv_ratio, the mu update and the ready fold)
against the np.longdouble host model of tests/_robust.py and the oracle, on the 650-pose ragged case with eight unequal
agents (tests/_robust.robust_case; tests/test_robust_reference.py checks the model against the oracle's Agents and
asserts every property of the case that the tests below rely on).  One rank, block-Jacobi.

(a)  the first reweighting at the lifted ground truth, every cost, GNC_TLS at all 13 compiled (d, r);
(a') crafted loop closures whose r^2 sits exactly on a branch bound, and on the doubles next to it;
(b)  GNC_TLS with mu 0.05 x 3 capped after 3 updates over 2 C + 1 = 11 iterations, the model fed with the engine's own X
     history: mu, the cap, the neighbour poses held since the owner's last selection, dict_ok;
(c)  the converged ratio through status()'s ready, one engine per threshold taken from the model's ratios, and before
     the first reweighting;
(d)  oracle parity (X, weights, colours, counters) for GM, L1, Huber, TLS and a capped GNC_TLS.

Bars: exact 0 / 1 decisions identical; elsewhere |w - w_ref| <= max(1e-12, 2 x the float64 numpy evaluation's own
distance from the np.longdouble one) (L1 relative to w_ref); (a') bitwise the float64 RobustCost; (d) 1e-9
once the oracle stays within 5e-10 of its twin started 1e-16 away.

Measured on an MI355X (device against np.longdouble | float64 numpy against np.longdouble, largest over the cases):
(a) GNC_TLS over the 13 shapes 3.4e-14 | 3.4e-14, L1 (relative) 4.6e-14 | 4.6e-14, Huber 7.1e-15 | 5.7e-15, GM 6.5e-15 |
6.5e-15, TLS identical; 416 loop closures reweighted, 528 held at 1, none within 1e-9 of a threshold.  (b) per iteration
7.1e-15 .. 2.2e-14 | 4.3e-15 .. 2.4e-14 at (3, 5), 1.2e-14 .. 2.0e-14 | 1.4e-14 .. 2.5e-14 at (2, 3); 528, 172, 51, then no
loop closures waiting for their owner's first selection.  (c) ratios 1, 0.6692, 0.9780, 0.8462, 0.9462, 0.9306, 1, NaN at
d = 3 (13 thresholds); accelerated schedule X 3.7e-13 and weights 1.6e-11 from the oracle.  (d) X 3.6e-14 .. 2.1e-12 at
(3, 4), <= 7.8e-16 at (2, 4); weights <= 3.4e-13 (L1, weights up to 66: 4.7e-12 / 4.0e-11; TLS identical); the oracle is
<= 1.4e-13 from its twin.
"""
import math

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _robust as RB
from tests._common import rel

pytestmark = pytest.mark.gpu

SHAPES = [(2, r) for r in range(2, 9)] + [(3, r) for r in range(3, 9)]  # DPGO_DISPATCH: every compiled (d, r)
K = len(RB.AGENTS)
NEAR = 1e-9        # residuals this close (relative) to a branch threshold are not held to the exact decision
VALUE_BAR = 1e-12  # the project's bar for evaluations

# engine parameter -> model / oracle parameter
_PARAM = dict(gnc_barc="gnc_barc", gnc_init_mu="gnc_init_mu", gnc_mu_step="gnc_mu_step", gnc_max_iters="gnc_max_iters",
              huber_threshold="huber", tls_threshold="tls")
FIRST = {"GNC_TLS": dict(gnc_barc=0.6, gnc_init_mu=1.0), "L1": {}, "TLS": dict(tls_threshold=0.8),
         "Huber": dict(huber_threshold=0.6), "GM": {}}
SCHEDULE = dict(gnc_barc=0.6, gnc_init_mu=0.05, gnc_mu_step=3.0, gnc_max_iters=3)
PARITY = {"GM": {}, "L1": {}, "Huber": dict(huber_threshold=0.6), "TLS": dict(tls_threshold=0.8),
          "GNC_TLS": dict(gnc_barc=0.6, gnc_init_mu=0.45, gnc_mu_step=3.0, gnc_max_iters=1)}


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1, "no gfx950 device"
    return H


def _model_params(kw):
    return dict(RB.DEFAULTS, **{_PARAM[k]: v for k, v in kw.items()})


def _oracle_params(kw):
    return {_PARAM[k]: v for k, v in kw.items()}


_cache = {}


def _structure(d):
    if ("st", d) not in _cache:
        meas, aop, _ = RB.robust_case(d)
        _cache[("st", d)] = (RB.Structure(meas, aop, K), O.greedy_colors(meas, aop, K))
    return _cache[("st", d)]


def _engine(hip, d, r, kind, **kw):
    """(engine, graph) on the robust case from the lifted ground truth."""
    meas, aop, T = RB.robust_case(d)
    g = hip.Graph.from_arrays(d, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    a = g.arrays()
    assert g.m == meas.m and np.array_equal(a["p1"], meas.p1) and np.array_equal(a["p2"], meas.p2)  # edge order kept
    e = hip.Rbcd(g, aop, np.zeros(K, np.int32), 0, 1, hip.rbcd_params(r=r, robust_cost=hip.ROBUST[kind], **kw))
    st, colors = _structure(d)
    assert list(e.color_of_agent) == colors
    assert np.array_equal(hip.weight_owner(g, aop, K), st.owner)
    e.set_X(O.lifting_matrix(d, r) @ T)
    return e, g


def _step(e, it):
    c = it % e.num_colors
    e.pre_exchange(c)
    e.update(c, None)


def _weights(e, g):
    w = np.full(g.m, np.nan)
    e.weights_into(w)
    assert not np.isnan(w).any()
    return w


def _X(hip, e, g, r):
    out = np.zeros(g.n * (g.d + 1) * r)
    e.get_X_into(out)
    return hip.from_dev_layout(out, r)


def check_weights(kind, w, ref, twin, st, p, label):
    """The engine's weights of one iteration against the model's record ref (np.longdouble) with the bar set by twin
    (the same model in float64).  Returns (largest distance, the twin's distance, edges left out of the exact check)."""
    lc = st.lc
    assert np.all(w[st.owner < 0] == 1.0), f"{label}: odometry reweighted"
    wl, w64 = ref["w"][lc], twin["w"][lc].astype(np.longdouble)
    gap = RB.branch_gap(kind, ref["res"], ref["mu"], p)  # NaN where this iteration left the weight alone
    near = gap < NEAR
    assert near.sum() <= 0.01 * len(lc), f"{label}: {int(near.sum())} residuals on a threshold"
    ok = ~near
    wd = w[lc]
    if kind in ("GNC_TLS", "TLS", "Huber"):
        for v in (0.0, 1.0):
            bad = np.nonzero(ok & ((wd == v) != (wl == v)))[0]
            assert len(bad) == 0, (f"{label}: {len(bad)} decisions w == {v} differ, first edge {lc[bad[0]]}: "
                                   f"device {wd[bad[0]]!r}, reference {float(wl[bad[0]])!r}, gap {gap[bad[0]]:.2e}")
    if kind == "TLS":
        assert np.all((wd == 0.0) | (wd == 1.0))
    scale = np.abs(wl) if kind == "L1" else np.ones(len(lc), np.longdouble)
    err = (np.abs(wd.astype(np.longdouble) - wl) / scale).astype(float)
    own = (np.abs(w64 - wl) / scale).astype(float)
    worst, dist = float(err[ok].max()), float(own[ok].max())
    bar = max(VALUE_BAR, 2 * dist)
    k = int(np.argmax(np.where(ok, err, -1)))
    assert worst <= bar, (f"{label}: edge {lc[k]} off by {worst:.3e} (bar {bar:.3e}): device {wd[k]!r}, reference "
                          f"{float(wl[k])!r}, residual {float(ref['res'][k])!r}, mu {ref['mu']}")
    return worst, dist, int(near.sum())


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("kind,d,r", [("GNC_TLS", d, r) for d, r in SHAPES] +
                         [(k, d, r) for k in ("L1", "TLS", "Huber", "GM") for d, r in ((3, 5), (2, 3))])
def test_first_reweighting_matches_longdouble(hip, kind, d, r):
    """robust_opt_inner_iters = 2: iteration 1 reweights at X0, before any optimisation.  Private loop closures and the
    shared ones whose owner has colour 0 sit at w(r(X0)); shared ones of the other colours are exactly 1 (their owner
    has received no pose yet: dict_ok == 0); odometry is exactly 1."""
    meas, aop, T = RB.robust_case(d)
    st, colors = _structure(d)
    kw = FIRST[kind]
    p = _model_params(kw)
    e, g = _engine(hip, d, r, kind, acceleration=0, robust_opt_inner_iters=2, **kw)
    assert np.all(_weights(e, g) == 1.0)
    _step(e, 0)
    w = _weights(e, g)
    X0 = O.lifting_matrix(d, r) @ T
    ref = RB.run_model(meas, aop, colors, kind, [X0, X0], 2, p)[0]
    twin = RB.run_model(meas, aop, colors, kind, [X0, X0], 2, p, np.float64)[0]
    late = st.shared & (np.asarray(colors)[np.maximum(st.owner, 0)] != 0)
    assert late.sum() >= 10 and np.all(ref["w"][late] == 1.0)
    assert np.all(w[late] == 1.0), "a shared loop closure was reweighted before its owner received a pose"
    moved = st.lc[~late[st.lc]]
    if kind == "GNC_TLS":  # all three branches among the reweighted ones (>= 10 % each, asserted on the CPU)
        br = RB.gnc_branch(ref["res"][~np.isnan(ref["res"])], ref["mu"], p)
        assert all((br == k).any() for k in range(3))
        assert (w[moved] == 0.0).any() and (w[moved] == 1.0).any() and ((w[moved] > 0.0) & (w[moved] < 1.0)).any()
    worst, dist, near = check_weights(kind, w, ref, twin, st, p, f"{kind} d={d} r={r}")
    print(f"{kind} d={d} r={r}: max |w - w_longdouble| = {worst:.2e}, float64 numpy's own {dist:.2e}, {near} on a "
          f"threshold, {len(moved)} reweighted / {int(late.sum())} held back")


# ------------------------------------------------------------------------------------------ (a'), at equality
def _crafted(hip, kind, errs, **kw):
    """One agent, identity rotations, pose j at (j, 0, 0), r = d = 3: odometry without residual and loop closures
    0 -> 2 + k whose translation is off by exactly (1, 0, 0) with tau = errs[k], so computeMeasurementError is errs[k]
    without any rounding.  Returns the engine's weights of the loop closures after the first reweighting."""
    n = len(errs) + 2
    p1 = list(range(n - 1)) + [0] * len(errs)
    p2 = list(range(1, n)) + [2 + k for k in range(len(errs))]
    m = len(p1)
    R = np.tile(np.eye(3), (m, 1, 1))
    t = np.zeros((m, 3))
    t[:n - 1, 0] = 1.0
    t[n - 1:, 0] = [1.0 + k for k in range(len(errs))]  # p2 - p1 - t = (2 + k) - (1 + k) = 1
    tau = np.concatenate([np.ones(n - 1), errs])
    g = hip.Graph.from_arrays(3, n, p1, p2, R, t, np.ones(m), tau)
    e = hip.Rbcd(g, np.zeros(n, np.int32), np.zeros(1, np.int32), 0, 1,
                 hip.rbcd_params(r=3, robust_cost=hip.ROBUST[kind], robust_opt_inner_iters=2, **kw))
    X0 = np.zeros((3, 4 * n))
    for j in range(n):
        X0[:, 4 * j:4 * j + 3] = np.eye(3)
        X0[0, 4 * j + 3] = float(j)
    e.set_X(X0)
    _step(e, 0)
    w = _weights(e, g)
    assert np.all(w[:n - 1] == 1.0)
    return w[n - 1:]


@pytest.mark.parametrize("mu,barc", [(0.45, 2.1), (0.15, 0.6), (0.5, 0.6), (2.5, 0.9)])
def test_gnc_branches_at_equality(hip, mu, barc):
    """r^2 exactly on a GNC bound: w is exactly 0 from the upper bound (>=) and exactly 1 up to the lower one (<=).  At
    these parameters float64 evaluates the middle formula to 5.6e-17 / 1 -+ 2e-16 there, so a comparison turned
    strict shows; the neighbouring doubles on either side take the branches of the float64 RobustCost too.  Every
    operation from the poses to the weight is exact or a single correctly rounded one, so the weights are bitwise the
    oracle's."""
    c = O.RobustCost("GNC_TLS", gnc_barc=barc, gnc_init_mu=mu)
    bc = barc * barc
    lower, upper = mu / (mu + 1) * bc, (mu + 1) / mu * bc
    errs, seen = [], 0
    for thr, exact in ((upper, 0.0), (lower, 1.0)):
        root = math.sqrt(thr)
        if root * root == thr:  # the kernel compares r * r, r = sqrt(err)
            middle = math.sqrt(bc * mu * (mu + 1) / thr) - mu
            seen += middle != exact
            assert c.weight(root) == exact
        errs += [np.nextafter(thr, 0.0), thr, np.nextafter(thr, np.inf), thr * 0.99, thr * 1.01]
    assert seen >= 1, "no bound of these parameters separates the branch from the middle formula"
    errs = np.array(errs + [0.5 * (lower + upper)])
    w = _crafted(hip, "GNC_TLS", errs, gnc_barc=barc, gnc_init_mu=mu)
    want = np.array([c.weight(math.sqrt(x)) for x in errs])
    assert (want == 0.0).any() and (want == 1.0).any() and ((want > 0.0) & (want < 1.0)).any()
    assert np.array_equal(w, want), (w.tolist(), want.tolist())


def test_tls_and_huber_at_equality(hip):
    """r == threshold: TLS rejects (r < threshold is strict), Huber gives threshold / r = 1."""
    errs = np.array([np.nextafter(0.25, 0.0), 0.25, np.nextafter(0.25, 1.0), 0.0625, 4.0])
    tls, hub = O.RobustCost("TLS", tls=0.5), O.RobustCost("Huber", huber=0.5)
    w = _crafted(hip, "TLS", errs, tls_threshold=0.5)
    assert w.tolist() == [tls.weight(math.sqrt(x)) for x in errs] == [1.0, 0.0, 0.0, 1.0, 0.0]
    w = _crafted(hip, "Huber", errs, huber_threshold=0.5)
    assert w.tolist() == [hub.weight(math.sqrt(x)) for x in errs]
    assert w[1] == 1.0 and w[3] == 1.0 and w[4] == 0.25


# ------------------------------------------------------------------------------------------ (b)
def _schedule(hip, d, r):
    """The engine's run of (b), once per shape: X and the weights after every iteration, the model and its float64
    twin on that X history."""
    if ("sch", d, r) in _cache:
        return _cache[("sch", d, r)]
    meas, aop, T = RB.robust_case(d)
    st, colors = _structure(d)
    e, g = _engine(hip, d, r, "GNC_TLS", acceleration=0, robust_opt_inner_iters=1, **SCHEDULE)
    iters = 2 * e.num_colors + 1
    hist, ws = [_X(hip, e, g, r)], []
    assert np.array_equal(hist[0], O.lifting_matrix(d, r) @ T)
    for it in range(iters):
        _step(e, it)
        hist.append(_X(hip, e, g, r))
        ws.append(_weights(e, g))
    p = _model_params(SCHEDULE)
    model = RB.run_model(meas, aop, colors, "GNC_TLS", hist, 1, p)
    twin = RB.run_model(meas, aop, colors, "GNC_TLS", hist, 1, p, np.float64)
    _cache[("sch", d, r)] = (hist, ws, model, twin, p)
    return _cache[("sch", d, r)]


@pytest.mark.parametrize("d,r", [(3, 5), (2, 3)])
def test_mu_schedule_cap_and_dictionaries(hip, d, r):
    """Every iteration's weights against the model: mu is 0.05, 0.15, 0.45, 1.35 and stays there (gnc_max_iters 3), a
    non-selected owner reweights a shared loop closure from the neighbour pose it received at its last selection, and
    not at all before its first."""
    st, colors = _structure(d)
    hist, ws, model, twin, p = _schedule(hip, d, r)
    C = max(colors) + 1
    assert len(ws) == 2 * C + 1
    mus = [rec["mu"] for rec in model]
    assert mus[:4] == [0.05, 0.05 * 3.0, 0.05 * 3.0 * 3.0, 0.05 * 3.0 * 3.0 * 3.0] and set(mus[3:]) == {mus[3]}
    for t, w in enumerate(ws):
        worst, dist, near = check_weights("GNC_TLS", w, model[t], twin[t], st, p, f"d={d} r={r} iteration {t + 1}")
        held_back = int(np.isnan(model[t]["res"]).sum())
        print(f"d={d} r={r} iteration {t + 1} (mu {mus[t]:.4g}): max |w - w_longdouble| = {worst:.2e}, float64 numpy's "
              f"own {dist:.2e}, {near} on a threshold, {held_back} held back")
    last = model[-1]
    br = RB.gnc_branch(last["res"], last["mu"], p)
    wd = ws[-1][st.lc]
    assert not np.isnan(last["res"]).any()
    for k, took in enumerate((wd == 1.0, (wd > 0.0) & (wd < 1.0), wd == 0.0)):
        assert (br == k).any() and took.any(), f"branch {k} does not occur in the final iteration"
    # the held poses matter in this run: with the newest neighbour poses instead the weights would differ visibly
    meas, _, _ = RB.robust_case(d)
    newest = RB.weight("GNC_TLS", RB.residuals_at(meas, st, hist[-2]), last["mu"], p)
    assert float(np.max(np.abs(newest - last["w"][st.lc]))) > 1e-6


# ------------------------------------------------------------------------------------------ (c)
def _ready_run(hip, d, r, threshold, accel, iters):
    e, g = _engine(hip, d, r, "GNC_TLS", acceleration=accel, robust_opt_inner_iters=1, rel_change_tol=1e300,
                   min_convergence_ratio=threshold, **SCHEDULE)
    out = []
    for it in range(iters):
        _step(e, it)
        out.append(e.status()[1].copy())
    return e, g, out


@pytest.mark.parametrize("d,r", [(3, 5), (2, 3)])
def test_ready_follows_the_converged_ratio(hip, d, r):
    """rel_change_tol = 1e300: ready[a] == not (ratio_a < min_convergence_ratio) after every iteration, for every agent
    selected so far; thresholds below all ratios, between every two distinct ones, equal to each (count / total in
    double on both sides: the agent is ready) and above 1 (only the agent without loop closures, 0/0 = NaN, is ready)."""
    st, colors = _structure(d)
    _, _, model, _, _ = _schedule(hip, d, r)
    final = model[-1]["ratio"]
    assert math.isnan(final[RB.EXTRA_AGENT]) and len({x for x in final if not math.isnan(x)}) >= 3
    thresholds = RB.thresholds_from(final)
    print(f"d={d} r={r}: ratios {['%.4f' % x for x in final]}, {len(thresholds)} thresholds")
    for thr in thresholds:
        _, _, ready = _ready_run(hip, d, r, thr, 0, len(model))
        for t, rd in enumerate(ready):
            for a in range(K):
                if model[t]["selected"][a]:
                    want = RB.ready_from_ratio(model[t]["ratio"][a], thr)
                    assert bool(rd[a]) == want, (f"threshold {thr!r}, iteration {t + 1}, agent {a}: ready {rd[a]}, "
                                                 f"model ratio {model[t]['ratio'][a]!r}")
        got = [bool(x) for x in ready[-1]]
        assert got[RB.EXTRA_AGENT]  # NaN < threshold is false
        if thr > 1.0:
            assert sum(got) == 1
        if thr < min(x for x in final if not math.isnan(x)):
            assert all(got)


def test_ready_with_acceleration_matches_oracle(hip):
    """The same schedule with Nesterov acceleration at (3, 5) against the oracle's Agents: ready_to_terminate of every
    agent after the run, one engine per threshold from the oracle's converged_loop_closure_ratio() values; the oracle
    itself runs with 0.9, where its ready flags follow its ratios by the same rule."""
    d, r = 3, 5
    meas, aop, T = RB.robust_case(d)
    st, colors = _structure(d)
    iters = 2 * (max(colors) + 1) + 1
    X0 = O.lifting_matrix(d, r) @ T
    okw = _oracle_params(SCHEDULE)

    # ratios as of each agent's last selection: the flags are set there, and the weights of a non-selected agent move on
    seen, ags = {}, []

    def grab(it, agents):
        for ag in agents:
            if colors[ag.id] == it % (max(colors) + 1):
                seen[ag.id] = ag.converged_loop_closure_ratio()

    fixed = 0.9  # the oracle's own threshold: its flags follow its ratios by the rule the engine is held to
    Xo, _ = O.colour_rbcd(RB.fresh(meas), aop, K, X0, iters, r, acceleration=True, robust="GNC_TLS",
                          robust_opt_inner_iters=1, agents_out=ags, on_iteration=grab, rel_change_tol=1e300,
                          robust_opt_min_convergence_ratio=fixed, **okw)
    ratios = [seen[a] for a in range(K)]
    flags = [ag.ready_to_terminate for ag in ags]
    assert flags == [RB.ready_from_ratio(x, fixed) for x in ratios] and len(set(flags)) == 2
    thresholds = RB.thresholds_from(ratios) + [fixed]
    wo = RB.oracle_weights(ags, meas, aop)
    print(f"oracle ratios {['%.4f' % x for x in ratios]}")
    for thr in thresholds:
        e, g, ready = _ready_run(hip, d, r, thr, 1, iters)
        if thr == thresholds[0]:
            w = _weights(e, g)
            err = rel(_X(hip, e, g, r), Xo)
            print(f"accelerated schedule: X {err:.2e}, max |w - w_oracle| {np.max(np.abs(w - wo)):.2e}")
            assert err <= 1e-9 and np.max(np.abs(w - wo)) <= 1e-9
            assert np.array_equal(w == 0.0, wo == 0.0) and np.array_equal(w == 1.0, wo == 1.0)
        for a in range(K):
            assert bool(ready[-1][a]) == RB.ready_from_ratio(ratios[a], thr), (thr, a, ratios[a])


def test_ready_before_the_first_reweighting(hip):
    """robust_opt_inner_iters = 3, one iteration: nothing has been reweighted, every weight is 1, so the ratio is 1
    for an agent with loop closures and 0/0 = NaN for the one without (computeConvergedLoopClosureRatio runs in every
    iterate, src/PGOAgent.cpp:706-712).  With min_convergence_ratio = 1.5 only that agent is ready."""
    d, r = 3, 5
    meas, aop, T = RB.robust_case(d)
    st, colors = _structure(d)
    ags = []
    O.colour_rbcd(RB.fresh(meas), aop, K, O.lifting_matrix(d, r) @ T, 1, r, robust="GNC_TLS",
                  robust_opt_inner_iters=3, agents_out=ags, rel_change_tol=1e300, robust_opt_min_convergence_ratio=1.5)
    e, g = _engine(hip, d, r, "GNC_TLS", acceleration=0, robust_opt_inner_iters=3, rel_change_tol=1e300,
                   min_convergence_ratio=1.5)
    _step(e, 0)
    rd = e.status()[1]
    picked = [a for a in range(K) if colors[a] == 0]
    assert RB.EXTRA_AGENT in picked and len(picked) >= 2
    for a in picked:
        assert ags[a].ready_to_terminate == (a == RB.EXTRA_AGENT)
        assert bool(rd[a]) == ags[a].ready_to_terminate, (a, rd[a])


# ------------------------------------------------------------------------------------------ (d)
# d = 3: six iterations.  d = 2: five (every colour once; both reweightings, at iterations 2 and 5, still happen): the
# sixth iteration -- colour 0's second update -- takes the float64 oracle 1.4e-8 .. 3e-8 away from its own twin for TLS
# and GNC_TLS and up to 1e-10 for Huber (measured on the CPU, two noise seeds), while after five it is within 6e-16.
PARITY_ITERS = {3: 6, 2: 5}


def _oracle_counters(trace, num_agents):
    """(optimize calls, Runs, tCG iterations) per agent from colour_rbcd's trace (RTR outer records, then
    (iteration, agent, result) per update)."""
    calls, runs, inner = (np.zeros(num_agents, int) for _ in range(3))
    pending = []
    for t in trace:
        if isinstance(t, tuple):
            calls[t[1]] += 1
            runs[t[1]] += len(pending)
            inner[t[1]] += sum(q["ninner"] for q in pending)
            pending = []
        else:
            pending.append(t)
    return calls, runs, inner


@pytest.mark.parametrize("accel", [False, True])
@pytest.mark.parametrize("kind", ["GM", "L1", "Huber", "TLS", "GNC_TLS"])
@pytest.mark.parametrize("d,r", [(3, 4), (2, 4)])
def test_engine_matches_oracle_every_cost(hip, d, r, kind, accel):
    """PARITY_ITERS iterations with robust_opt_inner_iters = 3 (reweighting at iterations 2 and 5; GNC_TLS: mu 0.45,
    then 1.35 and capped) against the oracle's colour schedule: X and every reported weight at 1e-9, TLS decisions identical,
    colours and solver counters equal.  The bar is trusted once the oracle stays within 5e-10 of its own twin started
    1e-16 (relative) away."""
    meas, aop, T = RB.robust_case(d)
    X0 = O.lifting_matrix(d, r) @ T
    kw = PARITY[kind]

    def oracle(X, ags=None, trace=None):
        return O.colour_rbcd(RB.fresh(meas), aop, K, X, PARITY_ITERS[d], r, acceleration=accel, robust=kind,
                             robust_opt_inner_iters=3, agents_out=ags, trace=trace, **_oracle_params(kw))

    ags, trace = [], []
    Xo, colors = oracle(X0, ags, trace)
    noise = np.random.default_rng(3).standard_normal(X0.shape)
    twin = rel(oracle(X0 * (1.0 + 1e-16 * noise))[0], Xo)
    print(f"{kind} d={d} r={r} accel={accel}: oracle vs its perturbed twin {twin:.2e}")
    assert twin <= 5e-10
    e, g = _engine(hip, d, r, kind, acceleration=int(accel), robust_opt_inner_iters=3, **kw)
    for it in range(PARITY_ITERS[d]):
        _step(e, it)
    assert list(e.color_of_agent) == colors
    err = rel(_X(hip, e, g, r), Xo)
    w, wo = _weights(e, g), RB.oracle_weights(ags, meas, aop)
    st, _ = _structure(d)
    werr = float(np.max(np.abs(w - wo)))
    print(f"    engine vs oracle: X {err:.2e}, weights {werr:.2e} (largest weight {wo.max():.3g})")
    assert err <= 1e-9
    assert werr <= 1e-9
    assert np.all(w[st.owner < 0] == 1.0) and np.any(wo[st.lc] != 1.0)
    if kind == "TLS":
        assert np.array_equal(w, wo) and set(np.unique(w)) == {0.0, 1.0}
    calls, runs, inner = _oracle_counters(trace, K)
    stats = e.stats()
    assert list(stats[:, 0]) == list(calls)
    assert list(stats[:, 2]) == list(runs)
    assert list(stats[:, 3]) == list(inner)
