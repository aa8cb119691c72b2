"""GPU parity of the per-iteration RTR trace, RGD, solver statistics, the engine's PGOAgent status and
its central evaluation against the oracle (tests/ infrastructure only).

References: ROPTLIB ITERRESULT trace (src/QuadraticOptimizer.cpp:82-86),
QuadraticOptimizer::gradientDescent (src/QuadraticOptimizer.cpp:124-149), PGOAgent::iterate status
(src/PGOAgent.cpp:700-716, 1247-1289), central evaluation (examples/MultiRobotExample.cpp:229-256)."""
import math

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests._common import load_meas, random_point, rel
from tests._extended import rtr_extended as _rtr_extended

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _expected_records(trace):
    """Oracle RTR trace -> the device's record sequence (tCG step test, tCG stopping test, rho test)."""
    out = []
    for outer in trace:
        for t in outer["tcg"]:
            st = dict(op=3, j=t["j"], d_Hd=t["d_Hd"], alpha=t["alpha"], Delta=outer["Delta"])
            if "tau" in t:
                st.update(tau=t["tau"], status=t["status"])
            out.append(st)
            if "norm_r" in t:
                ck = dict(op=4, j=t["j"], norm_r=t["norm_r"])
                if "status" in t:
                    ck["status"] = t["status"]
                else:
                    ck.update(z_r=t["z_r"], beta=t["beta"])
                out.append(ck)
        out.append(dict(op=5, f1=outer["f1"], f2=outer["f2"], rho=outer["rho"], Delta=outer["Delta"],
                        accepted=float(outer["accepted"]), ngf=outer["ngf"], status=outer["status"],
                        alpha=outer["ninner"]))
    return out


def _close(a, b, tol):
    return abs(a - b) <= tol * max(abs(b), 1e-300)


@pytest.mark.parametrize("name,r,iters,tol,radius,inner", [
    ("smallGrid3D", 5, 10, 1e-1, 10.0, 50),   # localPoseGraphOptimization (src/PGOAgent.cpp:975-984)
    ("tinyGrid3D", 3, 10, 1e-1, 10.0, 50),
    ("sphere2500", 3, 10, 1e-1, 10.0, 50),
    ("smallGrid3D", 5, 1, 1e-2, 100.0, 10),   # updateX settings (:1131-1137)
])
@pytest.mark.parametrize("precon", ["bj", "bj-classic", "none", "none-classic", "exact", "bj-edges", "none-edges"])
def test_rtr_trace_matches_oracle(hip, name, r, iters, tol, radius, inner, precon):
    """Every tCG step (d_Hd, alpha, tau, status), stopping test (|r|, <z, r>, beta, status) and rho test
    (f1, f2, rho, Delta, accepted, |grad|, status, inner iterations) of the device RTR equals the
    oracle's at 1e-10 relative (rho: cancellation-aware), in the same order.  "bj": the merged tCG
    iteration (stopping test from one-step polynomials in alpha), "bj-classic": the five-launch sequence
    (tuning key TUNE_CLASSIC_TCG); the exact factor always runs the classic one.  Q is uploaded as BSR blocks,
    or ("-edges") as the measurement stream the engine uses (its SpMMs, and the merged partials' precision of
    kMergedDdSlots)."""
    hip.set_tuning(5, 1 if precon.endswith("-classic") else 0)
    try:
        _rtr_trace_case(hip, name, r, iters, tol, radius, inner, precon.split("-")[0],
                        merged=precon in ("bj", "none", "bj-edges", "none-edges"), edges=precon.endswith("-edges"))
    finally:
        hip.set_tuning(5, 0)


def _set_Q(H, meas, Q, edges):
    if edges:
        H.set_Q_edges(0, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau, meas.weight)
    else:
        H.set_Q_scipy(0, Q)


def _rtr_trace_case(hip, name, r, iters, tol, radius, inner, precon, merged, edges=False):
    rtr_tol = tol
    meas = load_meas(name)
    d, n = meas.d, meas.num_poses
    Q = O.connection_laplacian(meas, n)
    P = O.QuadraticProblem(n, d, r)
    P.set_Q(Q)
    P.precon_mode = {"bj": O.PRECON_BLOCK_JACOBI, "none": O.PRECON_NONE, "exact": O.PRECON_EXACT}[precon]
    X0 = O.lifting_matrix(d, r) @ O.chordal_initialization(d, n, meas)
    trace = []
    Xo, res = O.optimize(P, X0, O.OptParams(tr_iterations=iters, tr_tolerance=tol, tr_initial_radius=radius,
                                            tr_max_inner=inner), trace)
    H = hip.Problem(n, d, r)
    _set_Q(H, meas, Q, edges)
    H.set_trace(4096)
    p = hip.default_params(tr_iterations=iters, tr_tolerance=tol, tr_initial_radius=radius, tr_max_inner=inner,
                           precon={"bj": hip.PRECON_BLOCK_JACOBI, "none": hip.PRECON_NONE,
                                   "exact": hip.PRECON_EXACT}[precon])
    Xh, rh = H.optimize(X0, p)
    got = H.get_trace(0)
    exp = _expected_records(trace)
    assert len(exp) > 3
    assert len(got) == len(exp)
    # Tolerance: 1e-10 relative with block-Jacobi.  With the exact factor the bar is derived the same way as the
    # merged sequence's below: max(1e-10, 2 x the float64 oracle's own distance from the extended-precision Run of
    # the same settings (its exact branch: (Q + 0.1 I)^-1 by sparse LU refined in extended precision)).  That is
    # 1e-10 on smallGrid3D, ~2.5e-10 on sphere2500 and ~1.3e-7 on tinyGrid3D, whose exact-preconditioned trajectory
    # amplifies rounding ~1e5-fold from the second Run on (a 1e-16 perturbation of X0 moves the extended-precision
    # Run itself by 7e-11; every float64 implementation sits 6e-8 from it).
    # Quantities that shrink inside one tCG (d_Hd, alpha, |r|, <z, r>, beta, tau) are measured against
    # their largest magnitude in that tCG: their terms cancel, so their rounding floor is set by it.
    # rho = (f1 - f2) / model decrease: f1 - f2 loses the digits |f1| / |f1 - f2|.
    tol = 1e-10
    if precon == "exact":
        ext = _rtr_extended(Q, X0, d, rtr_tol, radius, 5.0 * radius, iters, inner, precon="exact")
        assert [e["op"] for e in ext] == [e["op"] for e in exp]
        tol = max(1e-10, 2.0 * _trace_deviation(exp, ext))
        print(f"{name} r={r} exact: oracle vs extended-precision Run {_trace_deviation(exp, ext):.2e}, "
              f"device vs extended {_trace_deviation(got, ext):.2e}, device vs oracle {_trace_deviation(got, exp):.2e}; "
              f"bar {tol:.2e}")
    if precon == "none":
        # unpreconditioned tCG: 50 inner iterations on smallGrid3D amplify the summation-order rounding
        # (the classic sequence, the oracle's own operations, differs by 1.6e-9 of |r| at iteration 8 and
        # the merged one by 8e-8 at 11): the bars of this case are 1e-6
        tol = 1e-6
    # The merged tCG iteration forms |r_{j+1}|^2 and <z_{j+1}, r_{j+1}> (hence beta) from one-step
    # polynomials in alpha over r_j and Hd_j, whose terms cancel by the factor <z_j, r_j> / <z_{j+1},
    # r_{j+1}>; the partials are double-double (exact products, compensated sums, the polynomial in
    # double-double: dpgo_device.h dd_*), so the polynomials add no rounding of their own.  What remains is
    # the trajectory's own conditioning: on tinyGrid3D the third outer iteration's tCG amplifies 1e-16
    # differences in its starting point by ~1e5, and the float64 oracle itself is 1.3e-10 from an
    # extended-precision Run there (test_rtr_trace_extended_precision).  The merged sequence, which rounds
    # r' = r + alpha Hd once (FMA) where the oracle rounds twice, is held to the classic bar or to twice the
    # oracle's own distance from the extended-precision Run, whichever is larger (computed per case, for the
    # graphs whose dense extended-precision Run is cheap).
    tcg_tol = tol
    if merged and precon == "bj" and iters > 1 and n * (d + 1) <= 2000:
        ext = _rtr_extended(Q, X0, d, rtr_tol, radius, 5.0 * radius, iters, inner)
        if [e["op"] for e in ext] == [e["op"] for e in exp]:
            tcg_tol = max(tol, 2.0 * _trace_deviation(exp, ext))
    scale, run_id = {}, None
    for g, e in zip(got, exp):
        if e["op"] == 5 or run_id != g["run"]:
            run_id = g["run"]
            scale = {}
        for k in ("d_Hd", "alpha", "norm_r", "z_r", "beta", "tau"):
            if k in e and not (k == "alpha" and e["op"] == 5):
                scale[k] = max(scale.get(k, 0.0), abs(e[k]))
        if e["op"] == 3:  # the step test also carries <z, r> and |r_0| (not compared: the oracle has them
            for k in ("z_r", "norm_r"):  # only after the update) -- they set the scale of the later ones
                scale[k] = max(scale.get(k, 0.0), abs(g[k]))
        assert int(g["op"]) == e["op"], (g, e)
        for k, v in e.items():
            if k in ("op",):
                continue
            if k in ("j", "status", "accepted"):
                assert int(g[k]) == int(v), (k, g, e)
            elif k == "rho":
                # f1 and f2 themselves agree to 1e-10 (checked above); their difference carries f's
                # rounding (a Laplacian quadratic form over absolute positions: ~1e-12 of f), amplified
                # by |f1| / |f1 - f2|
                rt = 10 * tol + 1e-11 * abs(e["f1"]) / max(abs(e["f1"] - e["f2"]), 1e-300)
                assert _close(g[k], v, rt), (k, g[k], v)
            elif k == "alpha" and e["op"] == 5:
                assert int(g[k]) == int(v)  # inner iterations of the Run
            elif k == "alpha":  # z_r / d_Hd: inherits d_Hd's bound relative to its own size
                at = tcg_tol * abs(v) * (1.0 + scale["d_Hd"] / max(abs(e["d_Hd"]), 1e-300))
                assert abs(g[k] - v) <= at, (k, g[k], v, e)
            elif k == "beta":  # <z, r>_new / <z, r>_old: both bounded relative to the largest <z, r>
                bt = tcg_tol * abs(v) * (1.0 + 2.0 * scale["z_r"] / max(abs(e["z_r"]), 1e-300))
                assert abs(g[k] - v) <= bt, (k, g[k], v, e)
            elif k in scale:
                assert abs(g[k] - v) <= tcg_tol * max(scale[k], 1e-300), (k, g[k], v, e)
            else:
                assert _close(g[k], v, tol), (k, g[k], v, e)
    st = H.stats()[0]
    runs = [t for t in trace]
    assert st["calls"] == 1 and st["runs"] == len(runs)
    assert st["tcg_iters"] == sum(t["ninner"] for t in runs)
    for s, name_ in ((O.TCG_NEGCURVTURE, "NEGCURVTURE"), (O.TCG_EXCREGION, "EXCREGION"), (O.TCG_LCON, "LCON"),
                     (O.TCG_SCON, "SCON"), (O.TCG_MAXITER, "MAXITER")):
        assert st[name_] == sum(1 for t in runs if t["status"] == s)
    assert rel(Xh, Xo) <= max(1e-8, tol)


def _trace_deviation(got, ref):
    """Largest deviation of a trace from a reference one, per tCG quantity relative to its largest magnitude
    in that tCG (the trace test's scale), and for the rho-test quantities relative to themselves."""
    worst, scale = 0.0, {}
    for g, e in zip(got, ref):
        if e["op"] == 5:
            for k in ("f1", "f2", "ngf"):
                worst = max(worst, abs(g[k] - e[k]) / max(abs(e[k]), 1e-300))
            scale = {}
            continue
        for k in ("d_Hd", "alpha", "norm_r", "z_r", "beta", "tau"):
            if k in e:
                scale[k] = max(scale.get(k, 0.0), abs(e[k]))
        for k in ("d_Hd", "norm_r", "z_r", "beta", "tau"):
            if k in e:
                worst = max(worst, abs(g[k] - e[k]) / max(scale[k], 1e-300))
    return worst


@pytest.mark.parametrize("name,r", [("tinyGrid3D", 3), ("smallGrid3D", 5)])
def test_rtr_trace_extended_precision(hip, name, r):
    """The device RTR trace (localPoseGraphOptimization settings, block-Jacobi), merged and classic tCG
    sequences, against an extended-precision (64-bit mantissa) restatement of the same Run: both within
    1e-10 of it, as the float64 oracle is.  Where a float64 trajectory is ill-conditioned (tinyGrid3D's third
    outer iteration amplifies 1e-16 differences in its starting point by ~1e5), every float64
    implementation -- oracle, classic, merged -- sits at that distance from the extended-precision Run and
    from each other; this test shows the merged sequence is no further from it than the oracle is."""
    meas = load_meas(name)
    d, n = meas.d, meas.num_poses
    Q = O.connection_laplacian(meas, n)
    P_ = O.QuadraticProblem(n, d, r)
    P_.set_Q(Q)
    P_.precon_mode = O.PRECON_BLOCK_JACOBI
    X0 = O.lifting_matrix(d, r) @ O.chordal_initialization(d, n, meas)
    trace = []
    O.optimize(P_, X0, O.OptParams(tr_iterations=10, tr_tolerance=1e-1, tr_initial_radius=10.0, tr_max_inner=50),
               trace)
    ora = _expected_records(trace)
    ext = _rtr_extended(Q, X0, d, 1e-1, 10.0, 50.0, 10, 50)
    assert [e["op"] for e in ext] == [e["op"] for e in ora]
    dev = {"oracle": _trace_deviation(ora, ext)}
    for label, classic, edges in (("classic", 1, False), ("merged", 0, False), ("merged_edges", 0, True)):
        hip.set_tuning(5, classic)
        try:
            H = hip.Problem(n, d, r)
            _set_Q(H, meas, Q, edges)
            H.set_trace(4096)
            H.optimize(X0, hip.default_params(tr_iterations=10, tr_tolerance=1e-1, tr_initial_radius=10.0,
                                              tr_max_inner=50, precon=hip.PRECON_BLOCK_JACOBI))
            got = H.get_trace(0)
        finally:
            hip.set_tuning(5, 0)
        assert [int(g["op"]) for g in got] == [e["op"] for e in ext]
        dev[label] = _trace_deviation(got, ext)
    print(f"{name}: max deviation from the extended-precision Run: " +
          ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    # the bar: within 1e-10 of the extended-precision Run, or (an ill-conditioned trajectory, where every float64
    # implementation sits at the trajectory's own amplification of rounding) within 1.5x the float64 oracle's or
    # the classic sequence's distance from it
    for m in ("merged", "merged_edges"):
        assert dev[m] <= 1e-10 or dev[m] <= 1.5 * max(dev["oracle"], dev["classic"]), dev
    assert dev["classic"] <= 1e-10 or dev["classic"] <= 1.5 * dev["oracle"], dev


@pytest.mark.parametrize("name,r", [("tinyGrid3D", 3), ("smallGrid3D", 5), ("sphere2500", 3)])
def test_rtr_trace_extended_precision_exact(hip, name, r):
    """The reference's default preconditioner (exact factor of Q + 0.1 I, the classic tCG sequence) over BSR and
    edge-stream Q, localPoseGraphOptimization settings, against the extended-precision Run with the same
    preconditioner: the device trace within 1e-10 of it or within 2x the float64 oracle's own distance from it
    (the bar test_rtr_trace_matches_oracle derives for the exact cases)."""
    meas = load_meas(name)
    d, n = meas.d, meas.num_poses
    Q = O.connection_laplacian(meas, n)
    P_ = O.QuadraticProblem(n, d, r)
    P_.set_Q(Q)
    P_.precon_mode = O.PRECON_EXACT
    X0 = O.lifting_matrix(d, r) @ O.chordal_initialization(d, n, meas)
    trace = []
    O.optimize(P_, X0, O.OptParams(tr_iterations=10, tr_tolerance=1e-1, tr_initial_radius=10.0, tr_max_inner=50),
               trace)
    ora = _expected_records(trace)
    ext = _rtr_extended(Q, X0, d, 1e-1, 10.0, 50.0, 10, 50, precon="exact")
    assert [e["op"] for e in ext] == [e["op"] for e in ora]
    dev = {"oracle": _trace_deviation(ora, ext)}
    for label, edges in (("bsr", False), ("edges", True)):
        H = hip.Problem(n, d, r)
        _set_Q(H, meas, Q, edges)
        H.set_trace(4096)
        H.optimize(X0, hip.default_params(tr_iterations=10, tr_tolerance=1e-1, tr_initial_radius=10.0,
                                          tr_max_inner=50, precon=hip.PRECON_EXACT))
        got = H.get_trace(0)
        assert [int(g["op"]) for g in got] == [e["op"] for e in ext]
        dev[label] = _trace_deviation(got, ext)
    print(f"{name} exact: max deviation from the extended-precision Run: " +
          ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for m in ("bsr", "edges"):
        assert dev[m] <= max(1e-10, 2.0 * dev["oracle"]), dev


@pytest.mark.parametrize("batched", [False, True])
def test_rgd_matches_oracle(hip, batched):
    """QuadraticOptimizer::gradientDescent (src/QuadraticOptimizer.cpp:124-149): one fixed-step (1e-3)
    Riemannian gradient step with the QF retraction; X, fOpt, gradNormOpt and relativeChange."""
    meas = load_meas("smallGrid3D")
    d, r, n = 3, 5, meas.num_poses
    Q = O.connection_laplacian(meas, n)
    P = O.QuadraticProblem(n, d, r)
    P.set_Q(Q)
    Xs = [O.lifting_matrix(d, r) @ O.chordal_initialization(d, n, meas)]
    if batched:
        Xs += [random_point(r, d, n, 41), random_point(r, d, n, 42)]
    H = hip.Problem(None, d, r, poses_per_agent=[n] * len(Xs))
    for k in range(len(Xs)):
        H.set_Q_scipy(k, Q)
    p = hip.default_params(algorithm=hip.ALG_RGD, rgd_stepsize=1e-3)
    Xh, rh = H.optimize(np.hstack(Xs), p)
    b = d + 1
    for k, X0 in enumerate(Xs):
        Xo, ro = O.optimize(P, X0, O.OptParams(algorithm="RGD", rgd_stepsize=1e-3))
        assert rel(Xh[:, k * n * b:(k + 1) * n * b], Xo) <= 1e-12
        assert _close(rh[k]["fOpt"], ro["fOpt"], 1e-12)
        assert _close(rh[k]["fInit"], ro["fInit"], 1e-12)
        assert _close(rh[k]["gradNormOpt"], ro["gradNormOpt"], 1e-10)
        assert _close(rh[k]["relativeChange"], ro["relativeChange"], 1e-10)


def _grid_meas(hip, k, seed):
    g = hip.Graph.grid3d(k, seed=seed)
    a = g.arrays()
    meas = O.Measurements(3, np.zeros(g.m, np.int64), np.zeros(g.m, np.int64), a["p1"].astype(np.int64),
                          a["p2"].astype(np.int64), a["R"], a["t"], a["kappa"], a["tau"], np.ones(g.m), g.n)
    return g, meas


def _grid_outliers(hip, k, seed, frac, rng_seed):
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


@pytest.mark.parametrize("accel,robust,alg,want", [(False, "L2", "RTR", False), (True, "L2", "RTR", False),
                                                   (True, "GNC_TLS", "RTR", False), (False, "GNC_TLS", "RTR", False),
                                                   (False, "L2", "RGD", False), (True, "L2", "RGD", False),
                                                   (False, "L2", "RGD", True), (True, "L2", "RTR", True)])
def test_engine_status_and_counters_match_oracle(hip, accel, robust, alg, want):
    """Per selected agent: PGOAgentStatus relativeChange = |X - XPrev| / sqrt(n) and readyToTerminate
    (relChangeTol 5e-3; GNC_TLS: converged loop-closure ratio >= 0.8) after every iteration, and the
    cumulative solver counters (Runs, tCG iterations and exits) over the run, against the oracle's
    PGOAgent colour schedule (RGD: src/PGOAgent.cpp:1133, QuadraticOptimizer::gradientDescent).  want: the
    updates also return per-agent ROPTResults (the in-place update's status must not be recomputed from the
    overwritten XPrev)."""
    k, A, r = 6, 2, 5
    if robust == "L2":
        g, meas = _grid_meas(hip, k, 3)
        g0 = g
    else:
        g, g0, meas = _grid_outliers(hip, k, 3, 0.1, 7)
    aop = g0.grid_partition(A)
    X0 = g0.chain_init(r, O.lifting_matrix(3, r))
    e = hip.Rbcd(g, aop, np.zeros(A ** 3, np.int32), 0, 1,
                 hip.rbcd_params(r=r, acceleration=int(accel), robust_cost=hip.ROBUST[robust], robust_opt_inner_iters=3,
                                 algorithm=hip.ALG_RTR if alg == "RTR" else hip.ALG_RGD))
    e.set_X(X0)
    iters = 7
    agents, trace = [], []
    Xo, colors = O.colour_rbcd(meas, aop, A ** 3, X0, iters, r, acceleration=accel, robust=robust,
                               robust_opt_inner_iters=3, agents_out=agents, trace=trace, algorithm=alg)
    # the oracle replays the schedule in one go; compare the final status of every agent (the status of
    # its last selected iteration) and the counters accumulated over the whole run
    for it in range(iters):
        c = it % e.num_colors
        e.pre_exchange(c)
        res = e.update(c, None, want_results=want)
        if want:
            assert len(res) == int(e.agents_per_color[c])
    out = np.zeros(X0.size)
    e.get_X_into(out)
    assert rel(hip.from_dev_layout(out, r), Xo) <= 1e-9
    rc, rd = e.status()
    for a, ag in enumerate(agents):
        assert _close(rc[a], ag.status_relative_change, 1e-8), (a, rc[a], ag.status_relative_change)
        assert bool(rd[a]) == bool(ag.ready_to_terminate), a
    st = e.stats()
    # oracle per-agent counters from its trace: RTR outer records then (it, agent, result) per update
    runs = np.zeros(A ** 3, int)
    inner = np.zeros(A ** 3, int)
    pending = []
    for t in trace:
        if isinstance(t, tuple):
            a = t[1]
            runs[a] += len(pending)
            inner[a] += sum(p["ninner"] for p in pending)
            pending = []
        else:
            pending.append(t)
    if alg == "RTR":
        assert list(st[:, 2]) == list(runs)
        assert list(st[:, 3]) == list(inner)
    assert list(st[:, 0]) == [sum(1 for t in trace if isinstance(t, tuple) and t[1] == a) for a in range(A ** 3)]
    if robust == "GNC_TLS":
        ratios = [ag.converged_loop_closure_ratio() for ag in agents]
        assert min(ratios) < 1.0  # the reweighting decided some loop closures (ratio is exercised)


def test_central_eval_matches_oracle(hip):
    """Central cost and per-agent |RieGrad|^2 of the whole graph at the engine's X
    (examples/MultiRobotExample.cpp:229-235, 243-256)."""
    k, A, r = 6, 2, 5
    g, meas = _grid_meas(hip, k, 4)
    aop = g.grid_partition(A)
    X0 = g.chain_init(r, O.lifting_matrix(3, r))
    e = hip.Rbcd(g, aop, np.zeros(A ** 3, np.int32), 0, 1, hip.rbcd_params(r=r, acceleration=1))
    e.set_X(X0)
    for it in range(3):
        e.pre_exchange(it % 2)
        e.update(it % 2, None)
    f, gn = e.central_eval()
    out = np.zeros(X0.size)
    e.get_X_into(out)
    X = hip.from_dev_layout(out, r)
    assert _close(f, O.central_cost(meas, X), 1e-11)
    Qc = O.connection_laplacian(meas, g.n)
    RG = O.tangent_project(X, np.asarray((Qc @ X.T).T), 3)
    b = 4
    for a in range(A ** 3):
        cols = np.concatenate([np.arange(p * b, (p + 1) * b) for p in np.nonzero(aop == a)[0]])
        assert _close(gn[a], float(np.sum(RG[:, cols] ** 2)), 1e-10)
    # the evaluation changes nothing: continuing gives the oracle's trajectory
    for it in range(3, 6):
        e.pre_exchange(it % 2)
        e.update(it % 2, None)
    e.get_X_into(out)
    Xo, _ = O.colour_rbcd(meas, aop, A ** 3, X0, 6, r, acceleration=True)
    assert rel(hip.from_dev_layout(out, r), Xo) <= 1e-9


def test_consumer_side_finalize_bitwise(hip):
    """The classic tCG loop with the step / stopping tests run in the consuming kernels' prologues (tuning
    key TUNE_FUSE_TCG, measured slower and off by default) gives bitwise the classic five-launch result."""
    g = hip.Graph.grid3d(12, seed=5)
    aop = g.grid_partition(2)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    out = []
    for fuse in (0, 1):
        hip.set_tuning(3, fuse)
        hip.set_tuning(5, 1 - fuse)
        try:
            e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=5, acceleration=1))
            e.set_X(X0)
            for it in range(40):
                e.pre_exchange(it % e.num_colors)
                e.update(it % e.num_colors, None)
            X = np.zeros(X0.size)
            e.get_X_into(X)
            out.append((X, e.stats().copy()))
        finally:
            hip.set_tuning(3, 0)
            hip.set_tuning(5, 0)
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])
    assert out[0][1][:, 10].sum() > 0  # CG steps were taken


def test_first_step_kind_bitwise(hip):
    """The first tCG step's d_Hd is one formula whether the batch ran the each-edge-once pass (MODE_QF)
    or the full pass that also stores Hess[delta] (MODE_HESS_QF, chosen when the previous call took CG
    steps): forcing either kind gives bitwise the same iterates, traces and counters (tuning key 4)."""
    g = hip.Graph.grid3d(12, seed=5)
    aop = g.grid_partition(2)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    out = []
    for kind in (1, 2, 0):
        hip.set_tuning(4, kind)
        try:
            e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=5, acceleration=1))
            e.set_trace(512)
            e.set_X(X0)
            for it in range(40):
                e.pre_exchange(it % e.num_colors)
                e.update(it % e.num_colors, None)
            X = np.zeros(X0.size)
            e.get_X_into(X)
            tr = np.array([[rec[k] for k in hip.TRACE_FIELDS] for rec in e.get_trace(3)])
            out.append((X, e.stats().copy(), tr))
        finally:
            hip.set_tuning(4, 0)
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0])
        assert np.array_equal(out[0][1][:, :12], other[1][:, :12])
        assert np.array_equal(out[0][2], other[2], equal_nan=True)
    assert out[1][1][:, 12].sum() > 0 and out[0][1][:, 12].sum() == 0
    assert out[0][1][:, 10].sum() > 0  # CG steps were taken


def test_merged_tcg_matches_classic(hip):
    """The merged tCG iteration (HESS_M + one finalize + k_tcg_updir, the default) against the classic
    five-launch sequence over 40 engine iterations in the CG regime: the same solver decisions (every
    counter equal) and iterates equal to rounding (beta and |r| from one-step polynomials in alpha)."""
    g = hip.Graph.grid3d(12, seed=5)
    aop = g.grid_partition(2)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    out = []
    for classic in (1, 0):
        hip.set_tuning(5, classic)
        try:
            e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=5, acceleration=1))
            e.set_X(X0)
            for it in range(40):
                e.pre_exchange(it % e.num_colors)
                e.update(it % e.num_colors, None)
            X = np.zeros(X0.size)
            e.get_X_into(X)
            out.append((X, e.stats().copy()))
        finally:
            hip.set_tuning(5, 0)
    assert np.linalg.norm(out[0][0] - out[1][0]) <= 1e-10 * np.linalg.norm(out[0][0])
    assert np.array_equal(out[0][1][:, :12], out[1][1][:, :12])
    assert out[0][1][:, 10].sum() > 0  # CG steps were taken


def test_tcg_lookahead_bitwise(hip):
    """How the host queues the merged tCG (tuning key TUNE_TCG_LOOKAHEAD: 1 = one iteration ahead of a
    status published by every finalize, 2 = every iteration queued at once with no status inside tCG, 0
    = adaptive) changes no arithmetic: bitwise the same iterates and counters over 40 engine iterations
    that mix first-step boundary exits and CG steps."""
    g = hip.Graph.grid3d(12, seed=5)
    aop = g.grid_partition(2)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    out = []
    for la in (1, 2, 0):
        hip.set_tuning(7, la)
        try:
            e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=5, acceleration=1))
            e.set_X(X0)
            for it in range(40):
                e.pre_exchange(it % e.num_colors)
                e.update(it % e.num_colors, None)
            X = np.zeros(X0.size)
            e.get_X_into(X)
            out.append((X, e.stats().copy()))
        finally:
            hip.set_tuning(7, 0)
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0])
        assert np.array_equal(out[0][1][:, :12], other[1][:, :12])
    assert out[0][1][:, 10].sum() > 0  # CG steps were taken


@pytest.mark.parametrize("accel", [False, True])
def test_status_fold_bitwise(hip, accel):
    """The PGOAgent status folded into the retraction and the rho test (the default) against its own
    k_sqdiff + OP_STATUS pass (tuning key TUNE_STATUS_PASS): bitwise the same relativeChange, the same
    readyToTerminate, the same iterates, in the boundary regime and the CG regime."""
    g = hip.Graph.grid3d(12, seed=5)
    aop = g.grid_partition(2)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    Xc = g.chain_init_dev_layout(5, hip.lifting_matrix(3, 5))
    out = []
    for sep in (1, 0):
        hip.set_tuning(9, sep)
        try:
            e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=5, acceleration=int(accel)))
            res = []
            for start in (Xc, X0):
                e.set_X(start)
                for it in range(12):
                    e.pre_exchange(it % e.num_colors)
                    e.update(it % e.num_colors, None)
                    rc, rd = e.status()
                    res.append((rc.copy(), rd.copy()))
            X = np.zeros(X0.size)
            e.get_X_into(X)
            out.append((X, res))
        finally:
            hip.set_tuning(9, 0)
    assert np.array_equal(out[0][0], out[1][0])
    for (rc0, rd0), (rc1, rd1) in zip(out[0][1], out[1][1]):
        assert np.array_equal(rc0, rc1)
        assert np.array_equal(rd0, rd1)


def test_split_streams_bitwise(hip):
    """The merged tCG iterations queued at once with the batch's agents in two halves on two streams (tuning
    key TUNE_SPLIT_STREAMS; also four groups and one group per agent) give bitwise the one-stream iterates, traces and counters: the halves touch
    disjoint agents' poses, tiles, partial slots and finalize rows."""
    g = hip.Graph.grid3d(12, seed=5)
    aop = g.grid_partition(2)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    out = []
    for split in (0, 1, 2, 3, 4):
        hip.set_tuning(10, split)
        hip.set_tuning(7, 2)  # every tCG iteration queued at once (the path the split applies to)
        try:
            e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=5, acceleration=1))
            e.set_trace(512)
            e.set_X(X0)
            for it in range(40):
                e.pre_exchange(it % e.num_colors)
                e.update(it % e.num_colors, None)
            X = np.zeros(X0.size)
            e.get_X_into(X)
            tr = [e.get_trace(a) for a in range(8)]
            out.append((X, e.stats().copy(), tr))
        finally:
            hip.set_tuning(10, 1)
            hip.set_tuning(7, 0)
    for o in out[1:]:
        assert np.array_equal(out[0][0], o[0])
        assert np.array_equal(out[0][1], o[1])
        for a in range(8):
            assert len(out[0][2][a]) == len(o[2][a])
            for x, y in zip(out[0][2][a], o[2][a]):
                assert x == y
    assert out[0][1][:, 10].sum() > 0  # CG steps were taken


def test_round4_kernel_variants_bitwise(hip):
    """The round-4 SpMM kernels (tuning key TUNE_SPMM_V2): the XOR-rotated accumulator and the single edge-loop
    pipeline only reorder registers and loads, so with the same merged partials (v2 = 2: neither, 3: rotated in the
    merged modes, 4: rotated + one pipeline there, 1 / 5: rotated / + one pipeline in every mode, 6: 5 but the half
    passes plain -- the default since round 5) the iterates,
    traces and counters are bitwise equal over 40 engine iterations in the CG regime; the round-3 kernels (v2 = 0,
    every merged partial double-double) agree to rounding with the same solver decisions."""
    g = hip.Graph.grid3d(12, seed=5)
    aop = g.grid_partition(2)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    out = {}
    default = hip.get_tuning(11)
    for v2 in (2, 3, 4, 1, 5, 6, 0):
        hip.set_tuning(11, v2)
        try:
            e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=5, acceleration=1))
            e.set_trace(512)
            e.set_X(X0)
            for it in range(40):
                e.pre_exchange(it % e.num_colors)
                e.update(it % e.num_colors, None)
            X = np.zeros(X0.size)
            e.get_X_into(X)
            tr = np.array([[rec[k] for k in hip.TRACE_FIELDS] for rec in e.get_trace(3)])
            out[v2] = (X, e.stats().copy(), tr)
        finally:
            hip.set_tuning(11, default)
    for v2 in (3, 4, 1, 5, 6):
        assert np.array_equal(out[2][0], out[v2][0]), v2
        assert np.array_equal(out[2][1], out[v2][1]), v2
        assert np.array_equal(out[2][2], out[v2][2], equal_nan=True), v2
    assert np.linalg.norm(out[0][0] - out[2][0]) <= 1e-10 * np.linalg.norm(out[2][0])
    assert np.array_equal(out[0][1][:, :12], out[2][1][:, :12])
    assert out[2][1][:, 10].sum() > 0  # CG steps were taken
