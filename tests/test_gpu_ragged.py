"""GPU parity on the ragged graph (tests/_ragged.py): the SpMM's unstaged tiles, the two-stage loop of edge_loop_uni,
poses and agents without incidences, parallel measurements, ragged agent sizes and every compiled (d, r).

The committed datasets and grid3d never leave the staged, straight-line SpMM paths and use 5 of the 13 compiled
(r, b) instantiations; this file runs the evaluations, the per-pose kernels and one RTR Run at all 13, on a graph whose
tiles are unstaged by their incidences alone, by their first-visit records alone and by both, whose hub poses have 8..11
incidences, and which holds a pose without measurements and a parallel and an antiparallel pair
(test_ragged_reference.py asserts all of that, and the reference used here, on the CPU).

Bars: evaluations 1e-12 against the edge-by-edge np.longdouble reference, overall and per pose (relative to the largest
pose block of the reference); manifold ops 1e-13; one RTR Run against the oracle with equal runs / outer_iters /
tCGStatus, fOpt max(1e-11, 2 x ...) and X max(1e-10, 2 x the float64 oracle's own distance from the 64-bit-mantissa
restatement of the same call: measured <= 6e-14 in X and <= 1e-13 in fOpt on this graph, so the bars are 1e-10 and 1e-11);
exact preconditioner 1e-10 (the oracle's sparse LU against a dense solve: 1e-13); engine 1e-9.
Measured on an MI355X: Runs within 1.3e-13 (X) / 1.7e-13 (fOpt) of the oracle over the 111 cases, exact preconditioner
9.3e-14, engine 1e-14 .. 2.5e-13 (L2, GNC_TLS at d = 3) and 8e-11 / 9.5e-11 (GNC_TLS at d = 2, where the oracle is 3e-11 /
4e-11 from its own copy started 1e-16 away).
"""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _ragged as RG
from tests._common import random_point, random_tangent, rel
from tests._extended import optimize_extended

pytestmark = pytest.mark.gpu

TOL = 1e-12
SHAPES = [(2, r) for r in range(2, 9)] + [(3, r) for r in range(3, 9)]  # DPGO_DISPATCH: every compiled (d, r)
SPMM_V2, SV_STAGE, CLASSIC_TCG, DEVICE_CHOL = 11, 8, 5, 12  # tuning keys (kernels.h TuneKey)


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1, "no gfx950 device"
    return H


_cache = {}


def _graph(d):
    """(meas, T_true, Q, single-agent profile) of the ragged graph, computed once per d and never modified."""
    if ("g", d) not in _cache:
        meas, T = RG.ragged_graph(d)
        prof = RG.assert_profile(meas)
        _cache[("g", d)] = (meas, T, O.connection_laplacian(meas, meas.num_poses), prof)
    return _cache[("g", d)]


def _oracle(d, r):
    if ("p", d, r) not in _cache:
        meas, _, Q, _ = _graph(d)
        P = O.QuadraticProblem(meas.num_poses, d, r)
        P.set_Q(Q)
        P.precon_mode = O.PRECON_BLOCK_JACOBI
        _cache[("p", d, r)] = P
    return _cache[("p", d, r)]


def _inputs(d, r):
    """X, V and a G on a few poses, among them two hubs, the pose without measurements and a pose of the cut pair."""
    if ("x", d, r) not in _cache:
        n = RG.N_POSES
        X = random_point(r, d, n, 11)
        V = random_tangent(X, d, 12)
        G = np.zeros_like(X)
        rng = O.SplitMix64(13)
        b = d + 1
        hubs = sorted(RG.HUBS)
        for j in sorted(set(range(0, n, n // 7)) | {hubs[0], hubs[-1], RG.ISOLATED, RG.CUT[0]}):
            for c in range(b):
                for a in range(r):
                    G[a, j * b + c] = rng.normal()
        _cache[("x", d, r)] = (X, V, G)
    return _cache[("x", d, r)]


def _compare(what, got, ref, d, prof, lo=0):
    """got against ref (r x (d+1) n_a, the poses from global pose `lo`): 1e-12 overall and per pose, a failure naming
    the pose, its tile, its degree and whether the tile is staged."""
    r = got.shape[0]
    b = d + 1
    ref64 = np.asarray(ref, np.longdouble)
    diff = (np.asarray(got, np.longdouble) - ref64).astype(float).reshape(r, -1, b)
    refn = np.linalg.norm(ref64.astype(float).reshape(r, -1, b), axis=(0, 2))
    dn = np.linalg.norm(diff, axis=(0, 2))
    worst = int(np.argmax(dn))
    where = RG.describe_pose(prof, d, lo + worst)
    assert dn[worst] <= TOL * refn.max(), f"{what}: {where}: {dn[worst]:.3e} against largest block {refn.max():.3e}"
    tot = float(np.linalg.norm(dn) / max(np.linalg.norm(refn), 1e-300))
    assert tot <= TOL, f"{what}: {tot:.3e} overall, worst {where}"


def _check_evaluations(H, d, r, X, V, refs, prof, offsets=(0, RG.N_POSES)):
    """f, egrad, ehvp, riegrad and its norm, rhvp and the block-Jacobi preconditioner of every agent of H against
    refs[k] = (edge_reference dict, oracle preconditioner output)."""
    b = d + 1
    fh = H.f(X)
    EG, HV = H.egrad(X), H.ehvp(V)
    RGh, norms, _ = H.riegrad(X)
    RH = H.rhvp(X, V)
    PC = H.precondition(X, V)
    for k, (ref, pc) in enumerate(refs):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        sl = slice(lo * b, hi * b)
        # the per-pose quantities first: their failures name the pose and its path
        for what, got, want in (("egrad", EG, ref["egrad"]), ("ehvp", HV, ref["ehvp"]), ("riegrad", RGh, ref["riegrad"]),
                                ("rhvp", RH, ref["rhvp"]), ("precondition", PC, pc)):
            _compare(f"agent {k} {what}", got[:, sl], want, d, prof, lo)
        f = float(ref["f"])
        assert abs(fh[k] - f) <= TOL * max(1.0, abs(f)), (k, fh[k], f)
        gn = float(ref["gradnorm"])
        assert abs(norms[k] - gn) <= TOL * max(gn, 1e-300), (k, norms[k], gn)


def _set_Q(H, meas, Q, fmt, agent=0):
    if fmt == "bsr":
        H.set_Q_scipy(agent, Q)
    else:
        H.set_Q_edges(agent, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau, meas.weight)


def _single_refs(d, r):
    meas, _, _, _ = _graph(d)
    X, V, G = _inputs(d, r)
    P = _oracle(d, r)
    P.set_G(G)
    return [(RG.edge_reference(meas, X, G, V), P.precondition(X, V, O.PRECON_BLOCK_JACOBI))]


# ---------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("fmt", ["bsr", "edges"])
@pytest.mark.parametrize("d,r", SHAPES)
def test_evaluations_all_shapes(hip, d, r, fmt):
    """Every compiled (d, r), Q as BSR and as the edge stream: unstaged tiles (global-memory edge loops), hubs past the
    straight-line limit, an empty block row / a pose without incidences, parallel measurements."""
    meas, _, Q, prof = _graph(d)
    X, V, G = _inputs(d, r)
    H = hip.Problem(meas.num_poses, d, r)
    _set_Q(H, meas, Q, fmt)
    H.set_G_dense(0, G)
    _check_evaluations(H, d, r, X, V, _single_refs(d, r), prof)


# ---------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("sv", [0, 1])
@pytest.mark.parametrize("v2", [0, 3, 6])
@pytest.mark.parametrize("d,r", [(3, 5), (3, 8)])
def test_tuning_variants(hip, d, r, v2, sv):
    """The SpMM generations still compiled in (TUNE_SPMM_V2: 0 the plain accumulator and two pipelines, 3 rotated for the
    merged modes, 6 rotated + one pipeline) with and without the second-visit stage (TUNE_SV_STAGE, whose tables are
    built with Q: set before it), set on the handle only -- the process defaults are not touched."""
    meas, _, Q, prof = _graph(d)
    X, V, G = _inputs(d, r)
    saved = [hip.get_tuning(k) for k in (SPMM_V2, SV_STAGE)]
    try:
        H = hip.Problem(meas.num_poses, d, r)
        H.set_tuning(SPMM_V2, v2)
        H.set_tuning(SV_STAGE, sv)
        _set_Q(H, meas, Q, "edges")
        H.set_G_dense(0, G)
        _check_evaluations(H, d, r, X, V, _single_refs(d, r), prof)
    finally:
        for k, v in zip((SPMM_V2, SV_STAGE), saved):
            hip.set_tuning(k, v)


# ---------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("fmt", ["bsr", "edges"])
@pytest.mark.parametrize("d,r", [(3, 5), (3, 4), (2, 3), (2, 6)])
def test_ragged_agents(hip, d, r, fmt):
    """Agents of 1, 63, 64, 65, 2, 130 and 320 poses in one handle: Q_k is the principal submatrix of the global
    Laplacian on agent k's poses (private edges in full, shared edges on the diagonal only), uploaded as BSR or as the
    agent's edge stream with the other agents' endpoints at -1.  The one-pose agent and both poses of the two-pose
    agent have shared edges only (tiles without any incidence)."""
    meas, _, Q, _ = _graph(d)
    n, b = meas.num_poses, d + 1
    sizes = RG.RAGGED_AGENTS
    off = np.concatenate([[0], np.cumsum(sizes)])
    prof = RG.tile_profile(meas.p1, meas.p2, sizes)
    only_shared = np.nonzero((prof["degree"] == 0) & (prof["shared"] > 0))[0].tolist()
    assert 0 in only_shared and len(only_shared) >= 2 and sizes[0] == 1
    X, V, G = _inputs(d, r)
    H = hip.Problem(None, d, r, poses_per_agent=sizes)
    Qc = Q.tocsr()
    refs = []
    for k in range(len(sizes)):
        lo, hi = int(off[k]), int(off[k + 1])
        in1, in2 = (meas.p1 >= lo) & (meas.p1 < hi), (meas.p2 >= lo) & (meas.p2 < hi)
        sub = meas.subset(np.nonzero(in1 | in2)[0])
        p1 = np.where((sub.p1 >= lo) & (sub.p1 < hi), sub.p1 - lo, -1)
        p2 = np.where((sub.p2 >= lo) & (sub.p2 < hi), sub.p2 - lo, -1)
        Qk = Qc[lo * b:hi * b, lo * b:hi * b]
        if fmt == "bsr":
            H.set_Q_scipy(k, Qk)
        else:
            H.set_Q_edges(k, p1, p2, sub.R, sub.t, sub.kappa, sub.tau)
        sl = slice(lo * b, hi * b)
        H.set_G_dense(k, G[:, sl])
        Pk = O.QuadraticProblem(hi - lo, d, r)
        Pk.set_Q(Qk)
        refs.append((RG.edge_reference(sub, X[:, sl], G[:, sl], V[:, sl], p1, p2),
                     Pk.precondition(X[:, sl], V[:, sl], O.PRECON_BLOCK_JACOBI)))
    _check_evaluations(H, d, r, X, V, refs, prof, off)


# ---------------------------------------------------------------------------------------- (d)
RBCD = dict(tr_iterations=1, tr_tolerance=1e-2, tr_initial_radius=100.0)


def _starts(d, r):
    """The three starts of the Run test and what the oracle does from each (asserted): the lifted ground truth (tCG runs
    all tr_max_inner = 10 iterations), a random point (the first step leaves the region) and a point warmed by oracle
    iterations from the random one until a Run takes 2..5 tCG steps."""
    if ("s", d, r) in _cache:
        return _cache[("s", d, r)]
    _, T, _, _ = _graph(d)
    P = _oracle(d, r)
    P.set_G(np.zeros((r, (d + 1) * RG.N_POSES)))
    op = O.OptParams(tr_max_inner=10, **RBCD)

    def first(X0, inner=10):
        trace = []
        O.optimize(P, X0, O.OptParams(tr_max_inner=inner, **RBCD), trace)
        outer = [t for t in trace if "ninner" in t]
        return outer[0]["ninner"], outer[0]["status"]

    truth = O.lifting_matrix(d, r) @ T
    assert first(truth) == (10, O.TCG_MAXITER)
    rand = random_point(r, d, RG.N_POSES, 71)
    ni, st = first(rand)
    assert ni == 1 and st in (O.TCG_EXCREGION, O.TCG_NEGCURVTURE)
    warm = rand
    for _ in range(40):
        warm, _ = O.optimize(P, warm, op)
        if 2 <= first(warm)[0] <= 5:
            break
    assert 2 <= first(warm)[0] <= 5
    _cache[("s", d, r)] = dict(truth=truth, random=rand, warm=warm)
    return _cache[("s", d, r)]


def _run_case(hip, d, r, start, inner, fmt="edges", classic=0):
    meas, _, Q, _ = _graph(d)
    n = meas.num_poses
    X0 = _starts(d, r)[start]
    P = _oracle(d, r)
    P.set_G(np.zeros((r, (d + 1) * n)))
    trace = []
    Xo, ro = O.optimize(P, X0, O.OptParams(tr_max_inner=inner, **RBCD), trace)
    outer = [t for t in trace if "ninner" in t]
    if start == "truth":
        assert outer[0]["ninner"] == inner and outer[0]["status"] == O.TCG_MAXITER
    # the float64 oracle's own distance from the extended-precision restatement of the same call
    key = ("e", d, r, start, inner)
    if key not in _cache:
        xe, fe, runs_e = optimize_extended(Q, X0, d, RBCD["tr_tolerance"], RBCD["tr_initial_radius"], inner)
        _cache[key] = (xe.astype(float), float(fe), runs_e)
    Xe, fe, runs_e = _cache[key]
    assert runs_e == ro["runs"]
    dist_x, dist_f = rel(Xo, Xe), abs(ro["fOpt"] - fe) / abs(fe)
    print(f"d={d} r={r} {start} inner={inner}: oracle vs extended-precision Run: X {dist_x:.2e}, fOpt {dist_f:.2e}")
    assert dist_x <= 1e-9, "the oracle itself is too far from the extended-precision Run: replace this start"
    saved = hip.get_tuning(CLASSIC_TCG)
    try:
        H = hip.Problem(n, d, r)
        H.set_tuning(CLASSIC_TCG, classic)
        _set_Q(H, meas, Q, fmt)
        Xh, rh = H.optimize(X0, hip.default_params(tr_max_inner=inner, precon=hip.PRECON_BLOCK_JACOBI, **RBCD))
    finally:
        hip.set_tuning(CLASSIC_TCG, saved)
    rh = rh[0]
    assert rh["runs"] == ro["runs"]
    assert rh["outer_iters"] == len(outer)
    assert rh["tCGStatus"] == ro["tCGStatus"]
    err_f, err_x = abs(rh["fOpt"] - ro["fOpt"]) / abs(ro["fOpt"]), rel(Xh, Xo)
    print(f"    device vs oracle: X {err_x:.2e}, fOpt {err_f:.2e}")
    assert err_f <= max(1e-11, 2 * dist_f)
    assert err_x <= max(1e-10, 2 * dist_x)


@pytest.mark.parametrize("start", ["truth", "random", "warm"])
@pytest.mark.parametrize("d,r", SHAPES)
def test_rtr_run_all_shapes(hip, d, r, start):
    """PGOAgent::updateX settings (1 iteration, 10 inner, radius 100, tol 1e-2, block-Jacobi), the default merged tCG over
    the edge stream, at every compiled shape: ten tCG iterations, a first step that leaves the region, 2..5 CG steps."""
    _run_case(hip, d, r, start, 10)


@pytest.mark.parametrize("inner", [4, 1])
@pytest.mark.parametrize("start", ["truth", "random", "warm"])
@pytest.mark.parametrize("d,r", [(3, 5), (3, 6), (2, 4)])
def test_rtr_run_short_tcg(hip, d, r, start, inner):
    """tr_max_inner 4 and 1: the last iteration folded into the retraction is the second-to-last / the first one."""
    _run_case(hip, d, r, start, inner)


@pytest.mark.parametrize("inner", [10, 1])
@pytest.mark.parametrize("start", ["truth", "random", "warm"])
@pytest.mark.parametrize("fmt,classic", [("edges", 1), ("bsr", 0), ("bsr", 1)])
@pytest.mark.parametrize("d,r", [(3, 5), (3, 6), (2, 4)])
def test_rtr_run_classic_and_bsr(hip, d, r, fmt, classic, start, inner):
    """The classic five-launch tCG sequence (TUNE_CLASSIC_TCG = 1) and BSR Q on the same Runs."""
    _run_case(hip, d, r, start, inner, fmt, classic)


# ---------------------------------------------------------------------------------------- (e)
def _weighted(meas, w):
    return O.Measurements(meas.d, meas.r1, meas.r2, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau, w,
                          meas.num_poses)


def _exact_refs(d, r):
    """Oracle outputs of the exact preconditioner (two applications, a third at seeded weights), each first checked
    against a dense solve of the same system: sparse LU and dense LU within 1e-11 (measured 2e-13), so the reference
    carries the 1e-10 bar."""
    if ("c", d, r) in _cache:
        return _cache[("c", d, r)]
    meas, _, Q, _ = _graph(d)
    n = meas.num_poses
    X = random_point(r, d, n, 51)
    Vs = [random_tangent(X, d, 52), random_tangent(X, d, 53), random_tangent(X, d, 54)]
    w = np.array([1.0 - 0.999 * O.SplitMix64(900 + e).uniform() for e in range(meas.m)])  # (0, 1]
    assert w.min() > 0 and w.max() <= 1
    Pw = O.QuadraticProblem(n, d, r)
    Qw = O.connection_laplacian(_weighted(meas, w), n)
    Pw.set_Q(Qw)
    want = []
    for P, Qm, V in ((_oracle(d, r), Q, Vs[0]), (_oracle(d, r), Q, Vs[1]), (Pw, Qw, Vs[2])):
        z = P.precondition(X, V, O.PRECON_EXACT)
        dense = np.linalg.solve(Qm.toarray() + 0.1 * np.eye(Qm.shape[0]), V.T).T
        gap = rel(z, O.tangent_project(X, dense, d))
        print(f"d={d} r={r}: sparse LU vs dense solve {gap:.2e}")
        assert gap <= 1e-11
        want.append(z)
    _cache[("c", d, r)] = (X, Vs, w, want)
    return _cache[("c", d, r)]


@pytest.mark.parametrize("how", ["edges-device", "edges-host", "bsr"])
@pytest.mark.parametrize("d,r", [(3, 5), (3, 8), (2, 2), (2, 4), (3, 7)])
def test_exact_precondition_ragged(hip, d, r, how):
    """Exact preconditioner on the ragged graph: a disconnected pattern (the pose without measurements is its own tree),
    parallel measurements summed into one frontal entry, device and host numeric factorisation; two applications, then
    an on-device reweighting and a third against the reweighted oracle."""
    import torch
    meas, _, Q, _ = _graph(d)
    X, Vs, w, want = _exact_refs(d, r)
    H = hip.Problem(meas.num_poses, d, r)
    if how != "bsr":
        H.set_tuning(DEVICE_CHOL, 1 if how == "edges-device" else 0)
    _set_Q(H, meas, Q, "bsr" if how == "bsr" else "edges")
    H.set_precon(hip.PRECON_EXACT)
    for V, z in zip(Vs[:2], want[:2]):
        err = rel(H.precondition(X, V), z)
        print(f"{how} d={d} r={r}: {err:.2e}")
        assert err <= 1e-10
    assert not H.exact_fallback_agents().any()
    if how == "bsr":
        H.set_Q_scipy(0, O.connection_laplacian(_weighted(meas, w), meas.num_poses))
    else:
        wd = torch.tensor(w, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        H.set_edge_weights_dev(wd.data_ptr())
    err = rel(H.precondition(X, Vs[2]), want[2])
    print(f"{how} d={d} r={r} reweighted: {err:.2e}")
    assert err <= 1e-10
    assert not H.exact_fallback_agents().any()


# ---------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("d,r", SHAPES)
def test_manifold_ops_all_shapes(hip, d, r):
    """tangent_project, retract_qf and project_polar at every compiled (d, r), n = 130: tiles of 64, 64 and 2 poses."""
    n = 130
    X = random_point(r, d, n, 21)
    V = random_tangent(X, d, 22)
    assert rel(hip.tangent_project(X, V + X, d), O.tangent_project(X, V + X, d)) <= TOL
    assert rel(hip.retract_qf(X, V, d), O.retract_qf(X, V, d)) <= 1e-13
    assert rel(hip.retract_qf(X, V, d, scale=-0.25), O.retract_qf(X, -0.25 * V, d)) <= 1e-13
    for eps in (0.3, 0.01, 2.0):  # Jacobi fallback / Newton-Schulz fast path / far from St(d,r)
        M = X + eps * V
        assert rel(hip.project_polar(M, d), O.lifted_project(M, d)) <= 1e-13


# ---------------------------------------------------------------------------------------- (g)
ENGINE_AGENTS = [50, 130, 64, 97, 120, 65, 119]
ENGINE_ITERS = 6


def engine_case(d, r, robust):
    """(meas, agent_of_pose, X0) of the engine test: the ragged graph, for GNC_TLS with 10 % of its loop closures
    corrupted (translations + N(0, 5), as test_gpu_rbcd._grid_with_outliers), 7 agents over unequal contiguous ranges,
    from the lifted ground truth."""
    meas, T, _, _ = _graph(d)
    if robust != "L2":
        rng = np.random.default_rng(7)
        lc = np.nonzero(np.abs(meas.p2 - meas.p1) != 1)[0]
        bad = rng.choice(lc, size=max(1, int(0.1 * len(lc))), replace=False)
        t = meas.t.copy()
        t[bad] += rng.normal(0.0, 5.0, size=(len(bad), d))
        meas = O.Measurements(d, meas.r1, meas.r2, meas.p1, meas.p2, meas.R, t, meas.kappa, meas.tau, meas.weight,
                              meas.num_poses)
    assert sum(ENGINE_AGENTS) == meas.num_poses
    aop = np.repeat(np.arange(len(ENGINE_AGENTS)), ENGINE_AGENTS).astype(np.int32)
    return meas, aop, O.lifting_matrix(d, r) @ T


def engine_oracle(d, r, accel, robust, X0=None):
    meas, aop, X = engine_case(d, r, robust)
    Xo, colors = O.colour_rbcd(meas, aop, len(ENGINE_AGENTS), X if X0 is None else X0, ENGINE_ITERS, r,
                               acceleration=accel, robust=robust, robust_opt_inner_iters=3)
    return Xo, colors


@pytest.mark.parametrize("robust", ["L2", "GNC_TLS"])
@pytest.mark.parametrize("accel", [False, True])
@pytest.mark.parametrize("d,r", [(3, 4), (2, 4)])
def test_engine_ragged(hip, d, r, accel, robust):
    """The RBCD engine on the ragged graph: 7 agents of 50..130 poses, 6 colour-schedule steps, with and without
    acceleration, L2 and GNC_TLS (reweighting at iterations 2 and 5), against the oracle's colour schedule at the
    engine's 1e-9.  The oracle's Agent takes the pose without measurements as it is (a zero row of Q).  Before the bar
    is trusted the oracle runs a second time from X0 with 1e-16 relative noise: the two runs stay within 5e-10
    (measured on the CPU: 1e-15 .. 5e-15 at d = 3, 5e-14 .. 4.4e-11 at d = 2, GNC_TLS the largest), so a float64 implementation that rounds differently can
    stay within 1e-9 of it."""
    meas, aop, X0 = engine_case(d, r, robust)
    Xo, colors = engine_oracle(d, r, accel, robust)
    noise = np.random.default_rng(3).standard_normal(X0.shape)
    Xt, _ = engine_oracle(d, r, accel, robust, X0 * (1.0 + 1e-16 * noise))
    twin = rel(Xt, Xo)
    print(f"d={d} r={r} accel={accel} {robust}: oracle vs its perturbed twin {twin:.2e}")
    assert twin <= 5e-10
    g = hip.Graph.from_arrays(d, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    e = hip.Rbcd(g, aop, np.zeros(len(ENGINE_AGENTS), np.int32), 0, 1,
                 hip.rbcd_params(r=r, acceleration=int(accel), robust_cost=hip.ROBUST[robust],
                                 robust_opt_inner_iters=3))
    e.set_X(X0)
    for it in range(ENGINE_ITERS):
        c = it % e.num_colors
        e.pre_exchange(c)
        e.update(c, None)
    out = np.zeros(X0.size)
    e.get_X_into(out)
    assert list(e.color_of_agent) == colors
    err = rel(hip.from_dev_layout(out, r), Xo)
    print(f"    engine vs oracle {err:.2e}")
    assert err <= 1e-9
