"""GPU tests of the rank staircase (dpgo_hip_escape / dpgo_graph_escape / dpgo_amd.staircase) on the ring pose
graphs of tests/_ring.py, whose winding-2 configuration is a strict local minimum of the rank-d relaxation that is
not global (tests/test_ring_reference.py checks that ground on the CPU).  Build-defined, absent from the reference:
pinned against the numpy restatement in tests/_ring.py (the oracle's retract_qf, certificate_matrix and PGOAgent)."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _ring as RG
from tests._common import load_meas, rel

pytestmark = pytest.mark.gpu

AOP = np.array([0] * 5 + [1] * 4 + [2] * 3, np.int32)  # 3 agents of 5 / 4 / 3 consecutive poses


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


@pytest.fixture(scope="module", params=[2, 3])
def ring(request, hip):
    """The ring, its winding-2 point, numpy's eigenpair of the certificate matrix and the numpy line searches (shared,
    read-only)."""
    d = request.param
    meas = RG.ring(d)
    Q = O.connection_laplacian(meas, meas.num_poses)
    X = RG.winding2(meas)
    lam, v = RG.min_eig(Q, X, d)
    ref = {a0: RG.line_search(Q, X, v, lam, d, alpha0=a0) for a0 in (1.0, 64.0)}
    g = hip.Graph.from_arrays(d, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    for a in (X, v):
        a.setflags(write=False)
    return dict(d=d, meas=meas, Q=Q, X=X, lam=lam, v=v, ref=ref, g=g)


def _next_problem(H, ring):
    meas, d = ring["meas"], ring["d"]
    P = H.Problem(meas.num_poses, d, d + 1)
    P.set_Q_edges(0, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau, meas.weight)
    return P


@pytest.mark.parametrize("alpha0,alpha,trials", [(1.0, 1.0, 1), (64.0, 2.0, 6)])
def test_line_search_matches_numpy(hip, ring, alpha0, alpha, trials):
    d, X, v, lam = ring["d"], ring["X"], ring["v"], ring["lam"]
    Xw, want = ring["ref"][alpha0]
    assert (want["accepted"], want["trials"], want["alpha"]) == (1, trials, alpha)
    Xg, got = _next_problem(hip, ring).escape(X, v, lam, hip.escape_params(alpha0=alpha0))
    assert got["accepted"] == 1
    assert got["trials"] == trials
    assert got["alpha"] == alpha
    fb = want["f_before"]
    assert abs(got["f_before"] - fb) <= 1e-12 * fb, (got, want)
    assert abs(got["f_after"] - want["f_after"]) <= 1e-12 * fb, (got, want)
    assert abs(got["gradnorm_after"] - want["gradnorm_after"]) <= 1e-10, (got, want)
    assert got["f_after"] <= got["f_before"] + 0.25 * alpha * alpha * lam
    assert rel(Xg, Xw) <= 1e-13


def test_rejected_escape_returns_the_plain_lift(hip, ring):
    d, X, v, lam = ring["d"], ring["X"], ring["v"], ring["lam"]
    Xg, got = _next_problem(hip, ring).escape(X, v, lam, hip.escape_params(min_gradnorm=10.0))
    assert got["accepted"] == 0 and got["trials"] == 1 and got["alpha"] == 1.0
    assert got["gradnorm_after"] > 0.1 and got["f_after"] < got["f_before"]  # info is still filled
    assert np.array_equal(Xg, RG.lift(X))


def test_escape_refuses_bad_arguments(hip, ring):
    d, X, v, lam = ring["d"], ring["X"], ring["v"], ring["lam"]
    n = ring["meas"].num_poses
    P = _next_problem(hip, ring)
    with pytest.raises(hip.DPGOHipError, match="negative"):
        P.escape(X, v, 1.0)
    with pytest.raises(hip.DPGOHipError, match="negative"):
        P.escape(X, v, 0.0)
    with pytest.raises(hip.DPGOHipError):  # rank mismatch: X is not of rank handle - 1
        P.escape(RG.lift(X), v, lam)
    B = hip.Problem(None, d, d + 1, poses_per_agent=[n // 2, n - n // 2])
    with pytest.raises(hip.DPGOHipError, match="single-agent"):
        B.escape(X, v, lam)
    with pytest.raises(hip.DPGOHipError, match="not compiled"):
        ring["g"].escape(np.zeros((8, (d + 1) * n)), 8, v, lam)


def test_graph_escape_from_the_device_certificate(hip, ring):
    """Graph.escape fed Graph.certify's own Ritz matrix.  lambda_min is a double eigenvalue, so the vector is not
    compared: alpha, the decrease inequality, and f_after against the numpy line search along the same direction
    (1e-9: the Ritz pair's accuracy)."""
    d, X, g, Q = ring["d"], ring["X"], ring["g"], ring["Q"]
    c = g.certify(X, d, max_iters=100, tol=1e-10, want_vector=True)
    assert abs(c["lambda_min"] - ring["lam"]) <= 1e-8
    Xf, got = g.escape(X, d, c["eigvec"], c["lambda_min"])
    v = RG.escape_direction(c["eigvec"])
    assert rel(hip.escape_direction(c["eigvec"], d), v) <= 1e-14
    Xw, want = RG.line_search(Q, X, v, c["lambda_min"], d)
    assert got["accepted"] == 1 and got["alpha"] == 1.0 and got["trials"] == 1
    assert abs(got["f_after"] - want["f_after"]) <= 1e-9
    assert got["f_after"] <= got["f_before"] + 0.25 * c["lambda_min"]
    assert abs(got["f_before"] - RG.F_CRIT) <= 1e-12 * RG.F_CRIT
    assert Xf.shape == ((d + 1) * X.shape[1],)


def _engine(H, ring, r, accel, tolerance=1e-2):
    return H.Rbcd(ring["g"], AOP, np.zeros(3, np.int32), 0, 1,
                  H.rbcd_params(r=r, acceleration=int(accel), tolerance=tolerance, precon=H.PRECON_BLOCK_JACOBI))


@pytest.mark.parametrize("accel", [False, True])
def test_control_engine_stays_at_the_uncertified_point(hip, ring, accel):
    """What the feature changes: without it the engine at r = d sits at the winding-2 point (every agent's solve
    returns its input below its tolerance) and the certificate only says no.  Passes without the staircase."""
    d, X, g = ring["d"], ring["X"], ring["g"]
    e = _engine(hip, ring, d, accel, tolerance=1e-9)
    e.set_X(X)
    for it in range(50):
        e.pre_exchange(it % e.num_colors)
        e.update(it % e.num_colors, None)
    f, gsq = e.central_eval()
    assert abs(f - RG.F_CRIT) <= 1e-12
    Xd = np.zeros(X.size)
    e.get_X_into(Xd)
    assert g.certify(Xd, d, max_iters=100, tol=1e-10)["lambda_min"] < -0.1


# twice the longest level of the CPU replay that reached grad_tol (d = 3, rank 4, Nesterov off: 1,322 steps)
MAX_STEPS = 2644


@pytest.mark.parametrize("accel", [False, True])
def test_staircase_reaches_the_certified_optimum(hip, ring, accel):
    """staircase.solve from the winding-2 point: 3 agents (5 / 4 / 3 poses), L2, block-Jacobi, tolerance 1e-9,
    grad_tol 1e-7, eta 1e-6.

    The schedule replayed on the CPU (tests/_ring.py staircase_rbcd: the oracle's PGOAgent colour schedule, the dense
    certificate, the numpy escape) takes the ranks of the RTR staircase, d -> d + 1 -> d + 2, every escape at alpha = 1:
      d = 3:  rank 3: 0 steps, f 3.215390, lambda_min -0.1304;  rank 4: 1,322 steps (Nesterov: 741), f 1.607695,
              lambda_min -0.2679;  rank 5: 70 (72) steps, f 4e-15, lambda_min -4e-12.
      d = 2:  rank 2: 0 steps, f 3.215390, lambda_min -0.1304;  rank 3: |RieGrad| is still 4.5e-6 after 20,000 steps
              (sublinear: the rank-3 minimum is degenerate), f 2.188809, lambda_min -0.1791;  rank 4: 91 (94) steps,
              f 5e-15, lambda_min -5e-9.
    The d = 2 rank-3 level therefore ends at max_steps in the replay too (at 2,644 steps: |RieGrad| 4.7e-6 (6.3e-6),
    f 2.188809, lambda_min -0.1791, then rank 4 as above): its step count is not asserted to be below max_steps."""
    from dpgo_amd import staircase
    d, X, g = ring["d"], ring["X"], ring["g"]
    p = hip.rbcd_params(acceleration=int(accel), tolerance=1e-9, precon=hip.PRECON_BLOCK_JACOBI,
                        robust_cost=hip.ROBUST["L2"])
    Xf, r, levels = staircase.solve(g, AOP, np.zeros(3, np.int32), X, d, p, eta=1e-6, grad_tol=1e-7,
                                    max_steps=MAX_STEPS, cert=dict(max_iters=100, tol=1e-10))
    print(levels)
    assert [lv["r"] for lv in levels] == [d, d + 1, d + 2]
    assert r == d + 2 and r <= 8
    assert levels[-1]["lambda_min"] >= -1e-6
    assert levels[-1]["f"] <= 1e-8
    assert sum(1 for lv in levels if lv["trials"] > 0) >= 1 and all(lv["alpha"] > 0 for lv in levels[:-1])
    assert all(a["f"] > b["f"] for a, b in zip(levels, levels[1:]))
    assert levels[0]["steps"] == 0 and abs(levels[0]["f"] - RG.F_CRIT) <= 1e-12
    assert all(lv["steps"] <= MAX_STEPS for lv in levels)
    if d == 3:
        assert all(lv["steps"] < MAX_STEPS for lv in levels)
    Xm = hip.from_dev_layout(Xf, r)
    assert RG.cost(ring["Q"], Xm) <= 1e-8
    assert RG.min_eig(ring["Q"], Xm, d)[0] >= -1e-6


def test_staircase_single_rank_only(hip, ring):
    from dpgo_amd import staircase
    with pytest.raises(staircase.StaircaseError, match="one rank"):
        staircase.solve(ring["g"], AOP, np.array([0, 1, 0], np.int32), ring["X"], ring["d"])


def test_staircase_noop_level_at_a_certified_optimum(hip):
    """From the RTR optimum of smallGrid3D (where tests/test_gpu_certify.py certifies) the staircase returns after
    one level with no step and no escape.  eta is that test's bar, 1e-6 of the Gershgorin bound of S."""
    from dpgo_amd import staircase
    meas = load_meas("smallGrid3D")
    d, n, r = meas.d, meas.num_poses, 5
    Q = O.connection_laplacian(meas, n)
    X0 = O.lifting_matrix(d, r) @ O.chordal_initialization(d, n, meas)
    P = hip.Problem(n, d, r)
    P.set_Q_scipy(0, Q)
    Xo, _ = P.optimize(X0, hip.default_params(tr_iterations=100, tr_tolerance=1e-10, tr_max_inner=200,
                                              precon=hip.PRECON_EXACT))
    lam_bound = float(abs(O.certificate_matrix(Q, Xo, d)).sum(axis=1).max())
    g = hip.Graph.from_arrays(d, n, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    aop = np.minimum(np.arange(n) // (n // 5), 4).astype(np.int32)
    Xf, rf, levels = staircase.solve(g, aop, np.zeros(5, np.int32), Xo, r, hip.rbcd_params(acceleration=1),
                                     eta=1e-6 * lam_bound, grad_tol=1e-6, max_steps=10,
                                     cert=dict(max_iters=1500, tol=1e-10))
    assert rf == r and len(levels) == 1
    assert levels[0]["steps"] == 0 and levels[0]["trials"] == 0 and levels[0]["alpha"] == 0.0
    assert np.array_equal(Xf, hip.to_dev_layout(Xo))
