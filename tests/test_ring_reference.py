"""The ground the rank-staircase GPU tests stand on, checked on the CPU: the ring's winding-2 configuration is a
strict local minimum of the rank-d relaxation that is not global, the numpy escape leaves it, and the numpy staircase
reaches the certified global optimum.  Also hip.escape_direction (host only) against numpy."""
import math

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _ring as RG


@pytest.fixture(scope="module", params=[2, 3])
def case(request):
    d = request.param
    meas = RG.ring(d)
    Q = O.connection_laplacian(meas, meas.num_poses)
    X = RG.winding2(meas)
    lam, v = RG.min_eig(Q, X, d)
    return d, meas, Q, X, lam, v


def test_winding2_is_an_uncertified_critical_point(case):
    d, meas, Q, X, lam, v = case
    assert RG.gradnorm(Q, X, d) < 1e-12
    assert abs(RG.cost(Q, X) - RG.F_CRIT) <= 1e-12
    assert abs(RG.F_CRIT - 3.215390309173) <= 1e-11
    assert lam < -0.1
    w = np.linalg.eigvalsh(O.certificate_matrix(Q, X, d).toarray())
    assert abs(w[1] - w[0]) <= 1e-10  # a double eigenvalue


def test_winding2_is_a_strict_local_minimum(case):
    """RTR from a 1e-2 tangent perturbation returns to f_crit."""
    d, meas, Q, X, lam, v = case
    n = meas.num_poses
    rng = np.random.default_rng(5)
    V = O.tangent_project(X, rng.standard_normal(X.shape), d)
    X1 = O.retract_qf(X, 1e-2 * V / np.linalg.norm(V), d)
    assert RG.cost(Q, X1) > RG.F_CRIT
    P = O.QuadraticProblem(n, d, d)
    P.set_Q(Q)
    # to 1e-6: at r = d = 3 the Hessian is singular along the gauge and RTR stalls near 1e-7 (measured: f - f_crit =
    # 2e-15 after 2 iterations, d = 2 and 3)
    Xr, _, _, info = O.rtr_run(P, X1, 1e-6, 10.0, 1e3, 50, 200)
    assert info["iters"] <= 5 and info["ngf"] < 1e-6
    assert abs(info["f"] - RG.F_CRIT) <= 1e-10


def test_escape_line_search(case):
    d, meas, Q, X, lam, v = case
    Xp, e1 = RG.line_search(Q, X, v, lam, d, alpha0=1.0)
    assert (e1["accepted"], e1["trials"], e1["alpha"]) == (1, 1, 1.0)
    assert abs(e1["f_before"] - RG.F_CRIT) <= 1e-12
    assert e1["f_after"] <= e1["f_before"] + 0.25 * lam
    assert e1["gradnorm_after"] > 0.1
    assert Xp.shape[0] == d + 1
    Xp, e64 = RG.line_search(Q, X, v, lam, d, alpha0=64.0)
    assert (e64["accepted"], e64["trials"], e64["alpha"]) == (1, 6, 2.0)
    assert e64["f_after"] <= e64["f_before"] + 0.25 * 4.0 * lam
    if d == 2:
        assert abs(e1["f_after"] - 3.153767) <= 1e-6 and abs(e1["gradnorm_after"] - 0.132) <= 1e-3
        assert abs(e64["f_after"] - 3.005016) <= 1e-6 and abs(e64["gradnorm_after"] - 0.281) <= 1e-3
    # the rejected escape and the plain lift
    Xl, e = RG.line_search(Q, X, v, lam, d, min_gradnorm=10.0)
    assert e["accepted"] == 0 and np.array_equal(Xl, RG.lift(X))


def test_plain_lift_is_a_fixed_point(case):
    """The control: [X; 0] without the escape step is critical at rank d + 1 as well."""
    d, meas, Q, X, lam, v = case
    P = O.QuadraticProblem(meas.num_poses, d, d + 1)
    P.set_Q(Q)
    Xr, _, _, info = O.rtr_run(P, RG.lift(X), 1e-9, 10.0, 1e3, 100, 200)
    assert info["iters"] == 0 and abs(info["f"] - RG.F_CRIT) <= 1e-12


def test_numpy_staircase_certifies(case):
    d, meas, Q, X, lam, v = case
    Xs, levels = RG.staircase_rtr(meas, X)
    assert [lv["r"] for lv in levels] == [d, d + 1, d + 2]
    assert all(a["f"] > b["f"] for a, b in zip(levels, levels[1:]))
    assert levels[-1]["f"] <= 1e-12 and levels[-1]["lambda_min"] >= -1e-9
    assert levels[0]["lambda_min"] < -0.1 and levels[1]["lambda_min"] < -0.1
    assert Xs.shape[0] == d + 2


@pytest.mark.parametrize("r,d,n", [(1, 2, 7), (3, 2, 12), (5, 3, 9)])
def test_escape_direction_matches_numpy(r, d, n):
    from dpgo_amd import hip as H
    rng = np.random.default_rng(11 * r + d)
    V = rng.standard_normal((r, (d + 1) * n)) * rng.uniform(0.1, 2.0, size=(r, 1))
    if r > 1:
        V[1] = 0.0  # a zero row is never the direction
    got = H.escape_direction(V if r > 1 else V[0], d)
    want = RG.escape_direction(V)
    assert got.shape == ((d + 1) * n,)
    assert np.linalg.norm(got - want) <= 1e-15 * math.sqrt(got.size) * 4
    assert abs(np.linalg.norm(got) - 1.0) <= 1e-15 * 4
    with pytest.raises(H.DPGOHipError):
        H.escape_direction(np.zeros((r, (d + 1) * n)), d)
