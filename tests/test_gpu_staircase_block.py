"""GPU tests of staircase.solve(certifier="lobpcg"): the block certificate must take the staircase where the Lanczos
certificate takes it.

tinyGrid3D from the golden rank-3 RTR result (tests/_cholcert.py's OPT_TINY, lambda_min = -1.10e-3), 3 agents of 3
poses, L2, block-Jacobi, tolerance 1e-9, grad_tol 1e-7, eta = 1e-6 |lambda|_max of the start's certificate matrix:
certified rank and final cost equal the "lanczos" run's, the cost to 1e-9 relative.  Measured on an MI355X: that
start is not critical at grad_tol (its coupling |(I - U U^T) S U| is 9.2e-3), the rank-3 engine takes 117 steps from
it to f = 9.259682164563628, |RieGrad| 6.0e-8, and there both certificates hold at rank 3 (Lanczos lambda_min
6.5e-12; block lambda_min -3.1e-9, lower_bound -3.1e-9): the negative eigenvalue belonged to the unconverged start,
and neither certifier escapes to rank 4 on this dataset.

The escape itself is covered on the ring of tests/_ring.py (d = 3) with tests/test_gpu_staircase_chol.py's setup: from
the winding-2 critical point the staircase climbs 3 -> 4 -> 5 along the block certificate's vectors, as the default
run does, and ends certified by the bound at the same cost.  The ring's optimum has cost exactly 0, so "equal to 1e-9
relative" is taken relative to max(|f_default|, f(X0)) there, as that file explains.  The ring runs with flags = 0
(no locked block): its rank-5 optimum has rank 4 and its rows span S's whole null space, the translation gauge
included, so the gauge's remainder after Gram-Schmidt is the iterate's rounding (above the 1e-10 drop rule) and the
seed it leaves is a noise direction: measured coupling 0.93, lower_bound -0.85 at lambda_min -8.6e-13 -- a valid
bound, but no certificate.  Without U the r = 5 rows cover the four null vectors and the bound is
theta - residual."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _cholcert as CC
from tests import _ring as RG

pytestmark = pytest.mark.gpu

MAX_STEPS = 2644  # tests/test_gpu_escape.py's


def test_lobpcg_certifier_on_tinygrid_as_the_default():
    from dpgo_amd import hip as H
    from dpgo_amd import staircase
    assert H.device_count() >= 1
    c = CC.case(CC.OPT_TINY)
    m, d = c.meas, c.d
    aop = np.repeat(np.arange(3, dtype=np.int32), 3)
    Q = O.connection_laplacian(m, c.n)
    g = H.Graph.from_arrays(d, c.n, m.p1, m.p2, m.R, m.t, m.kappa, m.tau)
    p = H.rbcd_params(acceleration=1, tolerance=1e-9, precon=H.PRECON_BLOCK_JACOBI, robust_cost=H.ROBUST["L2"])
    kw = dict(eta=1e-6 * c.lam_max, grad_tol=1e-7, max_steps=MAX_STEPS)
    Xd, rd, ld = staircase.solve(g, aop, np.zeros(3, np.int32), c.X, c.r, p, cert=dict(max_iters=100, tol=1e-10), **kw)
    Xb, rb, lb = staircase.solve(g, aop, np.zeros(3, np.int32), c.X, c.r, p, certifier="lobpcg", **kw)
    print(ld)
    print(lb)
    assert all(set(lv) == {"r", "steps", "f", "gradnorm", "lambda_min", "alpha", "trials"} for lv in ld)
    assert ld[-1]["lambda_min"] >= -kw["eta"]
    assert rb == rd and [lv["r"] for lv in lb] == [lv["r"] for lv in ld]
    assert [lv["bound_ok"] for lv in lb] == [False] * (len(lb) - 1) + [True]
    assert lb[-1]["lower_bound"] >= -kw["eta"] and lb[-1]["iters"] >= 1
    assert all(lv["steps"] < MAX_STEPS for lv in ld + lb)

    def cost(X, r):
        Xm = H.from_dev_layout(X, r)
        return 0.5 * float(np.sum(np.asarray((Q @ Xm.T).T) * Xm))
    fd, fb = cost(Xd, rd), cost(Xb, rb)
    print("final cost: lanczos", fd, "lobpcg", fb)
    assert abs(fb - fd) <= 1e-9 * abs(fd)
    Sb = O.certificate_matrix(Q, H.from_dev_layout(Xb, rb), d).toarray()
    assert float(np.linalg.eigvalsh(0.5 * (Sb + Sb.T))[0]) >= -kw["eta"]


def test_lobpcg_certifier_climbs_the_ring_as_the_default():
    from dpgo_amd import hip as H
    from dpgo_amd import staircase
    d = 3
    aop = np.array([0] * 5 + [1] * 4 + [2] * 3, np.int32)
    meas = RG.ring(d)
    Q = O.connection_laplacian(meas, meas.num_poses)
    X = RG.winding2(meas)
    g = H.Graph.from_arrays(d, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    p = H.rbcd_params(acceleration=1, tolerance=1e-9, precon=H.PRECON_BLOCK_JACOBI, robust_cost=H.ROBUST["L2"])
    kw = dict(eta=1e-6, grad_tol=1e-7, max_steps=MAX_STEPS)
    Xd, rd, ld = staircase.solve(g, aop, np.zeros(3, np.int32), X, d, p, cert=dict(max_iters=100, tol=1e-10), **kw)
    Xb, rb, lb = staircase.solve(g, aop, np.zeros(3, np.int32), X, d, p, certifier="lobpcg", cert=dict(flags=0), **kw)
    print(ld)
    print(lb)
    assert rd == d + 2 and [lv["r"] for lv in ld] == [d, d + 1, d + 2]
    assert rb == rd and [lv["r"] for lv in lb] == [lv["r"] for lv in ld]
    assert [lv["bound_ok"] for lv in lb] == [False, False, True]
    assert lb[-1]["lower_bound"] >= -1e-6
    for a, b in zip(lb[:-1], ld[:-1]):  # the uncertified levels: the same eigenvalue, an accepted escape
        assert abs(a["lambda_min"] - b["lambda_min"]) <= 1e-6 * max(1.0, abs(b["lambda_min"]))
        assert a["lambda_min"] < -1e-6 and a["lower_bound"] <= a["lambda_min"] and a["alpha"] > 0.0
    fd, fb = RG.cost(Q, H.from_dev_layout(Xd, rd)), RG.cost(Q, H.from_dev_layout(Xb, rb))
    print("final cost: lanczos", fd, "lobpcg", fb)
    assert fd <= 1e-8 and fb <= 1e-8
    assert abs(fb - fd) <= 1e-9 * max(abs(fd), RG.F_CRIT)
    assert RG.min_eig(Q, H.from_dev_layout(Xb, rb), d)[0] >= -1e-6
