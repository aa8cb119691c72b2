"""GPU test of staircase.solve(certifier="chol") on the ring pose graphs of tests/_ring.py, with
tests/test_gpu_escape.py's setup: 3 agents (5 / 4 / 3 poses), L2, block-Jacobi, tolerance 1e-9, grad_tol 1e-7,
eta 1e-6.  The staircase climbs d -> d + 2 there with the Lanczos certificate; with the Cholesky certificate it
must climb the same ranks, end certified, and reach the same cost.

The cost bar: the ring's optimum has cost exactly 0 and both runs end at rounding level (f <= 1e-8 is what
tests/test_gpu_escape.py asserts of the default run), where a ratio of the two costs carries no information.  "Equal
to 1e-9 relative" is therefore taken relative to the problem's cost scale, max(|f_default|, f(X0)) with f(X0) =
_ring.F_CRIT the cost the solve starts from, and the default run's own bar is asserted of both."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _ring as RG

pytestmark = pytest.mark.gpu

AOP = np.array([0] * 5 + [1] * 4 + [2] * 3, np.int32)
MAX_STEPS = 2644  # tests/test_gpu_escape.py's


@pytest.mark.parametrize("d", [2, 3])
def test_chol_certifier_climbs_as_the_default(d):
    from dpgo_amd import hip as H
    from dpgo_amd import staircase
    assert H.device_count() >= 1
    meas = RG.ring(d)
    Q = O.connection_laplacian(meas, meas.num_poses)
    X = RG.winding2(meas)
    g = H.Graph.from_arrays(d, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    p = H.rbcd_params(acceleration=1, tolerance=1e-9, precon=H.PRECON_BLOCK_JACOBI, robust_cost=H.ROBUST["L2"])
    kw = dict(eta=1e-6, grad_tol=1e-7, max_steps=MAX_STEPS)
    Xd, rd, ld = staircase.solve(g, AOP, np.zeros(3, np.int32), X, d, p, cert=dict(max_iters=100, tol=1e-10), **kw)
    Xc, rc, lc = staircase.solve(g, AOP, np.zeros(3, np.int32), X, d, p, certifier="chol", **kw)
    print(ld)
    print(lc)
    # the default run is what it always was (tests/test_gpu_staircase_reduce.py's statement of it)
    assert rd == d + 2 and [lv["r"] for lv in ld] == [d, d + 1, d + 2]
    assert all(set(lv) == {"r", "steps", "f", "gradnorm", "lambda_min", "alpha", "trials"} for lv in ld)
    assert ld[-1]["lambda_min"] >= -1e-6 and ld[-1]["f"] <= 1e-8
    # the same climb, certified at the end by the factorisation itself
    assert rc == rd and [lv["r"] for lv in lc] == [lv["r"] for lv in ld]
    assert [lv["pd"] for lv in lc] == [False, False, True] and not any(lv["fallback"] for lv in lc)
    assert lc[-1]["lambda_min"] == -1e-6 and lc[-1]["factorisations"] == 1 and lc[-1]["invit_iters"] == 0
    for a, b in zip(lc[:-1], ld[:-1]):  # the uncertified levels: the same eigenvalue, an accepted escape
        assert abs(a["lambda_min"] - b["lambda_min"]) <= 1e-6 * max(1.0, abs(b["lambda_min"]))
        assert a["lambda_min"] < -1e-6 and a["alpha"] > 0.0 and a["factorisations"] >= 3 and a["invit_iters"] >= 1
    fd, fc = RG.cost(Q, H.from_dev_layout(Xd, rd)), RG.cost(Q, H.from_dev_layout(Xc, rc))
    print("final cost: default", fd, "chol", fc)
    assert fd <= 1e-8 and fc <= 1e-8
    assert abs(fc - fd) <= 1e-9 * max(abs(fd), RG.F_CRIT)
    assert RG.min_eig(Q, H.from_dev_layout(Xc, rc), d)[0] >= -1e-6


def test_unknown_certifier():
    from dpgo_amd import hip as H
    from dpgo_amd import staircase
    meas = RG.ring(3)
    g = H.Graph.from_arrays(3, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    with pytest.raises(staircase.StaircaseError, match="certifier"):
        staircase.solve(g, AOP, np.zeros(3, np.int32), RG.winding2(meas), 3, certifier="arpack")
