"""GPU test of the staircase's way down (dpgo_amd.staircase.solve(..., reduce_tol=...)) on the ring pose graphs of
tests/_ring.py, with tests/test_gpu_escape.py's setup: 3 agents (5 / 4 / 3 poses), L2, block-Jacobi, tolerance 1e-9,
grad_tol 1e-7, eta 1e-6.  The staircase climbs d -> d + 2 there; its certified iterate has numerical rank d
(tests/test_rank_reduce_reference.py), so with reduce_tol the solve must come back at rank d, certified."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _ring as RG

pytestmark = pytest.mark.gpu

AOP = np.array([0] * 5 + [1] * 4 + [2] * 3, np.int32)
MAX_STEPS = 2644  # tests/test_gpu_escape.py's: twice the longest level of the CPU replay that reached grad_tol


@pytest.fixture(scope="module", params=[2, 3])
def runs(request):
    """Both solves from the winding-2 point, once per d (shared, read-only)."""
    from dpgo_amd import hip as H
    from dpgo_amd import staircase
    assert H.device_count() >= 1
    d = request.param
    meas = RG.ring(d)
    Q = O.connection_laplacian(meas, meas.num_poses)
    X = RG.winding2(meas)
    g = H.Graph.from_arrays(d, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    p = H.rbcd_params(acceleration=1, tolerance=1e-9, precon=H.PRECON_BLOCK_JACOBI, robust_cost=H.ROBUST["L2"])
    kw = dict(eta=1e-6, grad_tol=1e-7, max_steps=MAX_STEPS, cert=dict(max_iters=100, tol=1e-10))
    plain = staircase.solve(g, AOP, np.zeros(3, np.int32), X, d, p, reduce_tol=None, **kw)
    reduced = staircase.solve(g, AOP, np.zeros(3, np.int32), X, d, p, reduce_tol=1e-6, **kw)
    return dict(d=d, Q=Q, H=H, plain=plain, reduced=reduced)


def test_reduce_tol_none_returns_what_it_always_did(runs):
    """reduce_tol=None (the default): the certified rank d + 2 iterate and the plain level records, as
    tests/test_gpu_escape.py expects them."""
    d, Q, H = runs["d"], runs["Q"], runs["H"]
    Xa, ra, la = runs["plain"]
    assert ra == d + 2 and [lv["r"] for lv in la] == [d, d + 1, d + 2]
    assert all(set(lv) == {"r", "steps", "f", "gradnorm", "lambda_min", "alpha", "trials"} for lv in la)
    assert Xa.shape == ((d + 2) * Q.shape[0],) and la[-1]["lambda_min"] >= -1e-6 and la[-1]["f"] <= 1e-8
    assert RG.cost(Q, H.from_dev_layout(Xa, d + 2)) <= 1e-8


def test_staircase_comes_back_down_to_rank_d(runs):
    d, Q, H = runs["d"], runs["Q"], runs["H"]
    Xp, rp, lp = runs["plain"]
    Xr, rr, lr = runs["reduced"]
    print(lr)
    assert rr == d and Xr.shape == (d * Q.shape[0],)
    # the way up is the same: ranks, steps and alpha
    assert len(lr) == len(lp) + 1
    for a, b in zip(lr, lp):
        assert (a["r"], a["steps"], a["alpha"], a["trials"]) == (b["r"], b["steps"], b["alpha"], b["trials"])
    last = lr[-1]
    assert last["r"] == d and last["reduced_from"] == d + 2 and last["certified"] is True
    assert last["lambda_min"] >= -1e-6
    assert abs(last["f"]) <= 1e-12
    assert last["w"].shape == (d + 2,) and np.all(last["w"][d:] <= 1e-6 * last["w"][0])
    assert abs(last["dropped"]) <= 1e-6 * last["w"][0]
    Xm = H.from_dev_layout(Xr, d)
    assert abs(RG.cost(Q, Xm)) <= 1e-12
    assert RG.min_eig(Q, Xm, d)[0] >= -1e-6
    P = O.to_poses(Xm, d, d)[:, :, :d]
    assert np.abs(np.swapaxes(P, 1, 2) @ P - np.eye(d)).max() <= 1e-13  # O(d) per pose: the manifold at r = d
