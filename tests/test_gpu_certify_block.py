"""GPU tests of the block certificate (dpgo_hip_certify_block, dpgo_graph_certify_block): LOBPCG on the
r rows of the lifted layout.  Build-defined, absent from the reference: pinned against the eigenvalues of the
oracle's explicit certificate matrix (tests/_cholcert.py) and, for the iteration counts, against the numpy model
tests/_lobpcg.py (tests/test_lobpcg_reference.py shows that model converges to the dense values).

The shapes are the smallest at which the kernels can go wrong: tinyGrid3D (36 columns, less than one 64-column
chunk of the Gram kernel; at r = 8 three blocks take 24 of the 27 free dimensions), the 60-pose INTEL prefix (d = 2),
smallGrid3D (500 columns, 8 chunks) and INTEL (3,684 columns: 58 chunks with a ragged tail, more than one workgroup
of the per-column kernels).

Bars of the eigenpair are tests/test_gpu_certify.py's: |v| = 1 to 1e-8, rows 1.. exactly zero,
|v S - lambda v| <= 1e-6 |lambda|_max and |lambda - lambda_dense| <= 1e-6 |lambda|_max against the dense S, the
reported residual within 1e-3 relative + 1e-9 |lambda|_max of the recomputed one.  With the locked block U: the
bars of its test_certificate_thick_restart.  Operator passes: at most 2 x the model's + 10 (the factor covers the
different summation order, not a different algorithm; the device also reads an iterate's stopping test together
with the next iteration's Gram matrices, one pass later than the model)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _cholcert as CC
from tests import _lobpcg as LB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ids = lambda k: "-".join(map(str, k))  # noqa: E731
INFO_FIELDS = ("iters", "restarts", "seeds", "residual", "lambda_seed", "lambda_complement", "residual_complement",
               "coupling", "lower_bound", "ritz")


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1, "no gfx950 device"
    return H


def _problem(hip, c):
    m = c.meas
    P = hip.Problem(c.n, c.d, c.r)
    P.set_Q_edges(0, m.p1, m.p2, m.R, m.t, m.kappa, m.tau, m.weight)
    return P


def _check(hip, key, out, seed_x, precon=False):
    """Every bar of the module docstring on one result of case `key`."""
    c = CC.case(key)
    ref = LB.model(key, seed_x, precon=precon)
    print(key, "seed_x", seed_x, "precon", precon, {k: v for k, v in out.items() if k != "eigvec"},
          "model passes", ref["iters"], "lambda_dense", c.lam)
    v, lam = out["eigvec"], out["lambda_min"]
    assert v.shape == (c.r, (c.d + 1) * c.n)
    assert float(np.abs(v[1:]).max()) == 0.0
    assert abs(np.linalg.norm(v) - 1.0) <= 1e-8
    res = float(np.linalg.norm(v[0] @ c.S - lam * v[0]))
    assert abs(res - out["residual"]) <= 1e-3 * res + 1e-9 * c.lam_max, (res, out["residual"])
    assert out["iters"] <= 2 * ref["iters"] + 10, (out["iters"], ref["iters"])
    assert out["lower_bound"] <= c.lam + 1e-9 * c.lam_max <= lam + 2e-9 * c.lam_max, (out, c.lam)
    if not seed_x:
        assert out["seeds"] == 0 and np.isnan(out["lambda_seed"]) and out["coupling"] == 0.0
        assert abs(lam - c.lam) <= 1e-6 * c.lam_max, (lam, c.lam)
        assert res <= 1e-6 * c.lam_max
        assert out["lambda_complement"] == lam and out["residual_complement"] == out["residual"]
        return
    blocks = LB.complement(key)
    assert out["seeds"] == blocks["seeds"]
    assert abs(out["lambda_seed"] - blocks["lambda_seed"]) <= 1e-9 * c.lam_max, (out, blocks)
    assert abs(out["lambda_complement"] - blocks["lambda_complement"]) <= 1e-6 * c.lam_max, (out, blocks)
    assert out["residual_complement"] <= 1e-6 * c.lam_max
    assert abs(out["coupling"] - blocks["coupling"]) <= 1e-9 * c.lam_max + 1e-6 * blocks["coupling"], (out, blocks)
    assert lam == min(out["lambda_seed"], out["lambda_complement"])


@pytest.mark.parametrize("fmt", ["bsr", "edges"])
@pytest.mark.parametrize("key", CC.MAIN_RANDOM, ids=_ids)
def test_eigenpair_at_random_points(hip, key, fmt):
    """No locked block: the lowest eigenpair of the dense S, from either Q format."""
    from oracle import dpgo_oracle as O
    c = CC.case(key)
    if fmt == "edges":
        P = _problem(hip, c)
    else:
        P = hip.Problem(c.n, c.d, c.r)
        P.set_Q_scipy(0, O.connection_laplacian(c.meas, c.n))
    out = P.certify_block(c.X, flags=0)
    _check(hip, key, out, False)
    assert out["lambda_min"] < 0


@pytest.mark.parametrize("key", CC.MAIN_RANDOM, ids=_ids)
def test_locked_block_at_random_points(hip, key):
    """The default flags (DPGO_CERT_SEED_X) at a random point, where U's block and the coupling are far from zero."""
    c = CC.case(key)
    _check(hip, key, _problem(hip, c).certify_block(c.X), True)


def test_optimum_certifies(hip):
    """smallGrid3D's RTR optimum: U carries the near-null cluster, the complement starts at 1.96 and the bound
    certifies at eta = 1e-6 |lambda|_max (the golden iterate's coupling is 2.7e-3: the bound is -coupling^2 / 1.96)."""
    c = CC.case(CC.OPT_SMALL)
    out = _problem(hip, c).certify_block(c.X)
    _check(hip, CC.OPT_SMALL, out, True)
    assert out["lower_bound"] >= -1e-6 * c.lam_max
    assert out["lambda_complement"] > 1.0


def test_critical_point_does_not_certify(hip):
    """tinyGrid3D's rank-3 critical point (lambda_min = -1.10e-3): the bound fails at eta = 1e-6 |lambda|_max, the
    value is the dense one and the vector is an escape direction as it stands.  The negative pair is U's own here
    (lambda_seed < theta_C = 3.34), so the vector's residual is the coupling's size (4.8e-3 at this iterate, whose
    coupling is 9.2e-3); _check holds the reported residual to the recomputed one."""
    c = CC.case(CC.OPT_TINY)
    out = _problem(hip, c).certify_block(c.X)
    _check(hip, CC.OPT_TINY, out, True)
    assert out["lower_bound"] < -1e-6 * c.lam_max
    assert abs(out["lambda_min"] - c.lam) <= 1e-6 * c.lam_max and out["lambda_min"] < -1e-3
    assert out["lambda_min"] == out["lambda_seed"]
    v = out["eigvec"]
    assert np.abs(hip.escape_direction(v, c.d) - v[0]).max() <= 1e-8


@pytest.mark.parametrize("seed_x", [False, True], ids=["plain", "seed_x"])
@pytest.mark.parametrize("key", CC.EVERY_RANK, ids=_ids)
def test_every_compiled_rank(hip, key, seed_x):
    """Every compiled (d, r): d = 3 with r = 3..8 on tinyGrid3D, d = 2 with r = 2..8 on the 60-pose INTEL prefix."""
    c = CC.case(key)
    out = _problem(hip, c).certify_block(c.X, flags=1 if seed_x else 0)
    _check(hip, key, out, seed_x)


def test_weights(hip):
    """Graph.certify_block(w=...) certifies the weighted problem: loop-closure weights from {0, 0.3, 1}, the
    reference S from the weighted Laplacian; the unit-weight matrix has another lambda_min."""
    from oracle import dpgo_oracle as O
    c = CC.case(CC.WEIGHTED)
    u = CC.case(("rand", "smallGrid3D", 5))
    m = c.meas
    g = hip.Graph.from_arrays(c.d, c.n, m.p1, m.p2, m.R, m.t, m.kappa, m.tau)
    assert g.m == len(m.p1)  # w below is in the graph's edge order
    out = g.certify_block(c.X, c.r, w=m.weight)  # the default flags: U's blocks of the weighted S
    _check(hip, CC.WEIGHTED, out, True)
    Qw = O.connection_laplacian(m, c.n)
    f_w = 0.5 * float(np.sum(np.asarray((Qw @ c.X.T).T) * c.X))
    assert abs(out["f_relax"] - f_w) <= 1e-11 * abs(f_w)
    plain = g.certify_block(c.X, c.r, w=m.weight, flags=0)  # no U: lambda_min of the weighted S itself
    _check(hip, CC.WEIGHTED, plain, False)
    assert abs(plain["f_relax"] - f_w) <= 1e-11 * abs(f_w)
    assert abs(plain["lambda_min"] - u.lam) > 1e-6 * c.lam_max
    unit = g.certify_block(c.X, c.r, flags=0)
    assert abs(unit["lambda_min"] - u.lam) <= 1e-6 * u.lam_max


@pytest.mark.parametrize("key", [CC.OPT_SMALL, CC.OPT_TINY], ids=_ids)
def test_preconditioned(hip, key):
    """precon = 1 (the handle's block-Jacobi inverse of Q + 0.1 I) at both optima: the same bars, the passes against
    the model run with the same option."""
    c = CC.case(key)
    out = _problem(hip, c).certify_block(c.X, precon=1)
    _check(hip, key, out, True, precon=True)


def test_deterministic(hip):
    """Two calls on one handle and one on a fresh handle: lambda, every info field and the vector bitwise equal
    (fixed-grid partials, fixed-order sums, no atomics)."""
    for key in [("rand", "input_INTEL_g2o", 3), CC.OPT_SMALL]:
        c = CC.case(key)
        P = _problem(hip, c)
        a, b2 = P.certify_block(c.X), P.certify_block(c.X)
        f = _problem(hip, c).certify_block(c.X)
        for o in (b2, f):
            assert o["lambda_min"] == a["lambda_min"]
            for k in INFO_FIELDS:
                assert np.array_equal(np.asarray(o[k]), np.asarray(a[k]), equal_nan=True), k
            assert np.array_equal(o["eigvec"], a["eigvec"])


def test_refusals(hip):
    """DPGO_HIP_EINVAL with lambda, eigvec and info untouched: a batched handle, three blocks beyond the free
    dimension, max_iters < 1, a non-finite tol, an unknown precon or flag."""
    lib, dp = hip.lib(), C.POINTER(C.c_double)
    c = CC.case(("rand", "tinyGrid3D", 3))
    good = _problem(hip, c)
    batched = hip.Problem(None, 3, 3, poses_per_agent=[4, 4])
    meas = CC.prefix(c.meas, 4)  # 16 columns; r = 5: U has 6 rows, 3 r = 15 > 16 - 6
    small = hip.Problem(4, 3, 5)
    small.set_Q_edges(0, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau, meas.weight)
    from tests._common import random_point
    xs_small = hip.to_dev_layout(random_point(5, 3, 4, 5))
    x = hip.to_dev_layout(c.X)
    cases = [(batched, np.zeros(batched.vec_len), {}), (small, xs_small, {}),
             (good, x, dict(max_iters=0)), (good, x, dict(tol=float("nan"))), (good, x, dict(tol=float("inf"))),
             (good, x, dict(precon=2)), (good, x, dict(flags=2)), (good, x, dict(refresh=-1))]
    for P, xs, kw in cases:
        lam, info = C.c_double(7.0), hip.CertInfo()
        info.iters, info.residual = -7, 123.25
        vec = np.full(P.vec_len, 123.25)
        rc = lib.dpgo_hip_certify_block(P.h, xs.ctypes.data_as(dp), C.byref(hip.block_cert_params(**kw)),
                                        C.byref(lam), vec.ctypes.data_as(dp), C.byref(info))
        assert rc == -1, (kw, rc)  # DPGO_HIP_EINVAL
        assert lam.value == 7.0 and info.iters == -7 and info.residual == 123.25 and np.all(vec == 123.25)
    with pytest.raises(hip.DPGOHipError, match="single-agent"):
        batched.certify_block(np.zeros((3, 32)))
    with pytest.raises(hip.DPGOHipError, match="free dimension"):
        small.certify_block(random_point(5, 3, 4, 5))
    with pytest.raises(TypeError):
        hip.block_cert_params(basis=3)
    p = hip.block_cert_params()
    assert (p.max_iters, p.tol, p.flags, p.precon, p.refresh) == (2000, 1e-8, 1, 0, 50)
    _check(hip, ("rand", "tinyGrid3D", 3), good.certify_block(c.X), True)  # the handle still works


def test_with_poisoned_allocations():
    """This file in a child process with DPGO_POISON=1 (every fresh device allocation NaN): a kernel that read an
    entry nothing wrote would turn a Gram matrix into NaN, which the driver refuses."""
    env = dict(os.environ, DPGO_POISON="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "gpu",
                          os.path.join(ROOT, "tests", "test_gpu_certify_block.py"), "-k",
                          "test_optimum_certifies or test_critical_point or test_preconditioned"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "4 passed" in out.stdout, out.stdout[-500:]
