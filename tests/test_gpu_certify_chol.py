"""GPU tests of the certificate by factorisation (dpgo_hip_certify_chol*, dpgo_graph_certify_chol).
Build-defined, absent from the reference: pinned against dense Cholesky and eigenvalues of the oracle's explicit
certificate matrix (tests/_cholcert.py; tests/test_certify_chol_reference.py shows each decision has margin).

Bars of the eigenpair are tests/test_gpu_certify.py's: |v| = 1 to 1e-8, |v S - lambda v| <= 1e-6 |lambda|_max and
|lambda - lambda_dense| <= 1e-6 |lambda|_max, residual against the dense S."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _cholcert as CC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ids = lambda k: "-".join(map(str, k))  # noqa: E731


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


def _raw_ex(hip, P, X, eta, lam, vec, info, params=None):
    """dpgo_hip_certify_chol_ex on the caller's own output buffers: the return code."""
    x = hip.to_dev_layout(X)
    return hip.lib().dpgo_hip_certify_chol_ex(P.h, x.ctypes.data_as(C.POINTER(C.c_double)), float(eta), params,
                                              C.byref(lam), vec.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info))


@pytest.mark.parametrize("tiled", [False, True], ids=["levels", "tiled"])
@pytest.mark.parametrize("key", CC.DECISION_CASES, ids=_ids)
def test_decisions(hip, key, tiled, monkeypatch):
    """pd of the device factorisation of S(X) + sigma I = the dense reference's, on each side of -lambda_min: the three
    random points, both golden optima, and every compiled (d, r).  tiled: DPGO_FAC_TILED_MIN_TILES=1 sends every tree
    level through the tile-parallel k_snf_* kernels; the decisions must be the same."""
    if tiled:
        monkeypatch.setenv("DPGO_FAC_TILED_MIN_TILES", "1")
    c = CC.case(key)
    P = _problem(hip, c)
    for sigma, pd in CC.sigmas(key):
        assert CC.reference_pd(c.S, sigma) is pd
        assert P.certify_chol(c.X, sigma) is pd, (key, sigma, c.lam)
    # the other order on the same handle: a refactorisation after a failed one starts clean
    for sigma, pd in reversed(CC.sigmas(key)):
        assert P.certify_chol(c.X, sigma) is pd, (key, sigma, c.lam)


def test_weighted_graph_decisions(hip):
    """Graph.certify_chol(w=...) certifies the weighted problem: loop-closure weights from {0, 0.3, 1}, the reference S
    from the weighted Laplacian, eta at +-25 % of -lambda_min."""
    from oracle import dpgo_oracle as O
    c = CC.case(CC.WEIGHTED)
    u = CC.case(("rand", "smallGrid3D", 5))
    m = c.meas
    g = hip.Graph.from_arrays(c.d, c.n, m.p1, m.p2, m.R, m.t, m.kappa, m.tau)
    assert g.m == len(m.p1)  # w below is in the graph's edge order
    assert abs(c.lam - u.lam) > 1e-6 * c.lam_max  # the weights move lambda_min: the unweighted S is another matrix
    Qw = O.connection_laplacian(m, c.n)
    f_w = 0.5 * float(np.sum(np.asarray((Qw @ c.X.T).T) * c.X))
    for eta, pd in CC.sigmas(CC.WEIGHTED):
        assert CC.reference_pd(c.S, eta) is pd
        out = g.certify_chol(c.X, c.r, eta, w=m.weight)
        assert out["pd"] is pd and out["certified"] == int(pd), (eta, out)
        assert abs(out["f_relax"] - f_w) <= 1e-11 * abs(f_w)  # f of the weighted problem, as Graph.certify's bar
        if pd:
            assert out["lambda_min"] == -eta and out["factorisations"] == 1 and "eigvec" not in out
        else:
            assert -out["sigma_hi"] < c.lam <= -out["sigma_lo"], (out, c.lam)
            assert abs(out["lambda_min"] - c.lam) <= 1e-6 * c.lam_max


@pytest.mark.parametrize("key", CC.BRACKET_CASES, ids=_ids)
def test_bracket_and_vector(hip, key):
    """The uncertified path: the bracket holds lambda_dense and is as narrow as asked, the vector is an eigenvector
    of the dense S on row 0 of the lifted layout."""
    c = CC.case(key)
    eta = [s for s, pd in CC.sigmas(key) if not pd][0]
    P = _problem(hip, c)
    out = P.certify_chol_ex(c.X, eta)
    print(key, {k: v for k, v in out.items() if k != "eigvec"}, "lambda_dense", c.lam)
    ratio = hip.chol_cert_params().ratio
    assert ratio == 1.0 + 1.0 / 16.0
    assert out["certified"] == 0 and out["sigma_lo"] >= eta
    assert -out["sigma_hi"] < c.lam <= -out["sigma_lo"]
    assert out["sigma_hi"] / out["sigma_lo"] <= ratio
    assert 3 <= out["factorisations"] <= 25 and 1 <= out["invit_iters"] <= 200
    assert out["factor_ms"] > 0.0 and out["panel_doubles"] > 0
    v = out["eigvec"]
    assert v.shape == (c.r, (c.d + 1) * c.n)
    assert float(np.abs(v[1:]).max()) == 0.0
    assert abs(np.linalg.norm(v) - 1.0) <= 1e-8
    lam = out["lambda_min"]
    res = float(np.linalg.norm(v[0] @ c.S - lam * v[0]))
    assert res <= 1e-6 * c.lam_max, (res, out["residual"])
    assert abs(res - out["residual"]) <= 1e-3 * res + 1e-9 * c.lam_max
    assert abs(lam - c.lam) <= 1e-6 * c.lam_max
    # the escape takes the matrix as it is: row 0, renormalised (|v| = 1 to 1e-8 above)
    assert np.abs(hip.escape_direction(v, c.d) - v[0]).max() <= 1e-8


def test_bracket_parameters(hip):
    """A narrower ratio costs more factorisations and still brackets; max_factorisations ends the bisection early
    with a valid (wider) bracket."""
    key = ("rand", "tinyGrid3D", 3)
    c = CC.case(key)
    eta = [s for s, pd in CC.sigmas(key) if not pd][0]
    P = _problem(hip, c)
    base = P.certify_chol_ex(c.X, eta)
    fine = P.certify_chol_ex(c.X, eta, ratio=1.0 + 1.0 / 256.0)
    assert fine["sigma_hi"] / fine["sigma_lo"] <= 1.0 + 1.0 / 256.0
    assert -fine["sigma_hi"] < c.lam <= -fine["sigma_lo"]
    assert fine["factorisations"] > base["factorisations"]
    few = P.certify_chol_ex(c.X, eta, max_factorisations=3)
    assert few["factorisations"] <= 4  # one more when the last trial failed: the factor at sigma_hi again
    assert -few["sigma_hi"] < c.lam <= -few["sigma_lo"]
    assert abs(few["lambda_min"] - c.lam) <= 1e-6 * c.lam_max


def test_certified_branch(hip):
    """At smallGrid3D's optimum with eta = 1e-6 |lambda|_max: certified by one factorisation, lambda_min = -eta (the
    bound), and the caller's eigvec buffer is not written."""
    c = CC.case(CC.OPT_SMALL)
    eta = 1e-6 * c.lam_max
    P = _problem(hip, c)
    lam, info = C.c_double(7.0), hip.CholCertInfo()
    vec = np.full(P.vec_len, 123.25)
    assert _raw_ex(hip, P, c.X, eta, lam, vec, info) == 0
    assert info.certified == 1 and info.factorisations == 1
    assert lam.value == -eta and info.sigma_lo == eta and info.sigma_hi == eta and info.invit_iters == 0
    assert np.all(vec == 123.25)
    out = P.certify_chol_ex(c.X, eta)
    assert out["certified"] == 1 and "eigvec" not in out


def test_isolated_from_the_exact_preconditioner(hip):
    """A handle that preconditions with PRECON_EXACT: a certificate through the bracket path in between leaves the
    preconditioner's output bitwise what it was, and its factor count and fallback flags unchanged."""
    from tests._common import random_tangent
    key = ("rand", "smallGrid3D", 5)
    c = CC.case(key)
    P = _problem(hip, c)
    P.set_precon(hip.PRECON_EXACT)
    V = random_tangent(c.X, c.d, 9)
    before = P.precondition(c.X, V)
    info0, fb0 = P.exact_factor_info(), P.exact_fallback_agents()
    assert info0["factor_count"] >= 1 and np.isfinite(before).all()
    out = P.certify_chol_ex(c.X, [s for s, pd in CC.sigmas(key) if not pd][0])
    assert out["certified"] == 0 and out["factorisations"] >= 3
    info1, fb1 = P.exact_factor_info(), P.exact_fallback_agents()
    assert info1["factor_count"] == info0["factor_count"] and np.array_equal(fb0, fb1)
    assert info1["panel_doubles"] == info0["panel_doubles"] and info1["factor_ms"] == info0["factor_ms"]
    after = P.precondition(c.X, V)
    assert np.array_equal(before, after)
    assert P.exact_factor_info()["factor_count"] == info0["factor_count"]
    # and the other way round: a handle certified first preconditions as one that never was
    P2 = _problem(hip, c)
    assert P2.certify_chol(c.X, -1.25 * c.lam) is True
    P2.set_precon(hip.PRECON_EXACT)
    assert np.array_equal(P2.precondition(c.X, V), before)


def test_refusals(hip):
    """EINVAL for a batched handle, a BSR handle and a non-finite sigma; no output is written on an error."""
    from oracle import dpgo_oracle as O
    c = CC.case(("rand", "tinyGrid3D", 3))
    lib = hip.lib()
    dp = C.POINTER(C.c_double)
    edges = _problem(hip, c)
    bsr = hip.Problem(c.n, c.d, c.r)
    bsr.set_Q_scipy(0, O.connection_laplacian(c.meas, c.n))
    batched = hip.Problem(None, 3, 3, poses_per_agent=[4, 4])
    x = hip.to_dev_layout(c.X)
    for P, sigma in [(batched, 1.0), (bsr, 1.0), (edges, float("nan")), (edges, float("inf"))]:
        xs = x if P is not batched else np.zeros(P.vec_len)
        pd = C.c_int(-7)
        assert lib.dpgo_hip_certify_chol(P.h, xs.ctypes.data_as(dp), sigma, C.byref(pd)) == -1  # DPGO_HIP_EINVAL
        assert pd.value == -7
        lam, info = C.c_double(7.0), hip.CholCertInfo()
        info.factorisations = -7
        vec = np.full(P.vec_len, 123.25)
        assert lib.dpgo_hip_certify_chol_ex(P.h, xs.ctypes.data_as(dp), sigma, None, C.byref(lam),
                                            vec.ctypes.data_as(dp), C.byref(info)) == -1
        assert lam.value == 7.0 and info.factorisations == -7 and np.all(vec == 123.25)
    with pytest.raises(hip.DPGOHipError, match="edge-stream"):
        bsr.certify_chol(c.X, 1.0)
    with pytest.raises(hip.DPGOHipError, match="single-agent"):
        batched.certify_chol(np.zeros((3, 32)), 1.0)
    assert edges.certify_chol(c.X, -1.25 * c.lam) is True  # the handle still works after the refusals


def test_decisions_with_poisoned_allocations():
    """test_decisions in a child process with DPGO_POISON=1 (every fresh allocation, and the frontal matrices and
    panels before each factorisation, NaN): a pivot computed from an entry nothing wrote would fail d > 0 and flip a
    positive-definite decision, so the same decisions prove the factorisation reads written memory only."""
    env = dict(os.environ, DPGO_POISON="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "gpu",
                          os.path.join(ROOT, "tests", "test_gpu_certify_chol.py"), "-k", "test_decisions and not poisoned"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert f"{2 * len(CC.DECISION_CASES)} passed" in out.stdout, out.stdout[-500:]
