"""The per-pose dense kernels on ill-conditioned and boundary inputs, against the np.longdouble references of
tests/_dense.py (bars and their derivation there; tests/test_dense_reference.py checks the references, the branches the
batches reach and that the float64 oracle passes the same bars on the CPU):

  1. polar_fast / polar_inplace (k_polar_comb) at prescribed singular values: on the manifold, a hair below and above
     the Newton-Schulz switch, small and clustered singular values, and 2^+-100 scaling;
  2. dpgo_hip_polar_combine_dev with per-agent coefficients, both forms, every agent compared on its own;
  3. qf_inplace (k_retract, k_lift_escape) with steps up to 1e8 times the point, which lose a direction;
  4. the tangent projection where almost all of V is removed;
  5. gauss_jordan (k_bj_inverse, k_bj_inverse_diag) at kappa, tau over eight decades, through k_precond;
  6. a NaN in one pose leaves every other pose bitwise alone.

Every batch has 130 poses (tiles of 64, 64 and 2).  Measured on an MI355X: at most 0.066 of the polar bar (just above
the switch), 0.046 in polar_combine_dev, 0.042 of the QF bar, 0.28 of the tangent bar and 0.097 of the block-Jacobi bar;
each case prints its worst pose and the fraction of the bar it reaches."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _dense as D

pytestmark = pytest.mark.gpu

LD = D.LD


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1, "no gfx950 device"
    return H


def _rot(X, d):
    return D.to_poses(X, d)[:, :, :d]


def _check_bar(what, got, ref, bar, d):
    """max |got - ref| per pose against bar (per pose), the worst pose named."""
    err = D.pose_max(got, ref, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.inf)
    j = int(np.argmax(ratio))
    print(f"{what}: worst pose {j} (tile {j // 64}) at {ratio[j]:.3g} of its bar {bar[j]:.3g}")
    assert np.isfinite(np.asarray(got)).all(), what
    assert ratio[j] <= 1.0, f"{what}: pose {j}: |got - ref| = {err[j]:.3e} over the bar {bar[j]:.3e}"


def _check_ortho(what, got, d):
    defect = D.ortho_defect(got, d)
    assert defect.max() <= D.ORTHO_BAR, f"{what}: |Q^T Q - I| = {defect.max():.3e} at pose {int(np.argmax(defect))}"


def _dev_call(H, P, fn, *mats):
    """fn(P, *device pointers of the matrices in device layout, out pointer) on torch buffers -> out (r x (d+1) n)."""
    import torch
    bufs = [torch.from_numpy(H.to_dev_layout(M)).cuda() if M is not None else None for M in mats]
    out = torch.full_like(bufs[0], float("nan"))
    torch.cuda.synchronize()
    fn(P, *[b.data_ptr() if b is not None else None for b in bufs], out.data_ptr())
    P.synchronize()
    return H.from_dev_layout(out.cpu().numpy(), P.r)


# ---------------------------------------------------------------------------------------------------------- 1. polar
@pytest.mark.parametrize("d,r", D.SHAPES)
def test_polar_prescribed_singular_values(hip, d, r):
    """hip.project_polar on every batch: within K_POLAR eps kappa_polar of polar_ref per pose, orthonormal to 1e-14
    whatever the conditioning, translations bitwise; on the core shapes dpgo_hip_project_polar_dev on torch buffers
    gives bitwise the same."""
    P = hip.Problem(D.N, d, r) if (d, r) in D.CORE else None
    for name in D.POLAR_BATCHES:
        M, sig, branch = D.polar_batch(d, r, name)
        got = hip.project_polar(M, d)
        bar = np.full(D.N, D.K_POLAR * D.EPS * D.kappa_polar(sig, r, d))
        _check_bar(f"polar d={d} r={r} {name} ({branch})", got, D.polar_reference(M, d), bar, d)
        _check_ortho(name, got, d)
        assert np.array_equal(got[:, d::d + 1], M[:, d::d + 1]), name
        if P is not None:
            dev = _dev_call(hip, P, lambda p, a, o: p.project_polar_dev(a, o), M)
            assert np.array_equal(dev, got), name


# -------------------------------------------------------------------------------------------------------- 2. combine
@pytest.mark.parametrize("two_operands", [True, False])
@pytest.mark.parametrize("d,r", D.CORE)
def test_polar_combine_per_agent(hip, d, r, two_operands):
    """project(ca[k] A + cb[k] B) and project(ca[k] A) with distinct coefficients per agent: the reference is polar_ref
    of the combination rounded as comb_xv rounds it, every agent is compared on its own, and the translation column
    is bitwise that combination."""
    A, B = D.combine_batch(d, r)
    if not two_operands:
        B = None
    P = hip.Problem(0, d, r, poses_per_agent=list(D.COMBINE_AGENTS))
    got = _dev_call(hip, P, lambda p, a, b, o: p.polar_combine_dev(a, b, list(D.COMBINE_CA), list(D.COMBINE_CB), o),
                    A, B)
    M = D.combine_exact(A, B, d)
    ref = D.polar_reference(M, d)
    bar = D.K_POLAR * D.EPS * D.kappa_polar_of(M, d)
    err = D.pose_max(got, ref, d)
    assert np.isfinite(got).all()
    b = d + 1
    for k in range(P.K):
        lo, hi = int(P.offsets[k]), int(P.offsets[k + 1])
        ratio = err[lo:hi] / bar[lo:hi]
        print(f"combine d={d} r={r} B={two_operands} agent {k}: worst {ratio.max():.3g} of its bar")
        assert ratio.max() <= 1.0, f"agent {k}: pose {lo + int(np.argmax(ratio))}: {err[lo:hi].max():.3e}"
        assert np.array_equal(got[:, lo * b + d:hi * b:b], M[:, lo * b + d:hi * b:b]), f"agent {k}: translations"
    _check_ortho("combine", got, d)


# ------------------------------------------------------------------------------------------------------------- 3. QF
@pytest.mark.parametrize("d,r", D.SHAPES)
def test_retraction_with_large_steps(hip, d, r):
    """hip.retract_qf(X, V, scale) with |V| = 1 per pose and scale up to 1e8 (X + s V loses a direction, in part only
    on the odd poses): within K_QF eps cond(X_Y + s V_Y) of qf_ref, diag(Q^T M) > 0, orthonormal to 1e-14."""
    X, V = D.qf_batch(d, r)
    for s in D.QF_SCALES:
        ref, cond, MY = D.qf_reference(X, V, s, d)
        got = hip.retract_qf(X, V, d, scale=s)
        _check_bar(f"retract d={d} r={r} s={s:g} (cond <= {cond.max():.3g})", got, ref, D.K_QF * D.EPS * cond, d)
        _check_ortho(f"retract s={s:g}", got, d)
        assert (np.einsum("jac,jac->jc", _rot(got, d).astype(LD), MY) > 0).all(), s
        assert np.array_equal(got[:, d::d + 1], X[:, d::d + 1]), s  # V has no translation part


@pytest.mark.parametrize("d,r", [(d, r) for d, r in D.SHAPES if (d, r + 1) in D.SHAPES])
def test_lift_escape_with_large_steps(hip, d, r):
    """hip.lift_escape on the same points: the rank r + 1 QF of [Y_j; alpha v_Y^T] with |v_Y| = 1 and alpha up to 1e4."""
    X, v = D.lift_batch(d, r)
    for alpha in D.LIFT_ALPHAS:
        ref, cond, MY = D.lift_reference(X, v, alpha, d)
        got = hip.lift_escape(X, d, v, alpha)
        _check_bar(f"lift d={d} r={r} alpha={alpha:g} (cond <= {cond.max():.3g})", got, ref, D.K_QF * D.EPS * cond, d)
        _check_ortho(f"lift alpha={alpha:g}", got, d)
        assert (np.einsum("jac,jac->jc", _rot(got, d).astype(LD), MY) > 0).all(), alpha
        assert np.array_equal(got[:, d::d + 1], ref[:, d::d + 1].astype(np.float64)), alpha


# -------------------------------------------------------------------------------------------------------- 4. tangent
@pytest.mark.parametrize("d,r", D.CORE)
def test_tangent_projection_removes_almost_everything(hip, d, r):
    """V = 1e8 X + t with t a unit tangent: 4 eps max|V_Y| per pose, absolute, against the longdouble statement."""
    X, V = D.tangent_batch(d, r)
    got = hip.tangent_project(X, V, d)
    bar = D.TANGENT_K * D.EPS * np.abs(_rot(V, d)).max(axis=(1, 2))
    _check_bar(f"tangent d={d} r={r}", got, D.tangent_ref(X, V, d), bar, d)
    assert np.array_equal(got[:, d::d + 1], V[:, d::d + 1])


# --------------------------------------------------------------------------------------------------- 5. block-Jacobi
@pytest.mark.parametrize("d", [2, 3])
def test_block_jacobi_over_eight_decades(hip, d):
    """k_bj_inverse (Q as BSR) and k_edge_diag + k_bj_inverse_diag (Q as the edge stream) through k_precond, against
    P_X(V bj_inverse_ref) in longdouble: K_BJ eps cond(block_j) |V_j| |Minv_j| per pose, and the same bar between the
    two formats.  One pose has no edge (block 0.1 I), one is a second endpoint only (a diagonal block)."""
    r = d + 2
    X, V, ref, unit = D.bj_reference(d, r)
    meas = D.bj_measurements(d)
    out = {}
    for fmt in ("bsr", "edges"):
        H = hip.Problem(D.N, d, r)
        if fmt == "bsr":
            H.set_Q_scipy(0, O.connection_laplacian(meas, D.N))
        else:
            H.set_Q_edges(0, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau, meas.weight)
        H.set_precon(O.PRECON_BLOCK_JACOBI)
        out[fmt] = H.precondition(X, V)
        _check_bar(f"block-Jacobi d={d} {fmt}", out[fmt], ref, D.K_BJ * unit, d)
    _check_bar(f"block-Jacobi d={d} bsr against edges", out["bsr"], out["edges"], D.K_BJ * unit, d)


# ------------------------------------------------------------------------------------------------------------ 6. NaN
def _with_nan(M, d):
    """M with a NaN in the first rotation entry of the poses NAN_POSES."""
    Mn = np.array(M)
    for j in D.NAN_POSES:
        Mn[0, j * (d + 1)] = np.nan
    return Mn


def _others_bitwise(what, clean, dirty, d):
    keep = np.ones(D.N, bool)
    keep[list(D.NAN_POSES)] = False
    assert np.isfinite(clean).all(), what
    assert np.array_equal(D.to_poses(clean, d)[keep], D.to_poses(dirty, d)[keep]), what


@pytest.mark.parametrize("d,r", D.CORE)
def test_a_nan_does_not_travel(hip, d, r):
    """A NaN in one pose of a full tile and in one pose of the short tile: the run returns, and every other pose of
    project_polar (Newton-Schulz and Jacobi neighbours), retract_qf and tangent_project is bitwise the clean run's."""
    for name in ("manifold", "graded"):
        M = D.polar_batch(d, r, name)[0]
        _others_bitwise(f"polar {name}", hip.project_polar(M, d), hip.project_polar(_with_nan(M, d), d), d)
    X, V = D.qf_batch(d, r)
    clean = hip.retract_qf(X, V, d, scale=1.0)
    _others_bitwise("retract, NaN in V", clean, hip.retract_qf(X, _with_nan(V, d), d, scale=1.0), d)
    _others_bitwise("retract, NaN in X", clean, hip.retract_qf(_with_nan(X, d), V, d, scale=1.0), d)
    X, V = D.tangent_batch(d, r)
    clean = hip.tangent_project(X, V, d)
    _others_bitwise("tangent, NaN in V", clean, hip.tangent_project(X, _with_nan(V, d), d), d)
    _others_bitwise("tangent, NaN in X", clean, hip.tangent_project(_with_nan(X, d), V, d), d)
