"""CPU checks of the ground tests/test_gpu_dense_edges.py stands on (tests/_dense.py): the longdouble references are
what they claim to be (orthonormal, the polar factor's symmetric product, equal to mpmath at 50 digits), every polar
batch reaches the branch of polar_fast it is built for, and the float64 oracle passes every bar, so the bars are
passable by a correct float64 implementation."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _dense as D

LD = D.LD


@pytest.mark.parametrize("d,r", D.SHAPES)
def test_polar_reference_is_the_polar_factor(d, r):
    """P^T P = I to 1e-17 and P^T M symmetric to 1e-17 sigma_max (positive definite: the d x d Newton iteration starts
    from Q^T M with positive diagonal and keeps the sign of the determinant; mpmath confirms below)."""
    for name in D.POLAR_BATCHES:
        M, sig, _ = D.polar_batch(d, r, name)
        ref = D.polar_reference(M, d)
        assert D.ortho_defect(ref, d).max() <= 1e-17, name
        P, MY = D.to_poses(ref, d)[:, :, :d], D.to_poses(np.asarray(M, LD), d)[:, :, :d]
        S = np.swapaxes(P, 1, 2) @ MY
        smax = np.abs(MY).max(axis=(1, 2))  # within sqrt(r d) of sigma_max, from below
        assert (np.abs(S - np.swapaxes(S, 1, 2)).max(axis=(1, 2)) <= LD(1e-17) * smax).all(), name
        assert np.array_equal(ref[:, d::d + 1].astype(np.float64), M[:, d::d + 1])  # translations kept
        assert len(sig) == d


@pytest.mark.parametrize("d,r", D.SHAPES)
def test_batches_reach_their_branch(d, r):
    """polar_fast's first-iteration test, restated: 'below' poses start Newton-Schulz (err < 0.5), 'above' poses go
    to the Jacobi fallback; the four switch batches sit within 1e-9 of the switch."""
    for name in D.POLAR_BATCHES:
        M, _, branch = D.polar_batch(d, r, name)
        err = D.ns_test_value(M, d)
        assert (err < 0.5).all() if branch == "below" else (err >= 0.5).all(), name
        if name.startswith(("below_", "above_")):
            assert (np.abs(err - 0.5) <= 0.5 * 1.1e-9).all() and (np.abs(err - 0.5) >= 0.5 * 0.9e-9).all(), name
    M, _, _ = D.polar_batch(d, r, "graded")
    for name, expo in (("graded_2^+100", 100), ("graded_2^-100", -100)):
        assert np.array_equal(D.polar_batch(d, r, name)[0], np.ldexp(M, expo))


def _mp_matrix(mp, A):
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in A])


def _mp_polar(mp, A):
    U, _, V = mp.svd_r(_mp_matrix(mp, A), full_matrices=False)
    return U * V


def _mp_qf(mp, A):
    """Thin Q with positive diagonal R from mpmath's Householder QR."""
    d = A.shape[1]
    Q, R = mp.qr(_mp_matrix(mp, A))
    return mp.matrix([[Q[i, j] * mp.sign(R[j, j]) for j in range(d)] for i in range(A.shape[0])])


def _mp_gap(mp, ref, want):
    return max(abs(mp.mpf(float(ref[i, j])) + mp.mpf(float(ref[i, j] - LD(float(ref[i, j])))) - want[i, j])
               for i in range(ref.shape[0]) for j in range(ref.shape[1]))


@pytest.mark.parametrize("d,r", D.CORE)
def test_references_agree_with_mpmath(d, r):
    """One pose per batch at 50 digits: polar_ref and qf_ref within 4 eps_longdouble kappa of mpmath's SVD and QR."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    eps_ld = float(np.finfo(LD).eps)
    with mp.workdps(50):
        for k, name in enumerate(D.POLAR_BATCHES):
            M, sig, _ = D.polar_batch(d, r, name)
            j = (17 * k + 3) % D.N
            A = D.to_poses(M, d)[j, :, :d]
            got = D.polar_ref(A)
            assert _mp_gap(mp, got, _mp_polar(mp, A)) <= 4 * eps_ld * D.kappa_polar(sig, r, d), name
        X, V = D.qf_batch(d, r)
        for k, s in enumerate(D.QF_SCALES):
            ref, cond, MY = D.qf_reference(X, V, s, d)
            j = (2 * k + 31) % D.N + (k % 2)  # even and odd poses: without and with the normal component
            A64 = MY[j].astype(np.float64)  # the mpmath input must be the same matrix: take its float64 rounding
            got = D.qf_ref(A64)
            assert _mp_gap(mp, got, _mp_qf(mp, A64)) <= 4 * eps_ld * cond[j], s


def test_bars_are_the_documented_ones():
    assert (D.K_POLAR, D.K_QF, D.K_BJ) == (8 * D.ORACLE_POLAR, 8 * D.ORACLE_QF, 8 * D.ORACLE_BJ)
    for k, v in (("ORACLE_POLAR", D.ORACLE_POLAR), ("ORACLE_QF", D.ORACLE_QF), ("ORACLE_BJ", D.ORACLE_BJ)):
        assert f"{k} = {v:g}" in D.__doc__, k


@pytest.mark.parametrize("d,r", D.SHAPES)
def test_oracle_polar_within_bar(d, r):
    for name in D.POLAR_BATCHES:
        M, sig, _ = D.polar_batch(d, r, name)
        got = O.lifted_project(M, d)
        ratio = D.pose_max(got, D.polar_reference(M, d), d) / (D.EPS * D.kappa_polar(sig, r, d))
        print(f"polar d={d} r={r} {name}: oracle ratio {ratio.max():.3g} of K = {D.K_POLAR:g}")
        assert ratio.max() <= D.K_POLAR, name
        assert D.ortho_defect(got, d).max() <= D.ORTHO_BAR, name


@pytest.mark.parametrize("d,r", D.SHAPES)
def test_oracle_qf_within_bar(d, r):
    X, V = D.qf_batch(d, r)
    assert D.ortho_defect(X, d).max() <= 4 * D.EPS
    assert np.abs(np.linalg.norm(D.to_poses(V, d), axis=(1, 2)) - 1).max() <= 1e-15 and not V[:, d::d + 1].any()
    worst_cond = 0.0
    for s in D.QF_SCALES:
        ref, cond, MY = D.qf_reference(X, V, s, d)
        got = O.retract_qf(X, s * V, d)
        ratio = D.pose_max(got, ref, d) / (D.EPS * cond)
        print(f"qf d={d} r={r} s={s:g}: cond <= {cond.max():.3g}, oracle ratio {ratio.max():.3g} of K = {D.K_QF:g}")
        assert ratio.max() <= D.K_QF, s
        assert D.ortho_defect(ref, d).max() <= 1e-17
        Rd = np.einsum("jac,jac->jc", D.to_poses(ref, d)[:, :, :d], MY)
        assert (Rd > 0).all()
        worst_cond = max(worst_cond, cond.max())
    if d == 3:  # the rank-2 step: a direction is lost as s grows (in part only where the normal component is)
        assert worst_cond >= 1e7
        if r > d:
            assert cond[1::2].max() < cond[0::2].min()
    if (d, r + 1) in D.SHAPES:
        X, v = D.lift_batch(d, r)
        for alpha in D.LIFT_ALPHAS:
            ref, cond, _ = D.lift_reference(X, v, alpha, d)
            Xl = np.vstack([X, np.zeros((1, X.shape[1]))])
            Dl = np.zeros_like(Xl)
            Dl[-1] = alpha * v
            ratio = D.pose_max(O.retract_qf(Xl, Dl, d), ref, d) / (D.EPS * cond)
            print(f"lift d={d} r={r} alpha={alpha:g}: cond <= {cond.max():.3g}, oracle ratio {ratio.max():.3g}")
            assert ratio.max() <= D.K_QF, alpha


@pytest.mark.parametrize("d,r", D.CORE)
def test_oracle_tangent_within_bar(d, r):
    X, V = D.tangent_batch(d, r)
    ref = D.tangent_ref(X, V, d)
    vmax = np.abs(D.to_poses(V, d)[:, :, :d]).max(axis=(1, 2))
    assert vmax.min() >= 1e6  # V is 1e8 X up to a unit tangent, which is all that stays
    left = np.linalg.norm(D.to_poses(ref.astype(np.float64), d)[:, :, :d], axis=(1, 2))
    assert left.max() <= 1 + 1e-6 and left.min() >= 1e-2
    ratio = D.pose_max(O.tangent_project(X, V, d), ref, d) / (D.EPS * vmax)
    print(f"tangent d={d} r={r}: oracle ratio {ratio.max():.3g} of {D.TANGENT_K:g}")
    assert ratio.max() <= D.TANGENT_K


@pytest.mark.parametrize("d", [2, 3])
def test_block_jacobi_graph_and_oracle_within_bar(d):
    g, A = D.bj_graph(d), D.bj_blocks(d)
    b = d + 1
    assert not ((g["p1"] == D.BJ_ISOLATED) | (g["p2"] == D.BJ_ISOLATED)).any()
    assert np.array_equal(A[D.BJ_ISOLATED], LD(D.BJ_SHIFT) * np.eye(b, dtype=LD))
    assert not (g["p1"] == D.BJ_P2_ONLY).any() and (g["p2"] == D.BJ_P2_ONLY).sum() == 3
    assert np.array_equal(A[D.BJ_P2_ONLY], np.diag(np.diag(A[D.BJ_P2_ONLY])))
    for key, lo, hi in (("kappa", 1e-3, 1e5), ("tau", 1e-3, 1e5)):
        assert g[key].min() >= lo and g[key].max() <= hi and g[key].max() / g[key].min() >= 1e6
    tl = np.linalg.norm(g["t"], axis=1)
    assert tl.min() >= 0.1 and tl.max() <= 100 and tl.max() / tl.min() >= 100
    assert np.abs(np.linalg.det(g["R"]) - 1).max() <= 1e-14
    cond = np.linalg.cond(A.astype(np.float64))
    assert cond.max() >= 1e6  # far beyond the blocks of the suite's other graphs (kappa, tau in [0.5, 50])
    for j in (0, D.BJ_ISOLATED, D.BJ_P2_ONLY, int(np.argmax(cond))):
        Minv = D.bj_inverse_ref(A[j])
        assert np.abs(Minv @ A[j] - np.eye(b)).max() <= 8 * float(np.finfo(LD).eps) * cond[j]
    r = d + 2
    X, V, ref, unit = D.bj_reference(d, r)
    Q = O.connection_laplacian(D.bj_measurements(d), D.N)
    P = O.QuadraticProblem(D.N, d, r)
    P.set_Q(Q)
    ratio = D.pose_max(P.precondition(X, V, O.PRECON_BLOCK_JACOBI), ref, d) / unit
    print(f"block-Jacobi d={d}: cond <= {cond.max():.3g}, oracle ratio {ratio.max():.3g} of K = {D.K_BJ:g}")
    assert ratio.max() <= D.K_BJ


@pytest.mark.parametrize("two_operands", [True, False])
@pytest.mark.parametrize("d,r", D.CORE)
def test_combination_batch_tells_the_agents_apart(d, r, two_operands):
    """The oracle on the exactly rounded combination passes the polar bar; with the coefficients of the next agent
    instead, every agent misses it (in the rotation columns, or in the translation column where project(ca A) only
    changes by a sign); and both branches of polar_fast are reached."""
    A, B = D.combine_batch(d, r)
    B = B if two_operands else None
    M = D.combine_exact(A, B, d)
    ref = D.polar_reference(M, d)
    bar = D.K_POLAR * D.EPS * D.kappa_polar_of(M, d)
    assert (D.pose_max(O.lifted_project(M, d), ref, d) <= bar).all()
    err = D.ns_test_value(M, d)
    assert (err < 0.5).any() and (err >= 0.5).any()
    off = np.concatenate([[0], np.cumsum(D.COMBINE_AGENTS)])
    width = np.asarray(D.COMBINE_AGENTS) * (d + 1)
    ca = np.repeat(np.roll(D.COMBINE_CA, 1), width)
    cb = np.repeat(np.roll(D.COMBINE_CB, 1), width)
    wrong = ca * A + (cb * B if two_operands else 0.0)
    miss = D.pose_max(D.polar_reference(wrong, d), ref, d)
    for k in range(len(D.COMBINE_AGENTS)):
        assert (miss[off[k]:off[k + 1]] > bar[off[k]:off[k + 1]]).all(), k
