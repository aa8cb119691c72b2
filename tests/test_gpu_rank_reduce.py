"""GPU tests of the rank reduction's two kernels (dpgo_hip_gram / dpgo_hip_rank_reduce and their _dev forms) against
the np.longdouble restatement and the seeded fixtures of tests/_rank.py (tests/test_rank_reduce_reference.py checks
that ground on the CPU).  Build-defined, absent from the reference."""
import functools

import numpy as np
import pytest

from tests import _rank as RK
from tests._common import random_point

pytestmark = pytest.mark.gpu
_L = np.longdouble


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


@functools.lru_cache(maxsize=None)
def _generic(d, r, n):
    """A seeded point of full rank r (shared, read-only): the Gram's input and the ill-conditioned reduce's."""
    X = random_point(r, d, n, 100 * d + 10 * r + n)
    X.setflags(write=False)
    return X


# ---------------------------------------------------------------------------------------- Gram
def _gram_dev(H, X, d, misalign):
    """dpgo_hip_gram_dev on torch device buffers (misalign: X starts 8 bytes off a 16-byte boundary: the kernel's
    8-byte staging path)."""
    import torch
    r = X.shape[0]
    n = X.shape[1] // (d + 1)
    off = 1 if misalign else 0
    xt = torch.empty(off + X.size, dtype=torch.float64, device="cuda")
    xt[off:].copy_(torch.from_numpy(H.to_dev_layout(X)))
    ct = torch.full((r * r,), float("nan"), dtype=torch.float64, device="cuda")
    wt = torch.full((H.gram_work_doubles(r, d, n),), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    H.gram_dev(r, d, n, xt.data_ptr() + 8 * off, ct.data_ptr(), wt.data_ptr(), s.cuda_stream)
    s.synchronize()
    return ct.cpu().numpy().reshape(r, r).T.copy()


@pytest.mark.parametrize("d,r", RK.SUPPORTED)
def test_gram_matches_longdouble_entry_by_entry(hip, d, r):
    """Every entry within gamma_m sum|terms| of the np.longdouble Gram, m = tests/_rank.py gram_depth: d + 6 for
    up to 64 poses, d + 7 for 65, d + 8 for 200 (the implemented order; the order-free bound d + 6 + spans + 2 would
    be d + 9 / d + 10 / d + 12).  Measured on an MI355X: the worst |error| / (u sum|terms|) over every case is
    printed below (1.73 when this was written, against m >= 8).  Exactly symmetric; a second launch and the
    misaligned _dev call are bitwise the first."""
    worst = 0.0
    for n in RK.SIZES:
        X = _generic(d, r, n)
        Cl, A = RK.gram(X, d)
        got = hip.gram(X, d)
        assert got.shape == (r, r) and np.array_equal(got, got.T)
        err = np.abs(got.astype(_L) - Cl)
        worst = max(worst, float((err / (RK.U_ROUND * A)).max()))
        assert np.all(err <= RK.gamma(RK.gram_depth(d, n)) * A), (n, float((err / (RK.U_ROUND * A)).max()))
        assert abs(np.trace(got) - d * n) <= 1e-12 * d * n
        assert np.array_equal(hip.gram(X, d), got)
        assert np.array_equal(_gram_dev(hip, X, d, False), got)
        assert np.array_equal(_gram_dev(hip, X, d, True), got)
    print(f"gram d={d} r={r}: worst |error| / (u sum|terms|) = {worst:.3f}")


# ---------------------------------------------------------------------------------------- reduce
def _check_reduce(H, X, d, W, what, orthonormal):
    """hip.rank_reduce(X, d, W) against tests/_rank.py: rotations entry by entry within 1e-13 / min(1, sigma_d(W^T
    Y_j)), translations within gamma_{r+1} sum|terms|.  Returns (X', worst err sigma_d)."""
    r, k = W.shape
    n = X.shape[1] // (d + 1)
    got = H.rank_reduce(X, d, W)
    assert got.shape == (k, X.shape[1]) and np.isfinite(got).all()
    ref = RK.reduce(X, d, W)
    sig = RK.sigma_min(X, d, W)
    Gp, Rp = RK.O.to_poses(got, k, d), RK.O.to_poses(ref, k, d)
    err = np.abs(Gp[:, :, :d] - Rp[:, :, :d]).max(axis=(1, 2))
    bar = 1e-13 / np.minimum(1.0, sig)
    j = int(np.argmax(err / bar))
    assert np.all(err <= bar), (what, j, err[j], sig[j])
    M, A = RK.project(X, d, W)
    tcol = np.arange(d, X.shape[1], d + 1)
    terr = np.abs(got[:, tcol].astype(_L) - M[:, tcol])
    assert np.all(terr <= RK.gamma(r + 1) * A[:, tcol]), what
    if orthonormal:
        G = np.swapaxes(Gp[:, :, :d], 1, 2) @ Gp[:, :, :d]
        assert np.abs(G - np.eye(d)).max() <= 1e-14, what
    return got, float((err * sig).max())


@pytest.mark.parametrize("d,r,k", RK.REDUCIBLE)
def test_reduce_near_low_rank(hip, d, r, k):
    """W from numpy's spectrum (independent of gram_eig).  On this fixture sigma_d >= 0.96, so the bar is at most
    1.04e-13 per entry; the outputs are orthonormal to 1e-14."""
    for n in RK.SIZES:
        _, W = RK.near_low_rank_W(d, r, k, n)
        _check_reduce(hip, RK.near_low_rank(d, r, k, n), d, W, (d, r, k, n), True)


@pytest.mark.parametrize("d,r,k", RK.REDUCIBLE)
def test_reduce_exact_low_rank_keeps_the_gram_of_poses(hip, d, r, k):
    """X of exact rank k: W^T Y_j is already on St(d, k), so X'^T X' = X^T X to 1e-13 max(1, |X^T X|_max) (from 63
    poses on, where the Gram determines all k directions)."""
    for n in RK.SIZES[1:]:
        X = RK.exact_low_rank(d, r, k, n)
        w, U = RK.spectrum(RK.gram(X, d)[0])
        got, _ = _check_reduce(hip, X, d, U[:, :k], (d, r, k, n), True)
        XtX = X.T @ X
        assert np.abs(got.T @ got - XtX).max() <= 1e-13 * max(1.0, np.abs(XtX).max()), (d, r, k, n)


@pytest.mark.parametrize("d,r,k", RK.REDUCIBLE)
def test_reduce_ill_conditioned(hip, d, r, k):
    """A generic point of rank r cut to rank k: W^T Y_j is nearly singular at some poses (over every case the smallest
    sigma_d is 4.7e-5, and 0.6 % of the poses are below 1e-2), and the bar 1e-13 / min(1, sigma_d) holds at every
    pose, none excluded.  Measured on an MI355X: worst err sigma_d over every case 4.6e-15 (printed below)."""
    worst, smin = 0.0, 1.0
    for n in (64, 200):
        X = _generic(d, r, n)
        w, U = RK.spectrum(RK.gram(X, d)[0])
        W = U[:, :k]
        _, es = _check_reduce(hip, X, d, W, (d, r, k, n), False)
        worst, smin = max(worst, es), min(smin, float(RK.sigma_min(X, d, W).min()))
    print(f"reduce d={d} r={r} k={k}: worst err sigma_d = {worst:.3e}, smallest sigma_d = {smin:.3e}")


@pytest.mark.parametrize("d,r,k", [(2, 5, 3), (3, 8, 4), (3, 6, 3)])
def test_reduce_pose_orthogonal_to_W_gives_finite_output(hip, d, r, k):
    """One crafted pose with Y_j exactly orthogonal to W (W^T Y_j = 0: no nearest point exists).  polar_inplace keeps
    a zero column zero, so the block comes out finite -- here exactly zero -- and every other pose is unaffected."""
    n, j = 65, 37
    W = np.eye(r)[:, :k]
    X = np.array(_generic(d, r, n))
    X[:, j * (d + 1):j * (d + 1) + d] = np.eye(r)[:, k:k + d]
    got = hip.rank_reduce(X, d, W)
    assert np.isfinite(got).all()
    blk = got[:, j * (d + 1):(j + 1) * (d + 1)]
    assert np.array_equal(blk[:, :d], np.zeros((k, d)))
    assert np.array_equal(blk[:, d], X[:k, j * (d + 1) + d])
    ref = RK.reduce(X, d, W)
    keep = np.ones(X.shape[1], bool)
    keep[j * (d + 1):(j + 1) * (d + 1)] = False
    sig = np.repeat(np.minimum(1.0, RK.sigma_min(X, d, W)), d + 1)[keep]
    assert np.all(np.abs(got - ref)[:, keep] <= 1e-13 / sig)


def _reduce_dev(H, X, d, W, misalign):
    import torch
    r, k = W.shape
    n = X.shape[1] // (d + 1)
    off = 1 if misalign else 0
    xt = torch.empty(off + X.size, dtype=torch.float64, device="cuda")
    xt[off:].copy_(torch.from_numpy(H.to_dev_layout(X)))
    ot = torch.full((off + n * k * (d + 1),), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    H.rank_reduce_dev(r, d, n, xt.data_ptr() + 8 * off, W, ot.data_ptr() + 8 * off, s.cuda_stream)
    s.synchronize()
    return H.from_dev_layout(ot[off:].cpu().numpy(), k)


@pytest.mark.parametrize("d,r,k", RK.REDUCIBLE)
def test_reduce_misaligned_device_pointers_are_bitwise(hip, d, r, k):
    """The _dev entry with X and X_out offset by one double (the 8-byte streaming paths) gives bitwise the aligned
    result, which is bitwise the host entry's."""
    for n in (64, 200):
        X = RK.near_low_rank(d, r, k, n)
        _, W = RK.near_low_rank_W(d, r, k, n)
        want = hip.rank_reduce(X, d, W)
        assert np.array_equal(_reduce_dev(hip, X, d, W, False), want)
        assert np.array_equal(_reduce_dev(hip, X, d, W, True), want)


def test_reduce_refusals(hip):
    import torch
    X = np.array(_generic(3, 5, 64))
    for W in (np.eye(5)[:, :2], np.eye(5), np.eye(5, 6)):  # k < d, k = r, k > r
        with pytest.raises(hip.DPGOHipError, match="d <= k < r"):
            hip.rank_reduce(X, 3, W)
    with pytest.raises(hip.DPGOHipError, match="unsupported"):
        hip.rank_reduce(np.zeros((9, 4 * 64)), 3, np.eye(9)[:, :3])
    with pytest.raises(hip.DPGOHipError, match="unsupported"):
        hip.gram(np.zeros((9, 4 * 64)), 3)
    xt = torch.zeros(5 * 4 * 64, dtype=torch.float64, device="cuda")
    with pytest.raises(hip.DPGOHipError, match="overlaps"):
        hip.rank_reduce_dev(5, 3, 64, xt.data_ptr(), np.eye(5)[:, :3], xt.data_ptr() + 8 * 100)
    with pytest.raises(hip.DPGOHipError, match="d <= k < r"):
        hip.rank_reduce_dev(3, 3, 64, xt.data_ptr(), np.eye(3), xt.data_ptr())
