"""Rank reduction restated in numpy / np.longdouble, and its seeded fixtures (test infrastructure).

With X r x (d+1) n, pose j = [Y_j | p_j] (build-defined; the reference has none):
  Gram      C = sum_j Y_j Y_j^T over the rotation columns only;
  spectrum  w_1 >= ... >= w_r, eigenvectors the columns of U, each column's largest-magnitude entry positive;
  rank      k = max(d, #{i : w_i > tol w_1});
  reduce    X'_j = [polar(W^T Y_j) | W^T p_j] with W = U[:, :k], polar = the oracle's project_to_stiefel.
"""
import functools

import numpy as np

from oracle import dpgo_oracle as O
from tests._common import random_point

_L = np.longdouble
U_ROUND = 2.0 ** -53
SIZES = (1, 63, 64, 65, 200)  # a partial block, a full one, a full one and a one-pose block, several blocks
SUPPORTED = [(2, r) for r in range(2, 9)] + [(3, r) for r in range(3, 9)]  # the 13 compiled (d, r)
REDUCIBLE = [(d, r, k) for d, r in SUPPORTED for k in range(d, r)]         # every d <= k < r
# k_gram's layout, restated (kernels.h): a block sums GRAM_SPANS consecutive 64-pose spans before its lane tree
GRAM_SPANS = 2


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u)."""
    return m * U_ROUND / (1.0 - m * U_ROUND)


def gram_depth(d, n):
    """Roundings on the longest path into one entry of the device Gram, as k_gram / k_gram_finish order the sum:
    d for a pose's product (one multiplication, d - 1 FMAs), one addition per further span a lane walks
    (min(GRAM_SPANS, spans) - 1), 6 for the block's 64-lane butterfly, and, when there is more than one block,
    k_gram_finish's ceil(blocks / 1024) - 1 serial additions per thread, the butterfly steps that meet a lane holding
    a partial, ceil(log2(min(blocks, 64))), and one addition per further wave that holds one,
    min(ceil(blocks / 64), 16) - 1 (adding an exact zero does not round).  Never more than the d + 6 + spans + 2
    that any order over 64-pose spans would need."""
    spans = (n + 63) // 64
    blocks = (spans + GRAM_SPANS - 1) // GRAM_SPANS
    m = d + (min(GRAM_SPANS, spans) - 1) + 6
    if blocks > 1:
        m += (blocks + 1023) // 1024 - 1 + int(np.ceil(np.log2(min(blocks, 64)))) + min((blocks + 63) // 64, 16) - 1
    assert m <= d + 6 + spans + 2
    return m


def rotations(X, d):
    """Y: n x r x d, the rotation columns of every pose."""
    return O.to_poses(np.asarray(X), X.shape[0], d)[:, :, :d]


def gram(X, d):
    """(C, A) in np.longdouble: C = sum_j Y_j Y_j^T and A = the same sum over the terms' magnitudes."""
    Y = rotations(X, d).astype(_L)
    C = np.einsum("jac,jbc->ab", Y, Y)
    A = np.einsum("jac,jbc->ab", np.abs(Y), np.abs(Y))
    return C, A


def fix_signs(U):
    """Each column's largest-magnitude entry (the first of equals) made positive."""
    U = np.array(U, dtype=float)
    for i in range(U.shape[1]):
        if U[int(np.argmax(np.abs(U[:, i]))), i] < 0:
            U[:, i] = -U[:, i]
    return U


def spectrum(C):
    """(w descending, U) of the symmetric C by numpy.linalg.eigh, with the sign convention."""
    w, U = np.linalg.eigh(np.asarray(C, dtype=float))
    return w[::-1].copy(), fix_signs(U[:, ::-1])


def numerical_rank(w, d, tol):
    return max(d, int(np.count_nonzero(np.asarray(w) > tol * w[0])))


def project(X, d, W):
    """(M, A): M = W^T X (k x (d+1) n) in np.longdouble and A = |W|^T |X|, the sums of the terms' magnitudes."""
    WL, XL = np.asarray(W).astype(_L), np.asarray(X).astype(_L)
    return WL.T @ XL, np.abs(WL).T @ np.abs(XL)


def reduce(X, d, W):
    """X' (k x (d+1) n, float64) = per pose [project_to_stiefel(W^T Y_j) | W^T p_j]; the products in longdouble."""
    k = W.shape[1]
    M, _ = project(X, d, W)
    P = O.to_poses(np.asarray(M, dtype=float), k, d).copy()
    P[:, :, :d] = O.project_to_stiefel(P[:, :, :d])
    return O.from_poses(P)


def sigma_min(X, d, W):
    """sigma_d(W^T Y_j) per pose."""
    return np.linalg.svd(np.asarray(W).T @ rotations(X, d), compute_uv=False)[:, -1]


def _basis(r, k):
    return np.linalg.qr(np.random.default_rng(10 * r + k).standard_normal((r, k)))[0]


@functools.lru_cache(maxsize=None)
def exact_low_rank(d, r, k, n):
    """X = G T: a point of rank exactly k (up to rounding) at rank r, T seeded on the rank-k manifold.  Read-only."""
    X = _basis(r, k) @ random_point(k, d, n, 1000 * d + 100 * r + 10 * k + n)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def near_low_rank(d, r, k, n):
    """The exact-low-rank point plus noise of sigma 0.05, projected back onto the rank-r manifold.  Read-only."""
    E = np.random.default_rng(n + k).standard_normal((r, (d + 1) * n))
    X = O.lifted_project(np.array(exact_low_rank(d, r, k, n)) + 0.05 * E, d)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def near_low_rank_W(d, r, k, n):
    """(w, W): numpy's spectrum of the near-low-rank fixture's Gram and its leading k eigenvectors."""
    C, _ = gram(near_low_rank(d, r, k, n), d)
    w, U = spectrum(C)
    W = U[:, :k].copy()
    W.setflags(write=False)
    return w, W
