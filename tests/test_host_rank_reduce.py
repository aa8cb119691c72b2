"""CPU tests of the rank reduction's host side (no GPU): dpgo_hip_gram_eig against numpy.linalg.eigh on the Grams of
the seeded fixtures of tests/_rank.py, its ordering and sign convention, the degenerate case, and the argument checks
of every new entry that refuses before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _rank as RK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1  # DPGO_HIP_EINVAL
NEW_SYMBOLS = ["dpgo_hip_gram", "dpgo_hip_gram_dev", "dpgo_hip_gram_work_doubles", "dpgo_hip_gram_eig",
               "dpgo_hip_rank_reduce", "dpgo_hip_rank_reduce_dev", "dpgo_graph_rank_reduce", "dpgo_rbcd_gram",
               "dpgo_rbcd_get_X_reduced"]


@pytest.fixture(scope="module")
def H():
    from dpgo_amd import hip
    return hip


def _check_eig(H, Cm, gap_k=None):
    """gram_eig(Cm) against eigh: eigenvalues within 1e-13 w_1, |U^T U - I| <= 1e-14, |U diag(w) U^T - C| <=
    1e-13 w_1, descending, signed; with gap_k the top-gap_k projector within 1e-12 of numpy's."""
    r = Cm.shape[0]
    w, U = H.gram_eig(Cm)
    wn, Un = RK.spectrum(Cm)
    w1 = np.abs(wn).max()
    assert w.shape == (r,) and U.shape == (r, r)
    assert np.all(np.diff(w) <= 0), w
    assert np.abs(w - wn).max() <= 1e-13 * w1, (w, wn)
    assert np.abs(U.T @ U - np.eye(r)).max() <= 1e-14
    assert np.abs((U * w) @ U.T - Cm).max() <= 1e-13 * w1
    for i in range(r):
        assert U[int(np.argmax(np.abs(U[:, i]))), i] > 0, (i, U[:, i])
    if gap_k is not None:
        W, Wn = U[:, :gap_k], Un[:, :gap_k]
        assert np.abs(W @ W.T - Wn @ Wn.T).max() <= 1e-12
    return w, U


@pytest.mark.parametrize("d,r,k", RK.REDUCIBLE)
def test_gram_eig_matches_eigh_on_the_near_low_rank_grams(H, d, r, k):
    for n in RK.SIZES:
        Cm = np.asarray(RK.gram(RK.near_low_rank(d, r, k, n), d)[0], dtype=float)
        w, U = _check_eig(H, Cm, gap_k=k if n >= 63 else None)  # the fixture's gap condition holds from 63 poses on
        if n >= 63:
            assert H.numerical_rank(w, d, 0.1 * w[k - 1] / w[0]) == k


@pytest.mark.parametrize("d,r,k", RK.REDUCIBLE)
def test_gram_eig_on_the_exact_low_rank_grams(H, d, r, k):
    """Trailing eigenvalues at rounding level (<= 1e-14 w_1): the numerical rank is the true one."""
    for n in RK.SIZES:
        Cm = np.asarray(RK.gram(RK.exact_low_rank(d, r, k, n), d)[0], dtype=float)
        w, U = _check_eig(H, Cm, gap_k=k if n >= 63 else None)
        assert np.all(np.abs(w[k:]) <= 1e-13 * w[0])
        if n >= 63:
            assert H.numerical_rank(w, d, 1e-6) == k


@pytest.mark.parametrize("r", range(1, 9))
def test_gram_eig_degenerate_and_diagonal(H, r):
    """C = 3 I: every vector is an eigenvector; U must still be orthonormal (and is the identity: nothing rotates).
    A diagonal C comes back sorted, with unit vectors."""
    w, U = H.gram_eig(3.0 * np.eye(r))
    assert np.array_equal(w, np.full(r, 3.0))
    assert np.abs(U.T @ U - np.eye(r)).max() <= 1e-14 and np.array_equal(U, np.eye(r))
    dg = np.arange(1.0, r + 1.0)
    w, U = H.gram_eig(np.diag(dg))
    assert np.array_equal(w, dg[::-1]) and np.array_equal(U, np.eye(r)[:, ::-1])


def test_gram_eig_random_symmetric_and_sign_convention(H):
    rng = np.random.default_rng(5)
    for r in range(2, 9):
        A = rng.standard_normal((r, r))
        _check_eig(H, A + A.T)          # indefinite: the routine does not need a Gram
        _check_eig(H, -(A @ A.T))       # negative semidefinite: descending still means algebraically
    # equal magnitudes: the first of the equals decides the sign
    w, U = H.gram_eig(np.array([[2.0, 1.0], [1.0, 2.0]]))
    assert np.allclose(w, [3.0, 1.0], rtol=0, atol=1e-15)
    assert U[0, 0] > 0 and U[0, 1] > 0 and U[1, 1] < 0


def test_gram_eig_takes_the_symmetric_part(H):
    rng = np.random.default_rng(6)
    A = rng.standard_normal((4, 4))
    w, U = H.gram_eig(A)
    wn, _ = RK.spectrum(0.5 * (A + A.T))
    assert np.abs(w - wn).max() <= 1e-13 * abs(wn).max()


def test_gram_eig_refuses_bad_arguments(H):
    L = H.lib()
    buf = (C.c_double * 81)()
    dp = C.cast(buf, C.POINTER(C.c_double))
    for r in (0, -1, 9):
        assert L.dpgo_hip_gram_eig(r, dp, dp, dp) == EINVAL, r
    for args in ((None, dp, dp), (dp, None, dp), (dp, dp, None)):
        assert L.dpgo_hip_gram_eig(3, *args) == EINVAL
    for bad in (np.nan, np.inf):
        Cm = np.eye(3)
        Cm[1, 2] = bad
        with pytest.raises(H.DPGOHipError, match="non-finite"):
            H.gram_eig(Cm)
    with pytest.raises(H.DPGOHipError, match="square"):
        H.gram_eig(np.zeros((2, 3)))
    with pytest.raises(H.DPGOHipError, match="r <= 8"):
        H.gram_eig(np.eye(9))


def test_device_entries_refuse_bad_arguments_before_any_device(H):
    """Every EINVAL of gram and rank_reduce is decided on the host, so it shows without a GPU."""
    X = np.zeros((5, 4 * 4))
    W = np.eye(5)[:, :3]
    with pytest.raises(H.DPGOHipError, match="unsupported"):
        H.gram(np.zeros((9, 8)), 3)
    with pytest.raises(H.DPGOHipError, match="unsupported"):
        H.gram(np.zeros((2, 8)), 3)       # r < d
    with pytest.raises(H.DPGOHipError, match="unsupported"):
        H.gram(np.zeros((5, 10)), 4)      # d = 4
    with pytest.raises(H.DPGOHipError, match="n >= 1"):
        H.gram(np.zeros((5, 0)), 3)
    with pytest.raises(H.DPGOHipError, match="d <= k < r"):
        H.rank_reduce(X, 3, np.eye(5)[:, :2])   # k < d
    with pytest.raises(H.DPGOHipError, match="d <= k < r"):
        H.rank_reduce(X, 3, np.eye(5))          # k = r
    with pytest.raises(H.DPGOHipError, match="d <= k < r"):
        H.rank_reduce(X, 3, np.eye(5, 6))       # k > r
    with pytest.raises(H.DPGOHipError, match="unsupported"):
        H.rank_reduce(np.zeros((9, 16)), 3, np.eye(9)[:, :3])
    with pytest.raises(H.DPGOHipError, match="n >= 1"):
        H.rank_reduce(np.zeros((5, 0)), 3, W)
    with pytest.raises(H.DPGOHipError, match="r x k"):
        H.rank_reduce(X, 3, np.eye(4)[:, :3])
    L = H.lib()
    x = np.zeros(5 * 4 * 4)
    w = np.ascontiguousarray(W.T).ravel()
    xp, wp = x.ctypes.data_as(H._dp), w.ctypes.data_as(H._dp)
    assert L.dpgo_hip_rank_reduce(5, 3, 4, xp, 3, wp, xp) == EINVAL  # in place
    tail = C.cast(x.ctypes.data + 8 * 70, H._dp)
    assert L.dpgo_hip_rank_reduce(5, 3, 4, xp, 3, wp, tail) == EINVAL  # out starts inside X
    assert b"overlaps" in L.dpgo_hip_last_error()
    assert L.dpgo_hip_rank_reduce(5, 3, 4, None, 3, wp, xp) == EINVAL
    assert L.dpgo_hip_rank_reduce(5, 3, 4, xp, 3, None, tail) == EINVAL
    assert L.dpgo_hip_gram(5, 3, 4, xp, None) == EINVAL
    assert L.dpgo_hip_gram_dev(5, 3, 4, C.c_void_p(x.ctypes.data), C.c_void_p(x.ctypes.data), None, None) == EINVAL
    assert H.gram_work_doubles(5, 3, 1) == 15 and H.gram_work_doubles(5, 3, 128) == 15
    assert H.gram_work_doubles(5, 3, 129) == 30 and H.gram_work_doubles(8, 2, 10 ** 6) == 36 * 7813
    assert H.gram_work_doubles(9, 3, 10) == 0 and H.gram_work_doubles(5, 3, 0) == 0
    assert RK.GRAM_SPANS * 64 == 128  # the restated layout the GPU tests' rounding depth rests on


def test_new_symbols_are_exported_and_bound(H):
    lib = os.path.join(ROOT, "dpgo_amd", "libdpgo_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dpgo_\w+)", out))
    assert set(NEW_SYMBOLS) <= exported
    assert set(NEW_SYMBOLS) <= set(H.EXPORTED_SYMBOLS)
    for name in ("gram", "gram_dev", "gram_eig", "rank_reduce", "rank_reduce_dev"):
        assert callable(getattr(H, name))
    for cls, name in ((H.Graph, "rank_reduce"), (H.Rbcd, "gram"), (H.Rbcd, "get_X_reduced_into")):
        assert callable(getattr(cls, name))
    assert C.sizeof(H.RankInfo) == 11 * 8
