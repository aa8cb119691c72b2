"""CPU checks of the ground the rank-reduction GPU tests stand on (tests/_rank.py; no GPU, no native code): the
seeded fixtures have the gap and the conditioning the GPU bars assume, an exactly low-rank point shows it in its Gram
spectrum, and on the ring graphs the staircase's certified iterate reduces to rank d without losing the optimum."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _rank as RK
from tests import _ring as RG


@pytest.mark.parametrize("d,r,k", RK.REDUCIBLE)
def test_near_low_rank_fixture_is_well_conditioned_with_a_gap(d, r, k):
    """sigma_d(W^T Y_j) >= 0.9 at every pose, and w_k / w_{k+1} >= 10 from 63 poses on (measured over every case:
    smallest sigma_d 0.964, smallest gap 42)."""
    for n in RK.SIZES:
        X = RK.near_low_rank(d, r, k, n)
        w, W = RK.near_low_rank_W(d, r, k, n)
        assert np.all(np.diff(w) <= 0) and abs(w.sum() - d * n) <= 1e-12 * d * n
        assert np.abs(W.T @ W - np.eye(k)).max() <= 1e-14
        assert RK.sigma_min(X, d, W).min() >= 0.9, (n, RK.sigma_min(X, d, W).min())
        if n >= 63:
            assert w[k - 1] / w[k] >= 10, (n, w)
            assert RK.numerical_rank(w, d, 0.1 * w[k - 1] / w[0]) == k


@pytest.mark.parametrize("d,r,k", RK.REDUCIBLE)
def test_exact_low_rank_fixture_has_a_null_trailing_spectrum(d, r, k):
    """X = G T: trailing eigenvalues <= 1e-14 w_1 (measured: 6.2e-16), at least d eigenvalues >= 1, the numerical
    rank is k (from k poses' worth of data on), and the reduction keeps X^T X."""
    for n in RK.SIZES:
        X = RK.exact_low_rank(d, r, k, n)
        w, U = RK.spectrum(RK.gram(X, d)[0])
        assert np.all(np.abs(w[k:]) <= 1e-14 * w[0]), (n, w)
        assert np.all(w[:d] >= 1 - 1e-12)
        if n >= 63:
            assert RK.numerical_rank(w, d, 1e-6) == k
            Xk = RK.reduce(X, d, U[:, :k])
            assert np.abs(Xk.T @ Xk - X.T @ X).max() <= 1e-13 * max(1.0, np.abs(X.T @ X).max())


def test_spectrum_convention():
    C = np.diag([1.0, 3.0, 2.0])
    w, U = RK.spectrum(C)
    assert np.array_equal(w, [3.0, 2.0, 1.0])
    assert np.array_equal(U, np.eye(3)[:, [1, 2, 0]])
    assert np.array_equal(RK.fix_signs(np.array([[0.6, -0.8], [-0.8, -0.6]])), [[-0.6, 0.8], [0.8, 0.6]])
    assert RK.numerical_rank(np.array([4.0, 1.0, 1e-9]), 2, 1e-6) == 2
    assert RK.numerical_rank(np.array([4.0, 1e-9, 1e-12]), 2, 1e-6) == 2  # never below d
    assert RK.numerical_rank(np.array([4.0, 1.0, 1e-3]), 2, 1e-6) == 3


def test_gram_depth_never_exceeds_the_order_free_bound():
    for d in (2, 3):
        assert [RK.gram_depth(d, n) for n in RK.SIZES] == [d + 6, d + 6, d + 6, d + 7, d + 8]
        assert RK.gram_depth(d, 10 ** 6) == d + 1 + 6 + 7 + 6 + 15


@pytest.fixture(scope="module", params=[2, 3])
def ring_top(request):
    """The RTR staircase's certified iterate on the ring (rank d + 2), shared and read-only."""
    d = request.param
    meas = RG.ring(d)
    Q = O.connection_laplacian(meas, meas.num_poses)
    X, levels = RG.staircase_rtr(meas, RG.winding2(meas))
    X.setflags(write=False)
    return dict(d=d, Q=Q, X=X, levels=levels)


def test_ring_certified_iterate_reduces_to_rank_d(ring_top):
    """The staircase climbed d -> d + 2; its certified iterate has numerical rank d at tol 1e-6 (trailing eigenvalues
    measured <= 2e-16 relative), and its reduction to rank d is the global optimum: |f| <= 1e-12 and
    lambda_min(S) >= -1e-9."""
    d, Q, X = ring_top["d"], ring_top["Q"], ring_top["X"]
    assert X.shape[0] == d + 2 and ring_top["levels"][-1]["lambda_min"] >= -1e-9
    w, U = RK.spectrum(RK.gram(X, d)[0])
    print("ring d =", d, "relative spectrum", w / w[0])
    assert RK.numerical_rank(w, d, 1e-6) == d
    assert np.all(w[d:] <= 1e-12 * w[0])
    Xd = RK.reduce(X, d, U[:, :d])
    assert Xd.shape == (d, X.shape[1])
    assert abs(RG.cost(Q, Xd)) <= 1e-12
    assert RG.min_eig(Q, Xd, d)[0] >= -1e-9
