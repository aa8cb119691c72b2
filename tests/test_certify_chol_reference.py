"""The Cholesky certificate's dense reference (no GPU): every (input, sigma) pair that test_gpu_certify_chol.py asks
the device to decide is decided by np.linalg.cholesky of the oracle's explicit S(X) + sigma I, and with margin.

Margin: the device factorisation is backward stable, so it decides the sign of lambda_min(S + sigma I) correctly when
|lambda_min(S) + sigma| is well above c n eps |S|; the smallest margin asked for here is 0.5e-6 |lambda|_max, seven
orders above eps |lambda|_max.  The pairs on lambda_min(S) = 0 itself (sigma = 0 at an optimum: a singular matrix)
are not used by any test."""
import numpy as np
import pytest

from tests import _cholcert as CC

MARGIN = 0.5e-6  # of |lambda|_max


@pytest.mark.parametrize("key", CC.DECISION_CASES + [CC.WEIGHTED], ids=lambda k: "-".join(map(str, k)))
def test_pairs_decided_with_margin(key):
    c = CC.case(key)
    for sigma, pd in CC.sigmas(key):
        assert CC.reference_pd(c.S, sigma) is pd, (key, sigma)
        gap = c.lam + sigma
        assert (gap > 0) is pd
        assert abs(gap) >= MARGIN * c.lam_max, (key, sigma, gap, c.lam_max)
        print(f"{key}: sigma {sigma:.6e} lambda_min {c.lam:.6e} margin {abs(gap) / c.lam_max:.2e} |lambda|max")


@pytest.mark.parametrize("key,lam", zip(CC.MAIN_RANDOM, [-294.6, -646.4, -20344.9]))
def test_random_point_eigenvalues(key, lam):
    """The three random-point inputs' lambda_min, to the digits the figures are quoted with."""
    assert round(CC.case(key).lam, 1) == lam


def test_optimum_eigenvalues():
    small, tiny = CC.case(CC.OPT_SMALL), CC.case(CC.OPT_TINY)
    assert abs(small.lam) <= 1e-9 * small.lam_max  # 1.7e-13: zero up to rounding
    assert round(small.lam_max) == 1178
    assert abs(tiny.lam + 1.10e-3) <= 0.005e-3


def test_weights_cover_every_value():
    """The weighted case draws all of 0, 0.3 and 1 on its loop closures and leaves odometry at 1."""
    m = CC.case(CC.WEIGHTED).meas
    lc = m.p2 != m.p1 + 1
    assert set(np.unique(m.weight[lc])) == {0.0, 0.3, 1.0}
    assert np.all(m.weight[~lc] == 1.0)
