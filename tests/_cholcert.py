"""The Cholesky certificate's test inputs and their dense reference (test infrastructure, no GPU).

Every (input, sigma) pair the GPU tests decide is listed here once; the reference is the oracle's explicit
S = O.certificate_matrix (dense), its eigenvalues by np.linalg.eigvalsh, and the decision "S + sigma I is positive
definite" by np.linalg.cholesky succeeding or failing.  test_certify_chol_reference.py asserts that each pair is decided
with margin, so the device factorisation's rounding cannot flip one.  Each case is built once per process."""
import dataclasses
import functools
import os
from types import SimpleNamespace

import numpy as np

from oracle import dpgo_oracle as O
from tests._common import GOLDEN, load_meas, random_point

# (kind, dataset, r): "rand" random_point(r, d, n, 5); "opt" the golden RTR optimum; "rand60" a random point on the
# dataset's first 60 poses; "weighted" a random point with loop-closure weights drawn from {0, 0.3, 1}
MAIN_RANDOM = [("rand", "tinyGrid3D", 3), ("rand", "smallGrid3D", 5), ("rand", "input_INTEL_g2o", 3)]
OPT_SMALL = ("opt", "smallGrid3D", 5)
OPT_TINY = ("opt", "tinyGrid3D", 3)
EVERY_RANK = [("rand", "tinyGrid3D", r) for r in range(3, 9)] + [("rand60", "input_INTEL_g2o", r) for r in range(2, 9)]
WEIGHTED = ("weighted", "smallGrid3D", 5)
DECISION_CASES = list(dict.fromkeys(MAIN_RANDOM + [OPT_SMALL, OPT_TINY] + EVERY_RANK))
BRACKET_CASES = MAIN_RANDOM + [OPT_TINY]


def prefix(meas, n):
    """The measurements among the first n poses."""
    keep = (meas.p1 < n) & (meas.p2 < n)
    return dataclasses.replace(meas, r1=meas.r1[keep], r2=meas.r2[keep], p1=meas.p1[keep], p2=meas.p2[keep],
                               R=meas.R[keep], t=meas.t[keep], kappa=meas.kappa[keep], tau=meas.tau[keep],
                               weight=meas.weight[keep], num_poses=n)


def loop_closure_weights(meas, seed=11):
    """Weights in the measurements' order: 1 on odometry, drawn from {0, 0.3, 1} on the loop closures."""
    rng = np.random.default_rng(seed)
    w = np.ones(len(meas.p1))
    lc = np.flatnonzero(meas.p2 != meas.p1 + 1)
    w[lc] = rng.choice([0.0, 0.3, 1.0], size=lc.size)
    return w


@functools.lru_cache(maxsize=None)
def case(key):
    """The input of `key` with its dense reference: meas (weights applied), d, n, r, X, S (dense), ev (ascending),
    lam = ev[0], lam_max = max |ev|."""
    kind, name, r = key
    meas = load_meas(name)
    if kind == "rand60":
        meas = prefix(meas, 60)
    if kind == "weighted":
        meas = dataclasses.replace(meas, weight=loop_closure_weights(meas))
    d, n = meas.d, meas.num_poses
    if kind == "opt":
        X = np.load(os.path.join(GOLDEN, f"{name}.r{r}.rtr.npz"))["Xopt"]
    else:
        X = random_point(r, d, n, 5)
    S = O.certificate_matrix(O.connection_laplacian(meas, n), X, d).toarray()
    S = 0.5 * (S + S.T)
    ev = np.linalg.eigvalsh(S)
    return SimpleNamespace(key=key, meas=meas, d=d, n=n, r=r, X=X, S=S, ev=ev, lam=float(ev[0]),
                           lam_max=float(np.abs(ev).max()))


def sigmas(key):
    """[(sigma, expected positive definite)] of the case: one on each side of -lambda_min."""
    c = case(key)
    if key == OPT_SMALL:  # lambda_min ~ 1e-13: the optimum's null space
        return [(1e-6 * c.lam_max, True), (-1e-6 * c.lam_max, False)]
    if key == OPT_TINY:  # lambda_min = -1.10e-3: a rank-3 critical point that is not the relaxation's optimum
        return [(2.0 * abs(c.lam), True), (0.5 * abs(c.lam), False)]
    return [(-1.25 * c.lam, True), (-0.75 * c.lam, False)]


def reference_pd(S, sigma):
    """The reference decision: does dense Cholesky of S + sigma I succeed?"""
    try:
        np.linalg.cholesky(S + sigma * np.eye(S.shape[0]))
        return True
    except np.linalg.LinAlgError:
        return False
