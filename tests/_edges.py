"""Edge errors restated in np.longdouble, their rounding bounds and seeded fixtures (test infrastructure).

For a measurement e = (p1, p2, R, t, kappa, tau) and poses [Y_j | p_j] of r x (d+1) doubles (the
reference has the per-edge computeMeasurementError, src/DPGO_utils.cpp:509-515, and no batch form):
  rot_e = |Y_p1 R - Y_p2|_F^2,  tra_e = |p_p2 - p_p1 - Y_p1 t|^2,  err_e = kappa rot_e + tau tra_e,
  cost  = 1/2 sum_e w_e err_e.

The bounds belong to k_edge_errors' operation order (kernels.hip), which is the same for every edge:
  v  = Y1[a,0] R[0,c], then d - 1 FMAs, then v - Y2[a,c]:          at most d + 1 roundings on any term's path;
  dt = (p2[a] - p1[a]) - yt, yt = Y1[a,0] t[0] then d - 1 FMAs:    at most d + 1 (yt's first product: d, then the
                                                                   subtraction; p2 - p1: 2);
  rot = fma(df, df, rot) over the r d entries, row by row:         a chain of r d roundings (tra: r);
  err = (kappa rot) + (tau tra):                                   two more on rot's path.
So an entry's error is |delta| <= gamma_{d+1} (sum of the magnitudes of its terms), and the longest sum of squares
has k = SQ_DEPTH(d, r) = r d + 2 roundings on its first square's path into err.
"""
import functools

import numpy as np

from oracle import dpgo_oracle as O
from tests._rank import SUPPORTED, U_ROUND, gamma  # noqa: F401  (re-exported)

_L = np.longdouble
EDGE_BLOCK = 256       # kEdgeErrThreads (kernels.h): edges per block partial
FINISH_THREADS = 1024  # kEdgeFinishThreads (kernels.hip)


def sq_depth(d, r):
    """k of the err bound: the r d chained FMAs of rot, the product with kappa and the final addition."""
    return r * d + 2


def cost_depth(m):
    """Roundings on the longest path of one term (0.5 w_e) err_e into the cost, as k_edge_errors /
    k_edge_cost_finish order the sum: 1 for the term's product, 6 for the wave's xor butterfly, 3 for the block's four
    wave sums in order; then in the finishing block ceil(blocks / 1024) - 1 serial additions per thread (the first
    adds to an exact zero), 6 butterfly steps and 15 additions of the wave sums.  Additions of exact zeros are
    counted: the depth only has to be an upper bound."""
    blocks = (m + EDGE_BLOCK - 1) // EDGE_BLOCK
    return 1 + 6 + 3 + max((blocks + FINISH_THREADS - 1) // FINISH_THREADS - 1, 0) + 6 + 15


def _poses(X, d):
    r = X.shape[0]
    return O.to_poses(np.asarray(X), r, d)


def residuals(X, d, p1, p2, R, t):
    """(V, Vabs, Dt, Dtabs) in np.longdouble: the m x r x d rotation differences Y1 R - Y2 and the m x r translation
    differences p2 - p1 - Y1 t, each with the sum of the magnitudes of its terms."""
    P = _poses(X, d).astype(_L)
    p1 = np.asarray(p1, np.int64)
    p2 = np.asarray(p2, np.int64)
    RL = np.asarray(R).astype(_L).reshape(len(p1), d, d)
    tL = np.asarray(t).astype(_L).reshape(len(p1), d)
    Y1, Y2 = P[p1][:, :, :d], P[p2][:, :, :d]
    q1, q2 = P[p1][:, :, d], P[p2][:, :, d]
    V = np.einsum("eau,euc->eac", Y1, RL) - Y2
    Vabs = np.einsum("eau,euc->eac", np.abs(Y1), np.abs(RL)) + np.abs(Y2)
    Yt = np.einsum("eau,eu->ea", Y1, tL)
    Dt = q2 - q1 - Yt
    Dtabs = np.abs(q2) + np.abs(q1) + np.einsum("eau,eu->ea", np.abs(Y1), np.abs(tL))
    return V, Vabs, Dt, Dtabs


def edge_errors(X, d, p1, p2, R, t, kappa, tau):
    """dict(rot, tra, err) per edge in np.longdouble, and their bounds rot_bound, tra_bound, err_bound for the
    kernel's order:
      |rot - rot_ref| <= sum (2 |v| |delta| + delta^2) + gamma_{r d} rot_ref,   |delta| <= gamma_{d+1} Vabs,
      |tra - tra_ref| <= sum (2 |dt| |delta| + delta^2) + gamma_r tra_ref,
      |err - err_ref| <= kappa sum (...) + tau sum (...) + gamma_k err_ref,      k = sq_depth(d, r)."""
    r = np.asarray(X).shape[0]
    V, Vabs, Dt, Dtabs = residuals(X, d, p1, p2, R, t)
    kL, tL = np.asarray(kappa).astype(_L), np.asarray(tau).astype(_L)
    rot = np.sum(V * V, axis=(1, 2))
    tra = np.sum(Dt * Dt, axis=1)
    err = kL * rot + tL * tra
    g = _L(gamma(d + 1))
    dv, dd = g * Vabs, g * Dtabs
    rot_first = np.sum(2 * np.abs(V) * dv + dv * dv, axis=(1, 2))
    tra_first = np.sum(2 * np.abs(Dt) * dd + dd * dd, axis=1)
    return dict(rot=rot, tra=tra, err=err,
                rot_bound=rot_first + _L(gamma(r * d)) * rot,
                tra_bound=tra_first + _L(gamma(r)) * tra,
                err_bound=kL * rot_first + tL * tra_first + _L(gamma(sq_depth(d, r))) * err)


def cost(err, w=None):
    """(cost, A): 1/2 sum w err in np.longdouble and the sum of the terms' magnitudes."""
    e = np.asarray(err).astype(_L)
    wl = np.ones_like(e) if w is None else np.asarray(w).astype(_L)
    terms = wl * e / 2
    return np.sum(terms, dtype=_L), np.sum(np.abs(terms), dtype=_L)


def cost_bound(err, w=None):
    """gamma_k sum |1/2 w err|, k = cost_depth(m): the bound on |cost - 1/2 sum w err| for the kernel's own err output
    (the sum in np.longdouble; 0.5 w is exact, the term's product is the counted 1).  The errors themselves are tied
    to the restatement edge by edge, so nothing is added for them here."""
    _, A = cost(err, w)
    return _L(gamma(cost_depth(len(np.asarray(err))))) * A


def cost_within_bound(got, err, w=None):
    """Is the device cost `got` within cost_bound of 1/2 sum w err, err being the device's own per-edge output?"""
    want, _ = cost(err, w)
    return bool(abs(_L(got) - want) <= cost_bound(err, w))


def meas_arrays(meas):
    """The measurement arrays of an O.Measurements as hip.edge_errors takes them."""
    return dict(p1=np.asarray(meas.p1, np.int32), p2=np.asarray(meas.p2, np.int32), R=np.asarray(meas.R, np.float64),
                t=np.asarray(meas.t, np.float64), kappa=np.asarray(meas.kappa, np.float64),
                tau=np.asarray(meas.tau, np.float64))


@functools.lru_cache(maxsize=None)
def noise_free(d, n=200, m=1000, seed=11):
    """(arrays, T): m measurements that are exactly (up to rounding) the relative poses of n seeded ground-truth
    poses T (d x (d+1) n) -- the case where the cancellation in Y1 R - Y2 is total.  Edge e joins two distinct
    seeded poses; kappa, tau uniform in [0.5, 50].  Read-only."""
    rng = O.SplitMix64(seed * 100 + d)
    b = d + 1
    Rg = [O.project_to_rotation(np.array([[rng.normal() for _ in range(d)] for _ in range(d)])) for _ in range(n)]
    tg = [np.array([10.0 * rng.uniform() - 5.0 for _ in range(d)]) for _ in range(n)]
    p1 = np.zeros(m, np.int32)
    p2 = np.zeros(m, np.int32)
    R = np.zeros((m, d, d))
    t = np.zeros((m, d))
    kappa = np.zeros(m)
    tau = np.zeros(m)
    for e in range(m):
        i = int(rng.next_u64() % n)
        j = (i + 1 + int(rng.next_u64() % (n - 1))) % n
        p1[e], p2[e] = i, j
        R[e] = Rg[i].T @ Rg[j]
        t[e] = Rg[i].T @ (tg[j] - tg[i])
        kappa[e] = 0.5 + 49.5 * rng.uniform()
        tau[e] = 0.5 + 49.5 * rng.uniform()
    T = np.zeros((d, b * n))
    for j in range(n):
        T[:, j * b:j * b + d] = Rg[j]
        T[:, j * b + d] = tg[j]
    arrays = dict(p1=p1, p2=p2, R=R, t=t, kappa=kappa, tau=tau)
    for a in list(arrays.values()) + [T]:
        a.setflags(write=False)
    return arrays, T


@functools.lru_cache(maxsize=None)
def random_edges(d, n, m, seed=3):
    """m seeded measurements between distinct poses of [0, n): random rotations, translations in [-5, 5], kappa and
    tau in [0.5, 50].  Read-only."""
    rng = O.SplitMix64(seed * 10000 + 100 * d + n + m)
    p1 = np.zeros(m, np.int32)
    p2 = np.zeros(m, np.int32)
    R = np.zeros((m, d, d))
    t = np.zeros((m, d))
    for e in range(m):
        i = int(rng.next_u64() % n)
        p1[e], p2[e] = i, (i + 1 + int(rng.next_u64() % (n - 1))) % n
        R[e] = O.project_to_rotation(np.array([[rng.normal() for _ in range(d)] for _ in range(d)]))
        t[e] = [10.0 * rng.uniform() - 5.0 for _ in range(d)]
    kappa = np.array([0.5 + 49.5 * rng.uniform() for _ in range(m)])
    tau = np.array([0.5 + 49.5 * rng.uniform() for _ in range(m)])
    arrays = dict(p1=p1, p2=p2, R=R, t=t, kappa=kappa, tau=tau)
    for a in arrays.values():
        a.setflags(write=False)
    return arrays
