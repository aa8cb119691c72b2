"""Trajectory evaluation restated in np.longdouble, its rounding bounds and seeded fixtures (test infrastructure).

Build-defined (the reference has none of it).  A trajectory is a d x (d+1) n matrix, pose j
the block [R_j | t_j]; That is the estimate, T the truth, use a mask (None = every pose).

  moments   with a = fl(t^_j - s^), b = fl(t_j - s) (the float64 subtraction, reproduced exactly):
            [count, sum |a|^2, sum |b|^2, sum a, sum b, M = sum b a^T (column-major)]
  alignment n = count, mu^ = s^ + sum a / n, mu = s + sum b / n, C = M - (sum b)(sum a)^T / n = U S V^T,
            A = U diag(1, .., det(U V^T)) V^T, a = mu - A mu^
  errors    tra_sq = |A t^ + a - t|^2, rot_sq = |A R^ - R|_F^2 per pose, sums = [count, sum, sum, max, max]
  relative  R_e = R_p1^T R_p2, t_e = R_p1^T (t_p2 - t_p1)

Every sum comes with the sum of the magnitudes of its terms, as tests/_rank.py and tests/_edges.py do.  The bounds
belong to the kernels' operation orders (kernels.hip):
  k_traj_moments  a term is at most d roundings (a squared norm: one product, d - 1 FMAs); the sums go through
                  tree_depth(n) more (below);
  k_traj_errors   A t^ + a - t: d roundings for the row product, one for + a, one for - t (d + 2); the squares
                  chain through d FMAs (gamma_{d+1} covers them); A R^ - R: d + 1, its d^2 squares gamma_{d^2+1};
  k_relative_poses  d roundings for the product and one for t_p2 - t_p1: gamma_{d+1} on the terms' magnitudes.
"""
import functools
import math

import numpy as np

from oracle import dpgo_oracle as O
from tests._rank import U_ROUND, gamma  # noqa: F401  (re-exported)

_L = np.longdouble
SPAN = 64              # poses per span (kernels.hip)
TRAJ_SPANS = 2         # kTrajSpans (kernels.h): spans per block partial
FINISH_THREADS = 1024  # kTrajFinishThreads (kernels.hip)
POSE_SIZES = (1, 127, 128, 129, 1000)  # a partial block, a full one, a full one plus one pose, several blocks
EDGE_SIZES = (1, 255, 256, 257, 1000)


def moments_len(d):
    return 3 + 2 * d + d * d


def _clog2(x):
    return 0 if x <= 1 else int(math.ceil(math.log2(x)))


def tree_depth(n):
    """Roundings a term meets on the longest path through k_traj_moments' / k_traj_errors' sums and k_traj_finish, for
    n poses.  Additions of an exact zero are exact and are not counted: a thread's first term, the butterfly levels
    whose partner lanes hold no pose, the finishing block's threads and waves beyond the partials.
      in the block    1 when a second span exists, then ceil(log2(min(n, 64))) butterfly levels;
      in the finish   ceil(B / 1024) - 1 serial additions per thread over the B = ceil(n / 128) partials,
                      ceil(log2(min(B, 64))) butterfly levels, min(ceil(B / 64), 16) - 1 wave sums in order."""
    B = -(-n // (SPAN * TRAJ_SPANS))
    return ((1 if n > SPAN else 0) + _clog2(min(n, SPAN)) + max(-(-B // FINISH_THREADS) - 1, 0)
            + _clog2(min(B, 64)) + min(-(-B // 64), FINISH_THREADS // 64) - 1)


def moments_depth(d, n):
    """m of the moments' bound gamma_m sum |terms|: the term's own d roundings, then the tree."""
    return d + tree_depth(n)


def split(T, d):
    """(R [n, d, d], t [n, d]) of a d x (d+1) n trajectory, in its own dtype."""
    T = np.asarray(T)
    n = T.shape[1] // (d + 1)
    P = T.reshape(d, n, d + 1).transpose(1, 0, 2)
    return P[:, :, :d], P[:, :, d]


def join(R, t):
    """The d x (d+1) n trajectory of rotations R [n, d, d] and translations t [n, d]."""
    n, d = t.shape
    P = np.concatenate([np.asarray(R), np.asarray(t)[:, :, None]], axis=2)
    return np.ascontiguousarray(P.transpose(1, 0, 2).reshape(d, n * (d + 1)))


def _used(n, use):
    return np.ones(n, bool) if use is None else np.asarray(use) != 0


def moments(That, T, d, use=None, shift=None):
    """(mom, mom_abs) in np.longdouble: the moments and, entry by entry, the sum of the magnitudes of their terms."""
    _, th = split(np.asarray(That, np.float64), d)
    _, tt = split(np.asarray(T, np.float64), d)
    s = np.zeros(2 * d) if shift is None else np.asarray(shift, np.float64)
    u = _used(th.shape[0], use)
    a = (th[u] - s[:d]).astype(_L)  # the float64 subtraction, as the kernel rounds it
    b = (tt[u] - s[d:]).astype(_L)
    M = np.einsum("ji,jc->ic", b, a)
    Mabs = np.einsum("ji,jc->ic", np.abs(b), np.abs(a))
    na, nb = np.sum(a * a), np.sum(b * b)
    mom = np.concatenate([[_L(a.shape[0]), na, nb], a.sum(axis=0), b.sum(axis=0), M.T.ravel()]).astype(_L)
    mabs = np.concatenate([[_L(a.shape[0]), na, nb], np.abs(a).sum(axis=0), np.abs(b).sum(axis=0),
                           Mabs.T.ravel()]).astype(_L)
    return mom, mabs


def svd_jacobi(Cm):
    """(U, s, V) of a small square matrix in np.longdouble by one-sided Jacobi, s descending, C = U diag(s) V^T; a
    zero singular value's column of U is completed to an orthonormal basis."""
    W = np.array(Cm, dtype=_L)
    d = W.shape[0]
    V = np.eye(d, dtype=_L)
    for _ in range(100):
        rotated = False
        for p in range(d - 1):
            for q in range(p + 1, d):
                al, be, ga = W[:, p] @ W[:, p], W[:, q] @ W[:, q], W[:, p] @ W[:, q]
                if ga == 0 or abs(ga) <= _L(1e-21) * np.sqrt(al * be):
                    continue
                rotated = True
                zeta = (be - al) / (2 * ga)
                t = np.copysign(_L(1), zeta) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                for Mx in (W, V):
                    mp, mq = Mx[:, p].copy(), Mx[:, q].copy()
                    Mx[:, p], Mx[:, q] = c * mp - s * mq, s * mp + c * mq
        if not rotated:
            break
    sig = np.sqrt(np.sum(W * W, axis=0))
    order = np.argsort(-sig, kind="stable")
    W, V, sig = W[:, order], V[:, order], sig[order]
    U = np.zeros((d, d), dtype=_L)
    for i in range(d):
        if sig[i] > 0:
            U[:, i] = W[:, i] / sig[i]
    for i in range(d):
        if sig[i] > 0:
            continue
        best = None
        for k in range(d):
            v = np.zeros(d, dtype=_L)
            v[k] = 1
            for _ in range(2):
                for c in range(d):
                    if c < i or sig[c] > 0:
                        v = v - (U[:, c] @ v) * U[:, c]
            if best is None or v @ v > best @ best:
                best = v
        U[:, i] = best / np.sqrt(best @ best)
    return U, sig, V


def _det(A):
    A = np.asarray(A)
    if A.shape[0] == 2:
        return A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    return (A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0])
            + A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]))


def align_moments(d, mom, shift=None, rank_tol=1e-12):
    """(Aa [d x (d+1)], info) in np.longdouble from a moment vector: the definition at the head of this file."""
    mom = np.asarray(mom).astype(_L)
    s = np.zeros(2 * d, dtype=_L) if shift is None else np.asarray(shift).astype(_L)
    n = mom[0]
    sa, sb = mom[3:3 + d], mom[3 + d:3 + 2 * d]
    M = mom[3 + 2 * d:].reshape(d, d).T
    muh, mu = s[:d] + sa / n, s[d:] + sb / n
    Cm = M - np.outer(sb, sa) / n
    U, sig, V = svd_jacobi(Cm)
    sgn = _L(-1) if _det(U) * _det(V) < 0 else _L(1)
    f = np.ones(d, dtype=_L)
    f[-1] = sgn
    A = np.eye(d, dtype=_L) if not sig[0] > 0 else (U * f) @ V.T
    a = mu - A @ muh
    sigma = sig.copy()
    if sig[0] > 0:
        sigma[-1] *= sgn
    info = dict(count=float(n), sigma=sigma, rank=int(np.count_nonzero(sig > _L(rank_tol) * sig[0])), mu_hat=muh, mu=mu)
    return np.concatenate([A, a[:, None]], axis=1), info


def align(That, T, d, use=None):
    """The two-pass driver restated: the means from the zero-shift moments rounded to float64 (they are the second
    launch's shift), then the moments about them."""
    m0, _ = moments(That, T, d, use)
    shift = np.asarray(m0[3:3 + 2 * d] / m0[0], dtype=np.float64)
    m1, _ = moments(That, T, d, use, shift)
    return align_moments(d, m1, shift)


def errors(That, T, d, Aa=None, use=None):
    """dict(tra, rot, tra_bound, rot_bound) per pose in np.longdouble (NaN for an unused pose):
      |tra_sq - tra| <= sum_i (2 |rho_i| e_i + e_i^2) + gamma_{d+1} tra,  e_i = gamma_{d+2} (sum_k |A_ik t^_k| + |a_i| + |t_i|),
      |rot_sq - rot| <= sum_ic (2 |f_ic| e_ic + e_ic^2) + gamma_{d^2+1} rot,  e_ic = gamma_{d+1} (sum_k |A_ik R^_kc| + |R_ic|)."""
    Rh, th = split(np.asarray(That, np.float64).astype(_L), d)
    Rt, tt = split(np.asarray(T, np.float64).astype(_L), d)
    Aa = np.eye(d, d + 1) if Aa is None else np.asarray(Aa)
    A, a = Aa[:, :d].astype(_L), Aa[:, d].astype(_L)
    rho = np.einsum("ik,jk->ji", A, th) + a - tt
    e = _L(gamma(d + 2)) * (np.einsum("ik,jk->ji", np.abs(A), np.abs(th)) + np.abs(a) + np.abs(tt))
    tra = np.sum(rho * rho, axis=1)
    tra_bound = np.sum(2 * np.abs(rho) * e + e * e, axis=1) + _L(gamma(d + 1)) * tra
    F = np.einsum("ik,jkc->jic", A, Rh) - Rt
    eF = _L(gamma(d + 1)) * (np.einsum("ik,jkc->jic", np.abs(A), np.abs(Rh)) + np.abs(Rt))
    rot = np.sum(F * F, axis=(1, 2))
    rot_bound = np.sum(2 * np.abs(F) * eF + eF * eF, axis=(1, 2)) + _L(gamma(d * d + 1)) * rot
    out = dict(tra=tra, rot=rot, tra_bound=tra_bound, rot_bound=rot_bound)
    u = _used(th.shape[0], use)
    for v in out.values():
        v[~u] = np.nan
    return out


def sums(tra_sq, rot_sq, use=None):
    """(sums, sums_abs) in np.longdouble of per-pose arrays: [count, sum tra, sum rot, max tra, max rot] over the used
    poses (the maxima of nothing are 0, as the kernel's)."""
    u = _used(len(tra_sq), use)
    tr, ro = np.asarray(tra_sq)[u].astype(_L), np.asarray(rot_sq)[u].astype(_L)
    s = np.array([_L(tr.size), tr.sum(), ro.sum(), tr.max(initial=_L(0)), ro.max(initial=_L(0))], dtype=_L)
    sabs = np.array([_L(tr.size), np.abs(tr).sum(), np.abs(ro).sum(), 0, 0], dtype=_L)
    return s, sabs


def relative_poses(T, d, p1, p2):
    """(R [m, d, d], t [m, d], R_abs, t_abs) in np.longdouble: R_p1^T R_p2 and R_p1^T (t_p2 - t_p1) with the sums of
    the magnitudes of their terms (|t_p2| + |t_p1| under the product for t)."""
    Rt, tt = split(np.asarray(T, np.float64).astype(_L), d)
    p1, p2 = np.asarray(p1, np.int64), np.asarray(p2, np.int64)
    R1, R2 = Rt[p1], Rt[p2]
    R = np.einsum("eku,ekc->euc", R1, R2)
    Rabs = np.einsum("eku,ekc->euc", np.abs(R1), np.abs(R2))
    t = np.einsum("eku,ek->eu", R1, tt[p2] - tt[p1])
    tabs = np.einsum("eku,ek->eu", np.abs(R1), np.abs(tt[p2]) + np.abs(tt[p1]))
    return R, t, Rabs, tabs


def rot_angle(rot_sq):
    return 2 * np.arcsin(np.minimum(1.0, np.sqrt(np.asarray(rot_sq, dtype=np.float64) / 8.0)))


# ---------------------------------------------------------------------------------------- fixtures
def exp_so(d, w):
    """Exp of so(d): w a scalar angle (d = 2) or a rotation vector (d = 3)."""
    if d == 2:
        c, s = math.cos(float(w)), math.sin(float(w))
        return np.array([[c, -s], [s, c]])
    return np.array(O._rodrigues([float(x) for x in w]))


def random_rotations(rng, d, n):
    return np.stack([O.project_to_rotation(rng.standard_normal((d, d))) for _ in range(n)])


OFFSET = {2: np.array([1500.0, -900.0]), 3: np.array([1500.0, -900.0, 600.0])}


@functools.lru_cache(maxsize=None)
def fixture(d, n, noise=True, seed=5):
    """dict(T, That, A0, a0, use), read-only.  T: n random SE(d) poses, translations N(0, 10^2) about OFFSET (of order
    10^3, so centring matters).  That: the truth moved by the inverse of the rigid map (A0, a0) -- A0 t^ + a0 = t and
    A0 R^ = R without noise -- and, with noise, composed with per-pose noise of 0.05 rad and 0.1.  use: a mask that
    keeps about 70 % of the poses (pose 0 always)."""
    rng = np.random.default_rng(1000 * seed + 10 * n + d)
    R = random_rotations(rng, d, n)
    t = OFFSET[d] + 10.0 * rng.standard_normal((n, d))
    A0 = random_rotations(rng, d, 1)[0]
    a0 = 50.0 * rng.standard_normal(d) - OFFSET[d] / 2
    Rh, th = np.empty_like(R), np.empty_like(t)
    for j in range(n):
        Rn, tn = R[j], t[j]
        if noise:
            w = 0.05 * rng.standard_normal(1 if d == 2 else 3)
            Rn = R[j] @ exp_so(d, w[0] if d == 2 else w)
            tn = t[j] + 0.1 * rng.standard_normal(d)
        Rh[j] = A0.T @ Rn
        th[j] = A0.T @ (tn - a0)
    use = (rng.uniform(size=n) < 0.7).astype(np.int32)
    use[0] = 1
    out = dict(T=join(R, t), That=join(Rh, th), A0=A0, a0=a0, use=use)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edges(n, m, seed=9):
    """(p1, p2): m seeded edges between distinct poses of [0, n) (n >= 2), int32, read-only."""
    rng = np.random.default_rng(100000 * seed + 1000 * n + m)
    p1 = rng.integers(0, n, m)
    p2 = (p1 + 1 + rng.integers(0, n - 1, m)) % n
    p1, p2 = p1.astype(np.int32), p2.astype(np.int32)
    p1.setflags(write=False)
    p2.setflags(write=False)
    return p1, p2
