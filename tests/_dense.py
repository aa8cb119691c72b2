"""Ground for the tests of the per-pose dense kernels on ill-conditioned and boundary inputs (test infrastructure, no
test): the QF retraction (qf_inplace), the polar projection (polar_fast / polar_inplace), the tangent projection and the
block-Jacobi inverse (gauss_jordan), each restated in np.longdouble (64-bit mantissa) independently of the oracle, and
the crafted batches the CPU and GPU tests share.  tests/test_dense_reference.py asserts what the references and the
batches must satisfy; tests/test_gpu_dense_edges.py runs the device kernels against them.

Every batch has N = 130 poses: tiles of 64, 64 and 2, i.e. the 16-byte vector path (even pose width), the scalar path
and a short tile.

The bars.  A result is compared per pose, in the maximum norm, with eps = 2^-52:
  polar            |P - polar_ref|  <= K_POLAR eps kappa_polar(sigma)
  QF               |Q - qf_ref|     <= K_QF eps cond_2(M)
  block-Jacobi     |Z - ref|        <= K_BJ eps cond_2(block_j) |V_j|_F |block_j^-1|_2
  tangent          |Z - ref|        <= 4 eps max|V_Y|       (absolute: almost all of V is removed)
K_* = 8 x the worst ratio error / (eps kappa) of the float64 oracle (numpy: LAPACK's SVD for O.lifted_project,
Householder QR for O.retract_qf, LU for np.linalg.inv) against the longdouble references on exactly these batches
(oracle_ratios() below, every compiled shape).  The device kernels sum in another order, contract to FMA and use other
algorithms (Newton-Schulz / one-sided Jacobi, Gram-Schmidt twice, Gauss-Jordan); 8 x leaves room for that, while a kernel
that loses half its digits misses the bar by orders of magnitude.  Measured oracle ratios and the bars:
  polar            21.7  (d = 3, r = 5, the clustered batch)       ORACLE_POLAR = 22     K_POLAR = 176
  QF               3.41  (d = 2, r = 4, retraction at s = 1e8)     ORACLE_QF = 3.5       K_QF = 28
  block-Jacobi     0.386 (d = 2, the pose without edges)           ORACLE_BJ = 0.39      K_BJ = 3.12
(Polar by batch: 21.7 clustered, 10.7 graded and its 2^+-100 copies, <= 3.8 everywhere else; LAPACK's singular vectors of
a cluster are individually ill-determined, their product is not.)  On an MI355X the kernels reach at most 0.066 of the
polar bar (ratio 11.7, just above the switch, where Jacobi runs all its sweeps), 0.046 in polar_combine_dev, 0.042 of the
QF bar, 0.097 of the block-Jacobi bar and 0.28 of the tangent bar; |Q^T Q - I| stays below 1e-14 throughout.
"""
import functools

import numpy as np

from tests._extended import gauss_jordan_inverse

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
N = 130
NAN_POSES = (5, 129)  # one pose of a full tile, one of the short tile
SHAPES = [(2, r) for r in range(2, 9)] + [(3, r) for r in range(3, 9)]  # every compiled (d, r)
CORE = [(2, 2), (2, 3), (2, 4), (3, 3), (3, 5), (3, 8)]  # r = d and r > d, odd and even pose width r (d + 1)

# measured worst oracle ratios (oracle_ratios(), rounded up) and the bars: 8 x
ORACLE_POLAR, ORACLE_QF, ORACLE_BJ = 22.0, 3.5, 0.39
K_POLAR, K_QF, K_BJ = 8 * ORACLE_POLAR, 8 * ORACLE_QF, 8 * ORACLE_BJ
ORTHO_BAR = 1e-14  # |Q^T Q - I|_max of any result, whatever the conditioning
TANGENT_K = 4.0


# ----------------------------------------------------------------------------------------------------------- layout
def to_poses(X, d):
    """r x (d+1) n -> (n, r, d+1) pose blocks (a view)."""
    r = X.shape[0]
    return X.reshape(r, -1, d + 1).transpose(1, 0, 2)


def from_poses(P):
    n, r, b = P.shape
    return np.ascontiguousarray(P.transpose(1, 0, 2).reshape(r, n * b))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------------------------------------------- references
def qf_ref(M):
    """Thin Q (positive diagonal R) of the full-rank (..., r, d) matrices M: Gram-Schmidt, three passes, longdouble."""
    Q = np.array(M, dtype=LD)
    for c in range(Q.shape[-1]):
        v = Q[..., :, c].copy()
        for _ in range(3):
            for k in range(c):
                v = v - (Q[..., :, k] * v).sum(-1, keepdims=True) * Q[..., :, k]
        Q[..., :, c] = v / np.sqrt((v * v).sum(-1, keepdims=True))
    return Q


def _inv_t(X):
    """X^-T of (..., d, d) longdouble matrices, d = 2 or 3, by cofactors (tests/_frames._inv_t, batched)."""
    if X.shape[-1] == 2:
        Cf = np.stack([np.stack([X[..., 1, 1], -X[..., 1, 0]], -1), np.stack([-X[..., 0, 1], X[..., 0, 0]], -1)], -2)
        det = X[..., 0, 0] * X[..., 1, 1] - X[..., 0, 1] * X[..., 1, 0]
    else:
        r0, r1, r2 = X[..., 0, :], X[..., 1, :], X[..., 2, :]
        Cf = np.stack([np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)], -2)
        det = (r0 * Cf[..., 0, :]).sum(-1)
    return Cf / det[..., None, None]


def polar_ref(M):
    """Polar factor U V^T of the full-rank (..., r, d) matrices M in longdouble: Q = qf_ref(M), the orthogonal polar
    factor of the d x d matrix Q^T M by scaled Newton X <- (g X + X^-T / g) / 2, and their product.  Each matrix is
    scaled by a power of two first (exact), so 2^+-100 inputs take the same path."""
    M = np.asarray(M, dtype=LD)
    _, e = np.frexp(np.abs(M).max(axis=(-2, -1)).astype(np.float64))
    Ms = M * np.ldexp(LD(1), -e)[..., None, None]
    Q = qf_ref(Ms)
    X = np.swapaxes(Q, -1, -2) @ Ms
    nf = lambda A: np.sqrt((A * A).sum(axis=(-2, -1)))  # noqa: E731
    for _ in range(100):
        Xit = _inv_t(X)
        g = np.sqrt(nf(Xit) / nf(X))[..., None, None]
        Xn = (g * X + Xit / g) / 2
        done = np.abs(Xn - X).max() <= LD(1e-18)
        X = Xn
        if done:
            return Q @ X
    raise AssertionError("polar_ref: the scaled Newton iteration did not settle")


def tangent_ref(X, V, d):
    """P_X(V) = [V_Y - Y sym(Y^T V_Y) | V_p] per pose, in longdouble."""
    Xp, Vp = to_poses(np.asarray(X, LD), d), to_poses(np.asarray(V, LD), d).copy()
    Y, VY = Xp[:, :, :d], Vp[:, :, :d]
    S = np.swapaxes(Y, 1, 2) @ VY
    Vp[:, :, :d] = VY - Y @ ((S + np.swapaxes(S, 1, 2)) / 2)
    return from_poses(Vp)


def bj_inverse_ref(block):
    """(block)^-1 by Gauss-Jordan with pivoting in longdouble (the code rtr_extended uses)."""
    return gauss_jordan_inverse(block)


def kappa_polar(sigmas, r, d):
    """Condition number of the polar factor at singular values sigmas: sigma_max / sigma_min for r > d, and
    2 sigma_max / (sigma_{d-1} + sigma_d), the two smallest, for the square case."""
    s = np.sort(np.asarray(sigmas, dtype=np.float64))[::-1]
    return float(s[0] / s[-1]) if r > d else float(2.0 * s[0] / (s[-2] + s[-1]))


# --------------------------------------------------------------------------------------------------------- builders
def _gauss(rng, *shape):
    return rng.standard_normal(shape).astype(LD)


def with_singular_values(r, d, sigmas, rng, n=None):
    """U diag(sigmas) W^T with U (r x d) and W (d x d) orthonormal to longdouble (qf_ref of Gaussians), rounded to
    float64; n: a batch (n, r, d)."""
    lead = () if n is None else (n,)
    U, W = qf_ref(_gauss(rng, *lead, r, d)), qf_ref(_gauss(rng, *lead, d, d))
    return ((U * np.asarray(sigmas, dtype=LD)) @ np.swapaxes(W, -1, -2)).astype(np.float64)


def _sigmas(d, s3):
    """The batch's singular values at d = 3; at d = 2 the largest and the smallest of them."""
    return tuple(s3) if d == 3 else (s3[0], s3[-1])


def _switch_sigma(d, sign_err, above_one):
    """The sigma of sigma * (orthonormal) whose Newton-Schulz test value |Y^T Y - I|_F^2 = d (sigma^2 - 1)^2 is
    0.5 (1 + sign_err 1e-9): just below (sign_err = -1) or just above the switch, with sigma below or above 1."""
    e = LD(0.5) * (1 + LD(sign_err) * LD(1e-9))
    return float(np.sqrt(1 + (1 if above_one else -1) * np.sqrt(e / d)))


def polar_batch_specs(d):
    """name -> (singular values, scale exponent, branch): branch 'below' = Newton-Schulz (first test value < 0.5),
    'above' = the Jacobi fallback."""
    one = (1.0,) * d
    eq = lambda s: (s,) * d  # noqa: E731
    return {
        "manifold": (one, 0, "below"),
        "below_lt1": (eq(_switch_sigma(d, -1, False)), 0, "below"),
        "below_gt1": (eq(_switch_sigma(d, -1, True)), 0, "below"),
        "above_lt1": (eq(_switch_sigma(d, +1, False)), 0, "above"),
        "above_gt1": (eq(_switch_sigma(d, +1, True)), 0, "above"),
        "small_1e-3": (_sigmas(d, (1.0, 0.5, 1e-3)), 0, "above"),
        "small_1e-6": (_sigmas(d, (1.0, 0.5, 1e-6)), 0, "above"),
        "small_1e-9": (_sigmas(d, (1.0, 1.0, 1e-9)), 0, "above"),
        "clustered": (_sigmas(d, (1.0, 1.0 - 1e-9, 1.0 - 2e-9)), 0, "below"),
        "graded": (_sigmas(d, (1.0, 0.7, 0.4)), 0, "above"),
        "graded_2^+100": (_sigmas(d, (1.0, 0.7, 0.4)), 100, "above"),
        "graded_2^-100": (_sigmas(d, (1.0, 0.7, 0.4)), -100, "above"),
    }


POLAR_BATCHES = tuple(polar_batch_specs(3))


@functools.lru_cache(maxsize=None)
def polar_batch(d, r, name):
    """(M r x (d+1) N float64, singular values, branch) of one batch; the translation columns are Gaussian (scaled
    with the batch).  The graded batches at 2^+-100 are the graded batch times that power, exactly."""
    sig, expo, branch = polar_batch_specs(d)[name]
    tag = POLAR_BATCHES.index("graded" if expo else name)
    rng = np.random.default_rng([d, r, tag])
    P = np.empty((N, r, d + 1))
    if name == "manifold":
        P[:, :, :d] = polar_ref(_gauss(rng, N, r, d)).astype(np.float64)
    else:
        P[:, :, :d] = with_singular_values(r, d, sig, rng, N)
    P[:, :, d] = rng.standard_normal((N, r))
    return _frozen(from_poses(np.ldexp(P, expo))), sig, branch


def ns_test_value(M, d):
    """polar_fast's first-iteration test value |Y^T Y - I|_F^2 per pose, in float64 as the kernel forms it."""
    Y = to_poses(np.asarray(M, np.float64), d)[:, :, :d]
    E = np.swapaxes(Y, 1, 2) @ Y - np.eye(d)
    return (E * E).sum(axis=(1, 2))


def polar_reference(M, d):
    """polar_ref on the rotation columns of M (r x (d+1) n), the translation columns kept: longdouble."""
    P = to_poses(np.asarray(M, LD), d).copy()
    P[:, :, :d] = polar_ref(P[:, :, :d])
    return from_poses(P)


@functools.lru_cache(maxsize=None)
def manifold_point(d, r, seed=0):
    """X (r x (d+1) N float64) on the manifold: polar_ref of Gaussians, rounded."""
    rng = np.random.default_rng([d, r, 100 + seed])
    P = _gauss(rng, N, r, d + 1)
    P[:, :, :d] = polar_ref(P[:, :, :d])
    return _frozen(from_poses(P.astype(np.float64)))


QF_SCALES = (1.0, 1e2, 1e4, 1e6, 1e8)
LIFT_ALPHAS = (1.0, 1e4)


@functools.lru_cache(maxsize=None)
def qf_batch(d, r):
    """(X, V): X on the manifold, V = X Omega per pose with Omega skew (rank 2 at d = 3, so X + s V loses a direction
    as s grows) and no translation part; on the odd poses, where r > d leaves a normal space, 1e-3 of a unit normal
    component is added, so the loss is partial.  Every pose of V has unit Frobenius norm."""
    X = manifold_point(d, r)
    rng = np.random.default_rng([d, r, 200])
    Y = to_poses(X, d)[:, :, :d].astype(LD)
    G = _gauss(rng, N, d, d)
    VY = Y @ (G - np.swapaxes(G, 1, 2))
    VY /= np.sqrt((VY * VY).sum(axis=(1, 2)))[:, None, None]
    if r > d:
        Nn = _gauss(rng, N, r, d)
        Nn = Nn - Y @ (np.swapaxes(Y, 1, 2) @ Nn)
        Nn /= np.sqrt((Nn * Nn).sum(axis=(1, 2)))[:, None, None]
        VY[1::2] += LD(1e-3) * Nn[1::2]
        VY /= np.sqrt((VY * VY).sum(axis=(1, 2)))[:, None, None]
    V = np.zeros((N, r, d + 1))
    V[:, :, :d] = VY.astype(np.float64)
    return X, _frozen(from_poses(V))


def qf_reference(X, V, s, d):
    """(reference r x (d+1) N longdouble, cond_2 per pose of the float64 X_Y + s V_Y, M_Y longdouble (N, r, d))."""
    P = to_poses(np.asarray(X, LD) + LD(s) * np.asarray(V, LD), d).copy()
    MY = P[:, :, :d].copy()
    P[:, :, :d] = qf_ref(MY)
    return from_poses(P), np.linalg.cond(MY.astype(np.float64)), MY


@functools.lru_cache(maxsize=None)
def lift_batch(d, r):
    """(X, v) for the rank r + 1 QF of [Y_j; alpha v_Y^T]: X of qf_batch and, per pose, v_Y = the first row of its V
    at unit length with a Gaussian v_p ((d+1) N vector)."""
    X, V = qf_batch(d, r)
    rng = np.random.default_rng([d, r, 300])
    v = to_poses(V, d)[:, 0, :].copy()
    v[:, :d] /= np.linalg.norm(v[:, :d], axis=1)[:, None]
    v[:, d] = rng.standard_normal(N)
    return X, _frozen(v.ravel())


def lift_reference(X, v, alpha, d):
    """(reference (r+1) x (d+1) N longdouble, cond_2 per pose, M_Y longdouble) of [qf([Y; alpha v_Y^T]) | (p; alpha v_p)]
    with alpha v rounded to float64 first, as the kernel's translation entries are."""
    av = (alpha * np.asarray(v, np.float64)).reshape(-1, 1, d + 1)
    P = np.concatenate([to_poses(np.asarray(X, LD), d), av.astype(LD)], axis=1)
    MY = P[:, :, :d].copy()
    P[:, :, :d] = qf_ref(MY)
    return from_poses(P), np.linalg.cond(MY.astype(np.float64)), MY


@functools.lru_cache(maxsize=None)
def tangent_batch(d, r):
    """(X, V): V = 1e8 X + t with t tangent at X of unit Frobenius norm per pose: almost all of V_Y is removed."""
    X = manifold_point(d, r)
    rng = np.random.default_rng([d, r, 400])
    T = to_poses(tangent_ref(X, _gauss(rng, *X.shape), d), d).copy()
    T /= np.sqrt((T * T).sum(axis=(1, 2)))[:, None, None]
    return X, _frozen((LD(1e8) * X.astype(LD) + from_poses(T)).astype(np.float64))


# ----------------------------------------------------------------------------------------------------- block-Jacobi
BJ_ISOLATED, BJ_P2_ONLY = 37, 101
BJ_SHIFT = 0.1


@functools.lru_cache(maxsize=None)
def bj_graph(d):
    """N poses; kappa and tau log-uniform in [1e-3, 1e5] independently, |t| log-uniform in [0.1, 100].  A chain over all
    poses but BJ_ISOLATED (no edge at all: block 0.1 I) and BJ_P2_ONLY (the second endpoint of its three edges only:
    a diagonal block), plus 80 further edges."""
    rng = np.random.default_rng([d, 500])
    order = np.array([j for j in range(N) if j not in (BJ_ISOLATED, BJ_P2_ONLY)])
    extra = np.array([rng.choice(order, 2, replace=False) for _ in range(80)])
    p1 = np.concatenate([order[:-1], extra[:, 0], rng.choice(order, 3, replace=False)])
    p2 = np.concatenate([order[1:], extra[:, 1], [BJ_P2_ONLY] * 3])
    m = len(p1)
    R = polar_ref(_gauss(rng, m, d, d))
    R[:, :, -1] *= np.sign(np.linalg.det(R.astype(np.float64)))[:, None]
    t = rng.standard_normal((m, d))
    t *= (10.0 ** rng.uniform(-1, 2, m) / np.linalg.norm(t, axis=1))[:, None]
    g = dict(d=d, p1=p1.astype(np.int32), p2=p2.astype(np.int32), R=R.astype(np.float64), t=t,
             kappa=10.0 ** rng.uniform(-3, 5, m), tau=10.0 ** rng.uniform(-3, 5, m))
    _frozen(*[v for v in g.values() if isinstance(v, np.ndarray)])
    return g


@functools.lru_cache(maxsize=None)
def bj_blocks(d):
    """Q_jj + 0.1 I per pose (N, d+1, d+1), summed edge by edge in longdouble from the float64 measurements:
    Q_ii += T Om T^T, Q_jj += Om with T = [R t; 0 1], Om = diag(kappa, .., kappa, tau)."""
    g = bj_graph(d)
    b = d + 1
    A = np.zeros((N, b, b), LD)
    for e in range(len(g["p1"])):
        T = np.eye(b, dtype=LD)
        T[:d, :d], T[:d, d] = g["R"][e], g["t"][e]
        om = np.array([g["kappa"][e]] * d + [g["tau"][e]], LD)
        A[g["p1"][e]] += (T * om) @ T.T
        A[g["p2"][e]] += np.diag(om)
    return _frozen(A + LD(BJ_SHIFT) * np.eye(b, dtype=LD))


@functools.lru_cache(maxsize=None)
def bj_reference(d, r):
    """(X, V, P_X(V Minv) longdouble, bar per pose / K_BJ): X on the manifold, V Gaussian, Minv = bj_inverse_ref of
    bj_blocks; the bar's factor eps cond_2(block_j) |V_j|_F |Minv_j|_2."""
    X = manifold_point(d, r, seed=1)
    V = np.random.default_rng([d, r, 600]).standard_normal(X.shape)
    A = bj_blocks(d)
    Minv = np.stack([bj_inverse_ref(A[j]) for j in range(N)])
    ref = tangent_ref(X, from_poses(to_poses(V.astype(LD), d) @ Minv), d)
    A64 = A.astype(np.float64)
    unit = EPS * np.linalg.cond(A64) * np.linalg.norm(to_poses(V, d), axis=(1, 2)) * \
        np.linalg.norm(Minv.astype(np.float64), 2, axis=(1, 2))
    return X, _frozen(V), _frozen(ref), _frozen(unit)


def bj_measurements(d):
    """The graph as the oracle's Measurements (unit weights)."""
    from oracle import dpgo_oracle as O
    g = bj_graph(d)
    z = np.zeros(len(g["p1"]), np.int64)
    return O.Measurements(d, z, z, g["p1"], g["p2"], g["R"], g["t"], g["kappa"], g["tau"], np.ones(len(z)), N)


# ----------------------------------------------------------------------------------------------------------- errors
def pose_max(got, ref, d):
    """max |got - ref| per pose (N,), the difference taken in longdouble."""
    return np.abs(to_poses(np.asarray(got, LD) - np.asarray(ref, LD), d)).max(axis=(1, 2)).astype(np.float64)


def ortho_defect(X, d):
    """|Y^T Y - I|_max per pose."""
    Y = to_poses(np.asarray(X, LD), d)[:, :, :d]
    return np.abs(np.swapaxes(Y, 1, 2) @ Y - np.eye(d, dtype=LD)).max(axis=(1, 2)).astype(np.float64)


def oracle_ratios(shapes=SHAPES):
    """The worst ratio error / (eps kappa) of the float64 oracle against the references, over the batches:
    {'polar': (ratio, where), 'qf': .., 'bj': ..} (the figures the bars are 8 x of)."""
    from oracle import dpgo_oracle as O
    worst = {"polar": (0.0, None), "qf": (0.0, None), "bj": (0.0, None)}

    def note(key, ratios, where):
        j = int(np.argmax(ratios))
        if ratios[j] > worst[key][0]:
            worst[key] = (float(ratios[j]), where + (j,))

    for d, r in shapes:
        for name in POLAR_BATCHES:
            M, sig, _ = polar_batch(d, r, name)
            note("polar", pose_max(O.lifted_project(M, d), polar_reference(M, d), d) / (EPS * kappa_polar(sig, r, d)),
                 (d, r, name))
        X, V = qf_batch(d, r)
        for s in QF_SCALES:
            ref, cond, _ = qf_reference(X, V, s, d)
            note("qf", pose_max(O.retract_qf(X, s * V, d), ref, d) / (EPS * cond), (d, r, "retract", s))
        if (d, r + 1) in SHAPES:
            X, v = lift_batch(d, r)
            for alpha in LIFT_ALPHAS:
                ref, cond, _ = lift_reference(X, v, alpha, d)
                Xl = np.vstack([X, np.zeros((1, X.shape[1]))])
                D = np.zeros_like(Xl)
                D[-1] = alpha * v
                note("qf", pose_max(O.retract_qf(Xl, D, d), ref, d) / (EPS * cond), (d, r, "lift", alpha))
    for d in (2, 3):
        r = d + 2
        X, V, ref, unit = bj_reference(d, r)
        Q = O.connection_laplacian(bj_measurements(d), N)
        b = d + 1
        blocks = np.stack([Q[j * b:(j + 1) * b, j * b:(j + 1) * b].toarray() for j in range(N)]) + BJ_SHIFT * np.eye(b)
        Z = O.tangent_project(X, from_poses(to_poses(V, d) @ np.linalg.inv(blocks)), d)
        note("bj", pose_max(Z, ref, d) / unit, (d, r))
    return worst


# ---------------------------------------------------------------------------------------------- per-agent combination
COMBINE_AGENTS = (64, 1, 70, 129)  # a full tile, one pose, a full tile and a short one, two full tiles and one pose
COMBINE_CA = (0.9, 1.0, 0.3, -1.25)  # distinct per agent, and so are the ratios cb / ca
COMBINE_CB = (0.1, 2.5, 0.7, 0.05)


@functools.lru_cache(maxsize=None)
def combine_batch(d, r):
    """(A, B) over sum(COMBINE_AGENTS) poses: A with singular values (1, 0.95, 0.9) and Gaussian translations, B
    0.2 x Gaussian; with the coefficients above some agents start Newton-Schulz and the others go to Jacobi."""
    n = sum(COMBINE_AGENTS)
    rng = np.random.default_rng([d, r, 700])
    P = rng.standard_normal((n, r, d + 1))
    P[:, :, :d] = with_singular_values(r, d, _sigmas(d, (1.0, 0.95, 0.9)), rng, n)
    return _frozen(from_poses(P), from_poses(0.2 * rng.standard_normal((n, r, d + 1))))


def combine_exact(A, B, d):
    """comb_xv per agent, exactly as the kernel rounds it: fl(ca A) when B is None, else fma(cb, B, fl(ca A)) -- the
    sum formed exactly in rational arithmetic and rounded once."""
    from fractions import Fraction
    width = np.asarray(COMBINE_AGENTS) * (d + 1)
    ca = np.repeat(np.asarray(COMBINE_CA), width)[None, :]
    prod = ca * A
    if B is None:
        return prod
    cb = np.repeat(np.asarray(COMBINE_CB), width)[None, :] * np.ones_like(B)
    out = np.array([float(Fraction(c) * Fraction(v) + Fraction(p))
                    for c, v, p in zip(cb.ravel().tolist(), B.ravel().tolist(), prod.ravel().tolist())])
    return out.reshape(A.shape)


def kappa_polar_of(M, d):
    """kappa_polar per pose from the float64 singular values of M's rotation columns."""
    r = M.shape[0]
    S = np.linalg.svd(to_poses(np.asarray(M, np.float64), d)[:, :, :d], compute_uv=False)
    return np.array([kappa_polar(s, r, d) for s in S])
