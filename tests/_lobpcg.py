"""The block certificate (dpgo_hip_certify_block) restated in numpy on a dense S (test infrastructure,
no GPU): the same start stream and the same locked block U as dpgo_amd/csrc/cert_host.cpp (cert_start, seed_block),
the same drop and refresh rules and the same lower bound as dpgo_amd/csrc/blockcert.cpp, with numpy's eigh where the
library runs its host Householder/QL solver (dpgo_amd/csrc/host_eig.cpp).  Vectors
are rows (V -> V S), as the lifted r x (d+1) n layout holds them.  The result's `iters` counts operator applications
the way the library's info.iters does; `iterations` counts the loop's turns.

model(key, ...) runs it once per process on a case of tests/_cholcert.py; complement(key) is the dense reference with
U: the seed block's exact quantities from numpy's SVD, QR and eigvalsh, built independently of seed_block."""
import functools

import numpy as np

from oracle import dpgo_oracle as O
from tests import _cholcert as CC

DROP_GRAM = 1e-14   # rows of W (and directions of B) below this share of the largest Gram eigenvalue are dropped
DROP_P = 1e-10      # lambda_min(B) < DROP_P lambda_max(B): this iteration runs without P
SEED_KEEP = 1e-6    # eigenvalues of X X^T kept for U, relative to the largest
SEED_DROP = 1e-10   # a seed whose remainder after two Gram-Schmidt passes is below this share of its norm is dropped


def start_block(rows, nc):
    """rows x nc block of the certificate's SplitMix64 stream (seed 0x5EED, uniform in [-1, 1)) in the lifted layout's
    memory order: entry (i, x) is the stream's element x * rows + i."""
    k = np.arange(1, rows * nc + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(0x5EED) + k * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = 2.0 * ((z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)) - 1.0
    return u.reshape(nc, rows).T.copy()


def seed_block(X, d):
    """U (nl x (d+1) n, orthonormal rows): the principal row directions of X and the translation gauge, classical
    Gram-Schmidt twice, as DPGO_CERT_SEED_X builds it."""
    w, Z = np.linalg.eigh(X @ X.T)
    cand = [Z[:, e] @ X for e in range(len(w) - 1, -1, -1) if w[e] >= SEED_KEEP * w[-1]]
    gauge = np.zeros(X.shape[1])
    gauge[d::d + 1] = 1.0
    cand.append(gauge)
    U = np.zeros((0, X.shape[1]))
    for v in cand:
        n0 = np.linalg.norm(v)
        for _ in range(2):
            v = v - (U @ v) @ U
        nv = np.linalg.norm(v)
        if not nv > SEED_DROP * n0:
            continue
        U = np.vstack([U, v / nv])
    return U


def block_jacobi_inverse(Q, n, b, shift=0.1):
    """Per pose the inverse of Q_jj + shift I (n x b x b): the handle's block-Jacobi preconditioner."""
    Qd = Q.toarray() if hasattr(Q, "toarray") else np.asarray(Q)
    return np.stack([np.linalg.inv(Qd[j * b:(j + 1) * b, j * b:(j + 1) * b] + shift * np.eye(b)) for j in range(n)])


def _orthonormal_coeffs(G):
    """T (m x m', m' <= m) with T^T G T = I for the Gram matrix G of m vectors, through the eigendecomposition of G;
    directions at or below DROP_GRAM of the largest eigenvalue are dropped (so a row far smaller than the largest
    one leaves the block instead of being scaled up from its rounding noise)."""
    e, Z = np.linalg.eigh(0.5 * (G + G.T))
    keep = e > DROP_GRAM * max(e[-1], 0.0)
    return Z[:, keep] / np.sqrt(e[keep])


def _orthonormalise(V):
    """Rows of V orthonormalised through their Gram matrix (_orthonormal_coeffs)."""
    return _orthonormal_coeffs(V @ V.T).T @ V


def _ritz(A, B):
    """Rayleigh-Ritz of the pencil (A, B) by whitening B: ascending theta and the coefficient columns C; also
    (lambda_min(B), lambda_max(B))."""
    w, V = np.linalg.eigh(0.5 * (B + B.T))
    keep = w > DROP_GRAM * w[-1]
    T = V[:, keep] / np.sqrt(w[keep])
    At = T.T @ A @ T
    th, Y = np.linalg.eigh(0.5 * (At + At.T))
    return th, T @ Y, (w[0], w[-1])


def lobpcg(S, U=None, block=None, max_iters=2000, tol=1e-8, refresh=50, minv=None):
    """The block certificate on the dense symmetric S.  U: locked orthonormal rows (None / empty: none); block: rows of
    the iterate; minv: (n, b, b) block-Jacobi inverses for precon = 1."""
    nc = S.shape[0]
    U = np.zeros((0, nc)) if U is None else U
    nl, k = U.shape[0], block
    assert 3 * k <= nc - nl

    def proj(V):
        return V - (V @ U.T) @ U if nl else V

    def precond(V):
        b = minv.shape[1]
        out = np.empty_like(V)
        for j in range(minv.shape[0]):
            out[:, j * b:(j + 1) * b] = V[:, j * b:(j + 1) * b] @ minv[j]
        return out

    passes = restarts = iterations = 0
    scale = 0.0

    def alone(X):
        """project, orthonormalise, a real operator pass and Rayleigh-Ritz of X by itself"""
        nonlocal passes, scale
        X = _orthonormalise(proj(X))
        assert X.shape[0] == k, "the iterate lost a row"
        SX = X @ S
        passes += 1
        th, C, _ = _ritz(X @ SX.T, X @ X.T)
        scale = max(scale, np.abs(th).max())
        return C.T @ X, C.T @ SX, th

    X, SX, theta = alone(start_block(k, nc))
    P = SP = np.zeros((0, nc))
    converged = False
    while iterations < max_iters:
        R = proj(SX - theta[:, None] * X)
        if np.linalg.norm(R[0]) <= tol * scale:
            converged = True
            break
        iterations += 1
        W = proj(precond(R)) if minv is not None else R
        W = W - (W @ X.T) @ X
        W = _orthonormalise(W)
        if W.shape[0] == 0:  # an invariant subspace up to rounding
            converged = True
            break
        # the second orthogonalisation runs after the rows were scaled up, against U too: a small row's rounding-level
        # components along U and X grow with it, and S has lower eigenvalues on U than on its complement
        W = proj(W)
        W = W - (W @ X.T) @ X
        SW = W @ S
        passes += 1
        Z, SZ = np.vstack([X, W, P]), np.vstack([SX, SW, SP])
        A, B = Z @ SZ.T, Z @ Z.T
        th, C, (bmin, bmax) = _ritz(A, B)
        m = k + W.shape[0]
        if P.shape[0] and bmin < DROP_P * bmax:
            restarts += 1
            Z, SZ = Z[:m], SZ[:m]
            A, B = A[:m, :m], B[:m, :m]
            th, C, _ = _ritz(A, B)
        scale = max(scale, np.abs(th).max())
        C = C[:, :k]
        theta = th[:k]
        Cp = C.copy()
        Cp[:k] = 0.0  # the W and P part of the new iterate
        Cp = Cp @ _orthonormal_coeffs(Cp.T @ B @ Cp)
        X, SX, P, SP = C.T @ Z, C.T @ SZ, Cp.T @ Z, Cp.T @ SZ
        if refresh > 0 and iterations % refresh == 0:
            X, SX, theta = alone(X)
    # finish: the lowest pair's true residuals from a fresh pass, then U's own block
    X, SX, theta = alone(X)
    Rf = SX - theta[:, None] * X
    residual = float(np.linalg.norm(Rf[0]))
    theta_c, res_c = float(theta[0]), float(np.linalg.norm(proj(Rf)[0]))
    lam, vec, lam_s, coupling = theta_c, X[0], float("nan"), 0.0
    if nl:
        SU = U @ S
        passes += -(-nl // k)
        As = SU @ U.T
        coupling = float(np.sqrt(np.maximum(np.sum(SU * SU, axis=1) - np.sum(As * As, axis=1), 0.0).sum()))
        ws, Zs = np.linalg.eigh(0.5 * (As + As.T))
        lam_s = float(ws[0])
        if lam_s < theta_c:
            lam, vec = lam_s, Zs[:, 0] @ U
            passes += 1
            residual = float(np.linalg.norm(vec @ S - lam * vec))
    cl = theta_c - res_c
    lower = 0.5 * (lam_s + cl) - np.sqrt(0.25 * (cl - lam_s) ** 2 + coupling ** 2) if nl else cl
    return dict(lambda_min=float(lam), lambda_complement=theta_c, residual=residual, residual_complement=res_c,
                lambda_seed=lam_s, coupling=coupling, lower_bound=float(lower), seeds=nl, iters=passes,
                iterations=iterations, restarts=restarts, converged=converged, vec=vec / np.linalg.norm(vec),
                ritz=theta.copy())


@functools.lru_cache(maxsize=None)
def model(key, seed_x, precon=False, block=None):
    """lobpcg's result on tests/_cholcert.case(key) with the library's defaults (max_iters 2000, tol 1e-8, refresh
    50); block None: r rows."""
    c = CC.case(key)
    U = seed_block(c.X, c.d) if seed_x else None
    minv = block_jacobi_inverse(O.connection_laplacian(c.meas, c.n), c.n, c.d + 1) if precon else None
    return lobpcg(c.S, U, block or c.r, minv=minv)


@functools.lru_cache(maxsize=None)
def complement(key):
    """The seed block's exact quantities on the dense S of the case, as tests/test_gpu_certify.py's _seed_blocks:
    U = X's principal row directions (singular values >= 1e-3 of the largest) and the translation gauge by numpy's
    SVD and QR; dict(seeds, lambda_seed = lambda_min(U^T S U), lambda_complement = the lowest eigenvalue of S on U's
    complement, coupling = |(I - U U^T) S U|_F)."""
    c = CC.case(key)
    Uc, sv, _ = np.linalg.svd(c.X.T, full_matrices=False)
    Uc = Uc[:, sv >= 1e-3 * sv[0]]
    gauge = np.zeros(c.X.shape[1])
    gauge[c.d::c.d + 1] = 1.0
    Uc, _ = np.linalg.qr(np.column_stack([Uc, gauge]))
    SU = c.S @ Uc
    Pm = np.eye(c.S.shape[0]) - Uc @ Uc.T
    # P S P has U as an extra null space: lift it above the spectrum, the lowest eigenvalue is the complement's
    M = Pm @ c.S @ Pm + (c.lam_max + 1.0) * (Uc @ Uc.T)
    return dict(seeds=Uc.shape[1], lambda_seed=float(np.linalg.eigvalsh(Uc.T @ SU)[0]),
                lambda_complement=float(np.linalg.eigvalsh(0.5 * (M + M.T))[0]),
                coupling=float(np.linalg.norm(SU - Uc @ (Uc.T @ SU))))
