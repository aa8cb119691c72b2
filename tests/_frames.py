"""Ground for the robust multi-robot initialisation tests (test infrastructure, no test): numpy restatements of
robustSingleRotationAveraging (src/DPGO_utils.cpp:582-644 with RobustCost::weight for GNC_TLS,
src/DPGO_robust.cpp:49-61) and of initializeInGlobalFrame by computeRobustNeighborTransformTwoStage
(src/PGOAgent.cpp:250-331, 369-432) over odometry local trajectories, in np.longdouble, and the two corrupted
fixtures the host and GPU tests share.  tests/test_frames_reference.py asserts what the fixtures must satisfy."""
import functools
import gzip
import os

import numpy as np

from oracle import dpgo_oracle as O
from tests._common import GOLDEN

LD = np.longdouble
THRESHOLD = 2.0 * np.sqrt(2.0) * np.sin(0.25)  # angular2ChordalSO3(0.5)
W_TOL = 1e-8


def angular2chordal(rad):
    return 2.0 * np.sqrt(2.0) * np.sin(rad / 2.0)


def _inv_t(X):
    """X^-T and det X of a 2 x 2 or 3 x 3 longdouble matrix (cofactors)."""
    if X.shape[0] == 2:
        Cf = np.array([[X[1, 1], -X[1, 0]], [-X[0, 1], X[0, 0]]], dtype=LD)
        det = X[0, 0] * X[1, 1] - X[0, 1] * X[1, 0]
    else:
        Cf = np.array([np.cross(X[1], X[2]), np.cross(X[2], X[0]), np.cross(X[0], X[1])], dtype=LD)
        det = np.dot(X[0], Cf[0])
    return Cf / det, det


def project_so(M):
    """projectToRotationGroup (src/DPGO_utils.cpp:478-492) in longdouble.  det M > 0: the orthogonal polar factor by
    scaled Newton iterations X <- (g X + X^-T / g) / 2, which is the projection.  Otherwise (a reflection or a
    singular mean) the float64 SVD's U diag(1, .., -1) V^T, made orthogonal to longdouble by Newton-Schulz steps."""
    M = np.asarray(M, dtype=LD)
    d = M.shape[0]
    scale = np.abs(M).max()
    if scale > 0 and _inv_t(M / scale)[1] > 1e-6:
        X = M / scale
        for _ in range(100):
            Xit, _ = _inv_t(X)
            g = np.sqrt(np.sqrt((Xit * Xit).sum()) / np.sqrt((X * X).sum()))
            Xn = (g * X + Xit / g) / 2
            done = np.abs(Xn - X).max() <= LD(1e-18)
            X = Xn
            if done:
                break
        return X
    Q = O.project_to_rotation(M.astype(np.float64)).astype(LD)
    for _ in range(3):
        Q = Q @ (3 * np.eye(d, dtype=LD) - Q.T @ Q) / 2
    return Q


def rotation_average(Rs, kappa=None, threshold=THRESHOLD, max_iters=1000, mu_step=1.4):
    """(R_opt, weights, GNC iterations): the estimate is the one solved with the weights of the iteration before the
    final reweighting, as the reference returns it."""
    Rs = np.asarray(Rs, dtype=LD)
    n = Rs.shape[0]
    k = np.ones(n, dtype=LD) if kappa is None else np.asarray(kappa, dtype=LD)

    def solve(w):
        return project_so(np.tensordot(k * w, Rs, axes=1))

    def rsq(Ropt):
        return k * ((Ropt[None] - Rs) ** 2).sum(axis=(1, 2))

    w = np.ones(n, dtype=LD)
    Ropt = solve(w)
    c2 = LD(threshold) * LD(threshold)
    mu = min(c2 / (2 * rsq(Ropt).max() - c2), LD(1e-5))
    iters = 0
    if mu > 0:
        for it in range(max_iters):
            Ropt = solve(w)
            r = np.sqrt(rsq(Ropt))
            r2 = r * r
            upper, lower = (mu + 1) / mu * c2, mu / (mu + 1) * c2
            with np.errstate(divide="ignore", invalid="ignore"):
                mid = np.sqrt(c2 * mu * (mu + 1) / r2) - mu
            w = np.where(r2 >= upper, LD(0), np.where(r2 <= lower, LD(1), mid))
            iters = it + 1
            if np.all((w < W_TOL) | (w > 1 - W_TOL)):
                break
            mu = LD(mu_step) * mu
    return Ropt, w, iters


def local_index(aop, K):
    aop = np.asarray(aop)
    local = np.zeros(len(aop), np.int64)
    for a in range(K):
        idx = np.nonzero(aop == a)[0]
        local[idx] = np.arange(len(idx))
    return local


def odometry_local(d, p1, p2, R, t, aop, K):
    """Each agent's odometry (consecutive local indices) composed from its first pose = identity, through the
    oracle's odometry_initialization: T_local d x (d+1) n."""
    n, b = len(aop), d + 1
    local = local_index(aop, K)
    T = np.zeros((d, n * b))
    for a in range(K):
        idx = np.nonzero(np.asarray(aop) == a)[0]
        es = []
        for l in range(len(idx) - 1):
            hit = np.nonzero((p1 == idx[l]) & (p2 == idx[l + 1]))[0]
            assert len(hit) >= 1, (a, l)
            es.append(hit[0])
        es = np.asarray(es, np.int64)
        m = len(es)
        odo = O.Measurements(d, np.zeros(m, np.int64), np.zeros(m, np.int64), np.arange(m), np.arange(m) + 1,
                             R[es], t[es], np.ones(m), np.ones(m), np.ones(m), len(idx))
        Ta = O.odometry_initialization(d, len(idx), odo)
        for l, p in enumerate(idx):
            T[:, p * b:(p + 1) * b] = Ta[:, l * b:(l + 1) * b]
    assert np.array_equal(local, local_index(aop, K))
    return T


def two_stage_alignment(d, p1, p2, R, t, aop, K, T_local, threshold=THRESHOLD):
    """Breadth-first from the agent holding pose 0, neighbours ascending, each new agent against the single agent being
    dequeued: per shared closure the candidate frame W_A-pose T_local(A-pose)^-1 (computeNeighborTransform), rotations
    by rotation_average (unit kappa), translation = mean over the inlier candidates.  A pair without inliers is
    skipped.  Returns dict(frames K x d x (d+1), parent, candidates, inliers, edge_inlier, order, aligned)."""
    b = d + 1
    aop = np.asarray(aop)
    m = len(p1)
    Tl = np.asarray(T_local, dtype=LD)
    Rl = lambda p: Tl[:, p * b:p * b + d]
    tl = lambda p: Tl[:, p * b + d]
    FR = np.zeros((K, d, d), dtype=LD)
    Ft = np.zeros((K, d), dtype=LD)
    parent = -np.ones(K, np.int32)
    cand = np.zeros(K, np.int32)
    inl = np.zeros(K, np.int32)
    edge_inlier = np.full(m, 255, np.uint8)
    nbr = [set() for _ in range(K)]
    shared = [[] for _ in range(K)]
    for e in range(m):
        ai, aj = int(aop[p1[e]]), int(aop[p2[e]])
        if ai != aj:
            nbr[ai].add(aj)
            nbr[aj].add(ai)
            shared[ai].append(e)
            shared[aj].append(e)
    root = int(aop[0])
    FR[root] = np.eye(d)
    done = np.zeros(K, bool)
    done[root] = True
    order = [root]
    h = 0
    while h < len(order):
        P = order[h]
        h += 1
        for A in sorted(nbr[P]):
            if done[A]:
                continue
            es, cR, ct = [], [], []
            for e in shared[A]:
                i, j = int(p1[e]), int(p2[e])
                a_is_j = aop[j] == A
                other, mine = (i, j) if a_is_j else (j, i)
                if aop[other] != P:
                    continue
                Ro, to = FR[P] @ Rl(other), FR[P] @ tl(other) + Ft[P]
                Re, te = np.asarray(R[e], dtype=LD), np.asarray(t[e], dtype=LD)
                if a_is_j:  # W_j = W_i T_e
                    Rw, tw = Ro @ Re, to + Ro @ te
                else:  # W_i = W_j T_e^-1
                    Rw = Ro @ Re.T
                    tw = to - Rw @ te
                Fi = Rw @ Rl(mine).T
                es.append(e)
                cR.append(Fi)
                ct.append(tw - Fi @ tl(mine))
            if not es:
                continue
            cR, ct = np.asarray(cR, dtype=LD), np.asarray(ct, dtype=LD)
            Ropt, w, _ = rotation_average(cR, None, threshold)
            ok = w > 1 - W_TOL
            edge_inlier[np.asarray(es)] = ok.astype(np.uint8)
            if not ok.any():
                continue
            FR[A], Ft[A] = Ropt, ct[ok].sum(axis=0) / LD(ok.sum())
            parent[A], cand[A], inl[A] = P, len(es), int(ok.sum())
            done[A] = True
            order.append(A)
    frames = np.concatenate([FR, Ft[:, :, None]], axis=2).astype(np.float64)
    return dict(frames=frames, parent=parent, candidates=cand, inliers=inl, edge_inlier=edge_inlier, order=order,
                aligned=done)


def frame_distance(Fa, Fb):
    """(chordal distance of the rotations, Euclidean distance of the translations) of two d x (d+1) frames."""
    d = Fa.shape[0]
    return float(np.linalg.norm(Fa[:, :d] - Fb[:, :d])), float(np.linalg.norm(Fa[:, d] - Fb[:, d]))


def _random_rotation(rng, d):
    if d == 2:
        th = rng.uniform(-np.pi, np.pi)
        return np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return O.project_to_rotation(np.linalg.qr(rng.standard_normal((3, 3)))[0])


def corrupt(d, p1, p2, R, t, aop, K, seed, shared_frac=0.3, private_frac=0.1, threshold=THRESHOLD):
    """A seeded shared_frac of the shared loop closures replaced by outliers (rotation drawn until its chordal
    distance from the measured one exceeds 1.2 x threshold, the separation rule of tests/testUtils.cpp:100-105;
    translation + N(0, 5)) and private_frac of the private loop closures with translation + N(0, 5) as
    test_gpu_rbcd._grid_with_outliers.  Returns (R, t, shared_bad [m] bool, private_bad [m] bool)."""
    rng = np.random.default_rng(seed)
    aop = np.asarray(aop)
    local = local_index(aop, K)
    R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
    same = aop[p1] == aop[p2]
    shared = np.nonzero(~same)[0]
    private = np.nonzero(same & (local[p2] != local[p1] + 1))[0]
    sb = np.zeros(len(p1), bool)
    pb = np.zeros(len(p1), bool)
    for e in rng.choice(shared, size=max(1, int(shared_frac * len(shared))), replace=False):
        while True:
            Rn = _random_rotation(rng, d)
            if np.linalg.norm(Rn - R[e]) > 1.2 * threshold:
                break
        R[e] = Rn
        t[e] += rng.normal(0.0, 5.0, size=d)
        sb[e] = True
    if len(private):
        bad = rng.choice(private, size=max(1, int(private_frac * len(private))), replace=False)
        t[bad] += rng.normal(0.0, 5.0, size=(len(bad), d))
        pb[bad] = True
    return R, t, sb, pb


def _fixture(d, n, p1, p2, R, t, kappa, tau, starts, seed):
    K = len(starts)
    aop = (np.searchsorted(np.asarray(starts), np.arange(n), side="right") - 1).astype(np.int32)
    Rc, tc, sb, pb = corrupt(d, p1, p2, R, t, aop, K, seed)
    fx = dict(d=d, n=n, K=K, aop=aop, p1=p1, p2=p2, R=Rc, t=tc, R_clean=np.array(R), t_clean=np.array(t),
              kappa=np.array(kappa), tau=np.array(tau), shared_bad=sb, private_bad=pb)
    fx["T_local"] = odometry_local(d, p1, p2, Rc, tc, aop, K)  # odometry edges are never corrupted
    fx["robust"] = two_stage_alignment(d, p1, p2, Rc, tc, aop, K, fx["T_local"])
    fx["clean"] = two_stage_alignment(d, p1, p2, fx["R_clean"], fx["t_clean"], aop, K, fx["T_local"])
    for v in fx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def fixture3d():
    """grid3d(6) (216 poses; its chain p -> p + 1 is the odometry) in 4 contiguous agents of 54.  Measurement noise
    0.01 rad / 0.01: the odometry-composed local trajectories then drift by a few degrees over an agent, well
    inside the 30 degree threshold, as the averaging of the reference presumes."""
    g = O.grid3d(6, seed=5, rot_sigma=0.01, trans_sigma=0.01)
    return _fixture(3, g.num_poses, g.p1.astype(np.int64), g.p2.astype(np.int64), g.R, g.t, g.kappa, g.tau,
                    (0, 54, 108, 162), 11)


@functools.lru_cache(maxsize=None)
def fixture2d():
    """The 2D twin: CSAIL (1045 poses) in 4 contiguous ranges, the same corruption of its shared closures.  The
    ranges start at poses 0, 450, 850 and 975: CSAIL's 127 loop closures join few stretches of the trajectory (four
    equal ranges leave the first two with their one odometry edge in common), and with these every pair the
    breadth-first order uses shares at least 27."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "CSAIL.g2o")
        with gzip.open(os.path.join(GOLDEN, "CSAIL.g2o.gz"), "rb") as src, open(path, "wb") as dst:
            dst.write(src.read())
        g = O.read_g2o(path)
    return _fixture(2, g.num_poses, g.p1.astype(np.int64), g.p2.astype(np.int64), g.R, g.t, g.kappa, g.tau,
                    (0, 450, 850, 975), 12)


def graph_of(H, fx, clean=False):
    return H.Graph.from_arrays(fx["d"], fx["n"], fx["p1"], fx["p2"], fx["R_clean" if clean else "R"],
                               fx["t_clean" if clean else "t"], fx["kappa"], fx["tau"])


def host_lift(T, YLift, frames=None, frame_of=None):
    """YLift [F_R R_j | F_R t_j + F_t] per pose in longdouble, and the elementwise magnitude product
    |YLift| (|F_R| |T| + |F_t|) that the rounding bound multiplies."""
    T = np.asarray(T, dtype=LD)
    d = T.shape[0]
    b = d + 1
    n = T.shape[1] // b
    Y = np.asarray(YLift, dtype=LD)
    P = T.reshape(d, n, b).transpose(1, 0, 2)  # n x d x b
    if frames is None:
        W, Wa = P, np.abs(P)
    else:
        F = np.asarray(frames, dtype=LD)[np.asarray(frame_of)]
        W = F[:, :, :d] @ P
        Wa = np.abs(F[:, :, :d]) @ np.abs(P)
        W[:, :, d] += F[:, :, d]
        Wa[:, :, d] += np.abs(F[:, :, d])
    X = (Y[None] @ W).transpose(1, 0, 2).reshape(Y.shape[0], n * b)
    Xa = (np.abs(Y)[None] @ Wa).transpose(1, 0, 2).reshape(Y.shape[0], n * b)
    return X, Xa


def gamma(k):
    u = 2.0 ** -53
    return k * u / (1 - k * u)
