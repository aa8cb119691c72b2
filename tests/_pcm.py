"""Ground for the pairwise consistency (PCM) tests (test infrastructure, no test): np.longdouble restatements of the
pair test of include/dpgo_hip.h (e_rot, e_tra, A), a plain Bron-Kerbosch maximum clique for small graphs, a generator
of candidate groups with planted inliers and three kinds of outliers, the candidate frames of dpgo_graph_pcm and of
the single-parent alignment, and the corrupted fixtures the host and GPU tests share.
tests/test_pcm_reference.py asserts what those fixtures must satisfy."""
import functools

import numpy as np

from oracle import dpgo_oracle as O
from tests import _frames as F

LD = np.longdouble
C_R = F.THRESHOLD  # the library's default max_rotation_error
GROUP_SIZES = (0, 1, 2, 63, 64, 65, 130)  # one call: empty, single, pair, and both sides of one and two words
MARGIN = 1e-9  # no e within this relative distance of its threshold (test_pcm_reference)


# ---------------------------------------------------------------------------------------- the pair test
def pair_errors(Fk, xk):
    """(e_rot, e_tra) [m, m] in longdouble of one group: Fk [m, d, d + 1] frames, xk [m, d] lever points.
    e_rot(k,l) = |R_k - R_l|_F^2, e_tra(k,l) = 1/2 (|dR x_k + dt|^2 + |dR x_l + dt|^2)."""
    Fk = np.asarray(Fk, dtype=LD)
    xk = np.asarray(xk, dtype=LD)
    m, d = xk.shape
    R, t = Fk[:, :, :d], Fk[:, :, d]
    dR = R[:, None] - R[None, :]  # [k, l, d, d]
    dt = t[:, None] - t[None, :]
    e_rot = (dR * dR).sum(axis=(2, 3))
    vk = np.einsum("kluc,kc->klu", dR, xk) + dt
    vl = np.einsum("kluc,lc->klu", dR, xk) + dt
    e_tra = ((vk * vk).sum(axis=2) + (vl * vl).sum(axis=2)) / 2
    return e_rot, e_tra


def adjacency(Fk, xk, c_R, c_t):
    """A [m, m] bool: k != l, e_rot <= c_R^2 and e_tra <= c_t^2; any NaN gives False."""
    m = len(xk)
    if m == 0:
        return np.zeros((0, 0), bool)
    e_rot, e_tra = pair_errors(Fk, xk)
    with np.errstate(invalid="ignore"):
        A = (e_rot <= LD(c_R) * LD(c_R)) & (e_tra <= LD(c_t) * LD(c_t))
    A[np.arange(m), np.arange(m)] = False
    return A


def threshold_margin(Fk, xk, c_R, c_t):
    """The smallest relative distance of any off-diagonal e from its threshold (inf for fewer than two candidates)."""
    m = len(xk)
    if m < 2:
        return np.inf
    e_rot, e_tra = pair_errors(Fk, xk)
    off = ~np.eye(m, dtype=bool)
    cr2, ct2 = LD(c_R) ** 2, LD(c_t) ** 2
    return float(min(np.abs(e_rot[off] / cr2 - 1).min(), np.abs(e_tra[off] / ct2 - 1).min()))


def flat_frames(Fk):
    """[m, d, d + 1] frames as the library's column-major records [m, d (d + 1)]."""
    Fk = np.asarray(Fk, dtype=np.float64)
    return np.ascontiguousarray(Fk.transpose(0, 2, 1)).reshape(Fk.shape[0], -1)


# ---------------------------------------------------------------------------------------- maximum clique
def bron_kerbosch(A):
    """All maximum cliques of the graph with bool adjacency A (pivoting Bron-Kerbosch): a list of sorted tuples."""
    n = A.shape[0]
    nb = [set(np.nonzero(A[v])[0].tolist()) for v in range(n)]
    best = [0, []]

    def rec(Rs, P, X):
        if not P and not X:
            if len(Rs) > best[0]:
                best[0], best[1] = len(Rs), [tuple(sorted(Rs))]
            elif len(Rs) == best[0]:
                best[1].append(tuple(sorted(Rs)))
            return
        if len(Rs) + len(P) < best[0]:
            return
        u = max(P | X, key=lambda v: len(P & nb[v]))
        for v in sorted(P - nb[u]):
            rec(Rs | {v}, P & nb[v], X & nb[v])
            P = P - {v}
            X = X | {v}

    rec(set(), set(range(n)), set())
    if n == 0:
        return [()]
    return sorted(set(best[1]))


def is_clique(A, members):
    members = list(members)
    return all(A[u, v] for i, u in enumerate(members) for v in members[i + 1:])


def greedy_clique(A):
    """The documented budget-0 clique: vertices by descending degree, ties to the lower index, each kept when it is
    adjacent to all kept so far."""
    deg = A.sum(axis=1)
    kept = []
    for v in sorted(range(A.shape[0]), key=lambda v: (-deg[v], v)):
        if all(A[v, u] for u in kept):
            kept.append(v)
    return sorted(kept)


def random_graph(rng, n, density):
    U = np.triu(rng.random((n, n)) < density, 1)
    return U | U.T


def clique_cases():
    """200 seeded random graphs of 8-40 vertices at densities 0.1-0.9."""
    rng = np.random.default_rng(2024)
    return [random_graph(rng, int(rng.integers(8, 41)), float(rng.uniform(0.1, 0.9))) for _ in range(200)]


def planted_clique_graph():
    """200 vertices at density 0.3 with a clique planted on 30 seeded vertices (a G(200, 0.3) has none above ~9)."""
    rng = np.random.default_rng(77)
    A = random_graph(rng, 200, 0.3)
    members = np.sort(rng.choice(200, size=30, replace=False))
    A[np.ix_(members, members)] = True
    A[members, members] = False
    return A, members


# ---------------------------------------------------------------------------------------- candidate groups
def _small_rotation(rng, d, noise):
    if d == 2:
        a = rng.uniform(-noise, noise)
        return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    v = rng.standard_normal(3)
    v *= rng.uniform(0, noise) / np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    th = np.linalg.norm(v)
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * K @ K if th > 0 else np.eye(3)


C_T = 1.0  # the generated groups' translation threshold


def far_offset(rng, d, c_t):
    """N(0, 5) per component, drawn until its length exceeds 2.5 c_t: the rotation outliers' separation rule
    (tests/testUtils.cpp:100-105: redraw until 1.2 x the threshold away) for translations.  An inlier and an outlier
    then disagree by at least 2.5 c_t less the inliers' own spread, which the fixtures keep below c_t."""
    while True:
        v = rng.normal(0.0, 5.0, size=d)
        if np.linalg.norm(v) > 2.5 * c_t:
            return v


def make_group(d, m, n_in, seed):
    """m candidates of one true frame: n_in inliers (rotation within 0.02 rad, translation + N(0, 0.02), lever points
    within a cube of side 10) at seeded positions, the rest outliers cycling through three kinds: a random rotation,
    the right rotation with translation + N(0, 5) (far_offset), both.  Returns (F [m, d, d + 1], x [m, d], inlier [m]
    bool)."""
    rng = np.random.default_rng(seed)
    Rt, tt = F._random_rotation(rng, d), rng.uniform(-5, 5, d)
    inl = np.zeros(m, bool)
    inl[rng.choice(m, size=n_in, replace=False)] = True
    Fk, xk = np.zeros((m, d, d + 1)), rng.uniform(-5, 5, (m, d))
    kind = 0
    for k in range(m):
        Rk = Rt @ _small_rotation(rng, d, 0.02)
        tk = tt + rng.normal(0.0, 0.02, d)
        if not inl[k]:
            if kind % 3 != 1:
                while True:
                    Rk = F._random_rotation(rng, d)
                    if np.linalg.norm(Rk - Rt) > 1.2 * C_R:
                        break
            if kind % 3 != 0:
                tk = tt + far_offset(rng, d, C_T)
            kind += 1
        Fk[k, :, :d], Fk[k, :, d] = Rk, tk
    return Fk, xk, inl


@functools.lru_cache(maxsize=None)
def multi_group(d):
    """Groups of GROUP_SIZES in one call, 40 % inliers each (at least two from size 2 on; 60 % outliers).  Returns
    dict(F [m, d, d + 1], x [m, d], group_off, inlier [m], c_R, c_t)."""
    Fs, xs, ins, off = [], [], [], [0]
    for i, mg in enumerate(GROUP_SIZES):
        n_in = mg if mg <= 2 else max(2, int(round(0.4 * mg)))
        Fk, xk, inl = make_group(d, mg, n_in, 1000 * d + i)
        Fs.append(Fk), xs.append(xk), ins.append(inl), off.append(off[-1] + mg)
    out = dict(d=d, F=np.concatenate(Fs), x=np.concatenate(xs), group_off=np.asarray(off, np.int32),
               inlier=np.concatenate(ins), c_R=C_R, c_t=C_T)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def big_group(d=3):
    """One group of 1,000 candidates (16 x 16 tiles, the last of 40), 40 % inliers."""
    Fk, xk, inl = make_group(d, 1000, 400, 4242)
    return dict(d=d, F=Fk, x=xk, group_off=np.asarray([0, 1000], np.int32), inlier=inl, c_R=C_R, c_t=C_T)


def groups_of(case):
    go = case["group_off"]
    return [(case["F"][go[g]:go[g + 1]], case["x"][go[g]:go[g + 1]], case["inlier"][go[g]:go[g + 1]])
            for g in range(len(go) - 1)]


# ---------------------------------------------------------------------------------------- graph level
def _se(T, p, d):
    b = d + 1
    return np.asarray(T[:, p * b:p * b + d], dtype=LD), np.asarray(T[:, p * b + d], dtype=LD)


def graph_candidates(d, p1, p2, R, t, aop, T_local):
    """dpgo_graph_pcm's groups in longdouble: {(A, B): (edges, F [m_g, d, d + 1], x [m_g, d])} for every agent pair
    A < B with shared closures, edges in graph order.  F_k = T_local(a_k) Z_k^{+-1} T_local(b_k)^-1, x_k = the
    translation of T_local(b_k)."""
    aop = np.asarray(aop)
    out = {}
    for e in range(len(p1)):
        i, j = int(p1[e]), int(p2[e])
        ai, aj = int(aop[i]), int(aop[j])
        if ai == aj:
            continue
        Re, te = np.asarray(R[e], dtype=LD), np.asarray(t[e], dtype=LD)
        if ai < aj:
            pa, pb, Zr, Zt = i, j, Re, te
        else:
            pa, pb, Zr, Zt = j, i, Re.T, -Re.T @ te
        Ra, ta = _se(T_local, pa, d)
        Rb, tb = _se(T_local, pb, d)
        Wr, Wt = Ra @ Zr, Ra @ Zt + ta
        Fr = Wr @ Rb.T
        es, Fs, xs = out.setdefault((min(ai, aj), max(ai, aj)), ([], [], []))
        es.append(e), Fs.append(np.concatenate([Fr, (Wt - Fr @ tb)[:, None]], axis=1)), xs.append(tb)
    return {k: (np.asarray(v[0]), np.asarray(v[1], dtype=LD), np.asarray(v[2], dtype=LD)) for k, v in out.items()}


def subset_alignment(d, p1, p2, R, t, aop, K, T_local, use):
    """The single-parent breadth-first alignment of tests/_frames.two_stage_alignment with the inlier set GIVEN
    (use [m] bool) instead of decided: per new agent the candidates of its closures with the agent being dequeued,
    rotation = the chordal L2 mean (unit weights) of the used candidates projected to SO(d), translation = their
    mean.  An agent none of whose candidates is used waits for another parent.  Longdouble; returns dict(frames
    K x d x (d + 1), parent, candidates, inliers)."""
    b = d + 1
    aop = np.asarray(aop)
    Tl = np.asarray(T_local, dtype=LD)
    Rl = lambda p: Tl[:, p * b:p * b + d]
    tl = lambda p: Tl[:, p * b + d]
    FR, Ft = np.zeros((K, d, d), dtype=LD), np.zeros((K, d), dtype=LD)
    parent, cand, inl = -np.ones(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int32)
    nbr, shared = [set() for _ in range(K)], [[] for _ in range(K)]
    for e in range(len(p1)):
        ai, aj = int(aop[p1[e]]), int(aop[p2[e]])
        if ai != aj:
            nbr[ai].add(aj), nbr[aj].add(ai), shared[ai].append(e), shared[aj].append(e)
    root = int(aop[0])
    FR[root] = np.eye(d)
    done = np.zeros(K, bool)
    done[root] = True
    order, h = [root], 0
    while h < len(order):
        P = order[h]
        h += 1
        for A in sorted(nbr[P]):
            if done[A]:
                continue
            cR, ct, n_c = [], [], 0
            for e in shared[A]:
                i, j = int(p1[e]), int(p2[e])
                a_is_j = aop[j] == A
                other, mine = (i, j) if a_is_j else (j, i)
                if aop[other] != P:
                    continue
                n_c += 1
                if not use[e]:
                    continue
                Ro, to = FR[P] @ Rl(other), FR[P] @ tl(other) + Ft[P]
                Re, te = np.asarray(R[e], dtype=LD), np.asarray(t[e], dtype=LD)
                if a_is_j:
                    Rw, tw = Ro @ Re, to + Ro @ te
                else:
                    Rw = Ro @ Re.T
                    tw = to - Rw @ te
                Fi = Rw @ Rl(mine).T
                cR.append(Fi), ct.append(tw - Fi @ tl(mine))
            if not cR:
                continue
            FR[A] = F.project_so(np.sum(np.asarray(cR, dtype=LD), axis=0))
            Ft[A] = np.sum(np.asarray(ct, dtype=LD), axis=0) / LD(len(ct))
            parent[A], cand[A], inl[A] = P, n_c, len(cR)
            done[A] = True
            order.append(A)
    assert done.all()
    frames = np.concatenate([FR, Ft[:, :, None]], axis=2).astype(np.float64)
    return dict(frames=frames, parent=parent, candidates=cand, inliers=inl)


def corrupt_shared(d, p1, p2, R, t, aop, seed, c_t, frac=0.6):
    """Per agent pair with at least three shared closures, int(frac m_g) of them replaced by outliers cycling through
    the three kinds (a rotation at more than 1.2 x the threshold from the measured one; the right rotation with
    translation + N(0, 5) by far_offset; both); smaller groups stay clean (one inlier next to one outlier has no unique maximum
    clique).  Returns (R, t, bad [m] bool)."""
    rng = np.random.default_rng(seed)
    aop = np.asarray(aop)
    R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
    bad = np.zeros(len(p1), bool)
    groups = {}
    for e in range(len(p1)):
        ai, aj = int(aop[p1[e]]), int(aop[p2[e]])
        if ai != aj:
            groups.setdefault((min(ai, aj), max(ai, aj)), []).append(e)
    kind = 0
    for key in sorted(groups):
        es = groups[key]
        if len(es) < 3:
            continue
        for e in rng.choice(es, size=int(frac * len(es)), replace=False):
            if kind % 3 != 1:
                while True:
                    Rn = F._random_rotation(rng, d)
                    if np.linalg.norm(Rn - R[e]) > 1.2 * C_R:
                        break
                R[e] = Rn
            if kind % 3 != 0:
                t[e] += far_offset(rng, d, c_t)
            kind += 1
            bad[e] = True
    return R, t, bad


def chordal_local(d, p1, p2, R, t, kappa, tau, aop, K):
    """Each agent's chordal initialisation on its private graph (the oracle's chordal_initialization, anchored at
    the agent's first pose): T_local d x (d+1) n.  The pair test does not depend on the frame an agent's local
    trajectory is expressed in, so the library's own anchor (the agent's breadth-first centre) gives the same e."""
    aop = np.asarray(aop)
    n, b = len(aop), d + 1
    local = F.local_index(aop, K)
    T = np.zeros((d, n * b))
    for a in range(K):
        idx = np.nonzero(aop == a)[0]
        es = np.nonzero((aop[p1] == a) & (aop[p2] == a))[0]
        m = len(es)
        meas = O.Measurements(d, np.zeros(m, np.int64), np.zeros(m, np.int64), local[p1[es]], local[p2[es]], R[es],
                              t[es], kappa[es], tau[es], np.ones(m), len(idx))
        Ta = O.chordal_initialization(d, len(idx), meas)
        for l, p in enumerate(idx):
            T[:, p * b:(p + 1) * b] = Ta[:, l * b:(l + 1) * b]
    return T


def _pcm_fixture(base, seed, c_t, local):
    fx = dict(d=base["d"], n=base["n"], K=base["K"], aop=base["aop"], p1=base["p1"], p2=base["p2"],
              kappa=base["kappa"], tau=base["tau"], c_R=C_R, c_t=c_t, local=local)
    fx["T_local"] = (np.array(base["T_local"]) if local == "odometry" else
                     chordal_local(fx["d"], fx["p1"], fx["p2"], base["R_clean"], base["t_clean"], fx["kappa"],
                                   fx["tau"], fx["aop"], fx["K"]))
    fx["R"], fx["t"], fx["bad"] = corrupt_shared(fx["d"], fx["p1"], fx["p2"], base["R_clean"], base["t_clean"],
                                                 fx["aop"], seed, c_t)
    shared = fx["aop"][fx["p1"]] != fx["aop"][fx["p2"]]
    fx["shared"] = shared
    fx["labels"] = np.where(shared, np.where(fx["bad"], 0, 1), 255).astype(np.uint8)
    for v in fx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx


# c_t per fixture: above the disagreement odometry drift leaves between clean closures of one agent pair, below what
# N(0, 5) puts between an outlier and anything else; tests/test_pcm_reference.py asserts both sides for these seeds
SEED3D, SEED2D = 21, 22


@functools.lru_cache(maxsize=None)
def fixture3d():
    """tests/_frames.fixture3d's graph, partition and odometry local trajectories (odometry is never corrupted) with
    60 % of every agent pair's shared closures corrupted."""
    return _pcm_fixture(F.fixture3d(), SEED3D, 1.5, "odometry")


@functools.lru_cache(maxsize=None)
def fixture2d():
    """The 2D twin on tests/_frames.fixture2d's CSAIL partition, local trajectories by each agent's chordal
    initialisation on its (uncorrupted) private graph.  The clean closures between the two long agents 0 and 1 then
    still disagree by up to 3.6 m (5.3 m under odometry), hence c_t = 4.5."""
    return _pcm_fixture(F.fixture2d(), SEED2D, 4.5, "chordal")


def graph_of(H, fx):
    return H.Graph.from_arrays(fx["d"], fx["n"], fx["p1"], fx["p2"], fx["R"], fx["t"], fx["kappa"], fx["tau"])
