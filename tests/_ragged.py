"""A deterministic ragged pose graph, its tiling restated on the host, and an edge-by-edge extended-precision
reference of the quadratic problem (test infrastructure).

The committed datasets and the grid3d generator never leave the SpMM's staged, straight-line paths: no tile of theirs
has more than 512 incidences, no d = 3 tile more than 200 first-visit records, no d = 3 pose more than 6 incidences and
no pose none.  ragged_graph() builds one small graph (n = 645, 11 tiles) that takes every other path, tile_profile()
restates what the kernels see of it so the tests can assert that it still does, and edge_reference() evaluates the
problem without ever assembling Q, in np.longdouble.
"""
import numpy as np

from oracle import dpgo_oracle as O

TILE = 64            # kTilePoses (dpgo_device.h)
# The kernels' thresholds, restated (kernels.hip); the graph clears each by at least 5 % on the side it needs.
INC_STAGE = 512      # kIncStage: incidences of a tile that fit the LDS stage
REC_STAGE = {3: 200, 2: 256}  # rec_stage<D>(): first-visit records of a tile that fit the LDS stage
UNI_MAX = 8          # kUniMax: incidences of a pose that edge_loop_uni handles straight-line
MARGIN = 1.05

N_POSES = 645        # ten full tiles and one of 5 poses
ISOLATED = 6 * TILE + 33            # no measurement at all; the chain is cut around it
CUT = (3 * TILE + 1, 3 * TILE + 2)  # 193, 194: no edge between them (with RAGGED_AGENTS both have only shared edges)
HUBS = {5 * TILE + 10: 8, 5 * TILE + 20: 9, 5 * TILE + 30: 10, 5 * TILE + 40: 11}  # pose -> exact degree (tile 5)
PARALLEL = (4 * TILE + 5, 4 * TILE + 9)        # i -> j twice
ANTIPARALLEL = (4 * TILE + 20, 4 * TILE + 25)  # i -> j and j -> i
TILE_BOTH, TILE_NI, TILE_NE = 2, 8, 1  # unstaged by ni and ne / by ni alone / by ne alone
RAGGED_AGENTS = [1, 63, 64, 65, 2, 130, N_POSES - 325]


def _pick(rng, k):
    return int(rng.next_u64() % k)


def _topology(seed):
    rng = O.SplitMix64(seed)
    n = N_POSES
    edges, seen = [], set()

    def add(i, j, force=False):
        key = (min(i, j), max(i, j))
        if i == j or (key in seen and not force):
            return False
        seen.add(key)
        edges.append((i, j))
        return True

    keep_out = set(HUBS) | {ISOLATED} | set(CUT)
    for i in range(n - 1):  # odometry chain, cut around the isolated pose and between the CUT pair
        if i in (ISOLATED - 1, ISOLATED, CUT[0]):
            continue
        add(i, i + 1)
    add(ISOLATED - 1, ISOLATED + 1)
    add(CUT[0], CUT[1] + 1)

    def tile_pose(t):
        while True:
            p = t * TILE + _pick(rng, TILE)
            if p not in keep_out:
                return p

    def scatter(ta, tb, count):
        got = 0
        while got < count:
            i, j = tile_pose(ta), tile_pose(tb)
            if _pick(rng, 2):
                i, j = j, i
            got += add(i, j)

    scatter(TILE_BOTH, TILE_BOTH, 240)  # dense inside the tile: both lists overflow
    for t in range(2, 8):  # many second visits from six lower tiles: the incidence list alone overflows
        scatter(t, TILE_NI, 72)
    for t, c in zip((3, 4, 5, 6, 7, 9), (39, 39, 38, 38, 38, 38)):  # first visits to higher tiles: the records alone
        scatter(TILE_NE, t, c)
    offsets = [-7, 3, -66, 5, -3, 70, -5, 7, 2]  # lower and higher partners, in the tile and in both neighbours
    for h, deg in HUBS.items():
        for q in range(deg - 2):  # the chain gives two
            x = h + offsets[q]
            assert add(h, x) if q % 2 == 0 else add(x, h)
    add(*PARALLEL)
    add(*PARALLEL, force=True)
    add(*ANTIPARALLEL)
    add(ANTIPARALLEL[1], ANTIPARALLEL[0], force=True)
    return np.array(edges, dtype=np.int64)


def _rot(rng, d, sigma=None):
    """A random rotation (sigma None) or one within ~sigma of the identity."""
    if sigma is None:
        M = np.array([[rng.normal() for _ in range(d)] for _ in range(d)])
    else:
        W = np.array([[rng.normal() for _ in range(d)] for _ in range(d)])
        M = np.eye(d) + sigma * 0.5 * (W - W.T)
    return O.project_to_rotation(M)


def ragged_graph(d, seed=7):
    """(meas, T_true): O.Measurements of the ragged graph and the ground-truth poses (d x (d+1) n, [R_j | t_j]).
    Measurements are the ground truth's relative poses with noise of sigma 0.05 on rotation and translation, kappa and
    tau uniform in [0.5, 50].  The topology depends on the seed only, not on d."""
    E = _topology(seed)
    n, m, b = N_POSES, len(E), d + 1
    rng = O.SplitMix64(seed * 1000 + d)
    Rg = [_rot(rng, d) for _ in range(n)]
    tg = [np.array([10.0 * rng.uniform() - 5.0 for _ in range(d)]) for _ in range(n)]
    R = np.zeros((m, d, d))
    t = np.zeros((m, d))
    kappa = np.zeros(m)
    tau = np.zeros(m)
    for e, (i, j) in enumerate(E):
        R[e] = Rg[i].T @ Rg[j] @ _rot(rng, d, 0.05)
        t[e] = Rg[i].T @ (tg[j] - tg[i]) + 0.05 * np.array([rng.normal() for _ in range(d)])
        kappa[e] = 0.5 + 49.5 * rng.uniform()
        tau[e] = 0.5 + 49.5 * rng.uniform()
    T = np.zeros((d, b * n))
    for j in range(n):
        T[:, j * b:j * b + d] = Rg[j]
        T[:, j * b + d] = tg[j]
    z = np.zeros(m, dtype=np.int64)
    return O.Measurements(d, z, z.copy(), E[:, 0].copy(), E[:, 1].copy(), R, t, kappa, tau, np.ones(m), n), T


def tile_profile(p1, p2, agent_sizes):
    """The tiling as the library builds it: tiles of 64 consecutive poses per agent; an incidence is an edge with both
    endpoints in one agent, counted at either endpoint; the lower endpoint visits an edge first.  Returns a dict of
    per-tile arrays (agent, start, count, ni, ne) and per-pose arrays (degree = incidences, shared = edges to other
    agents, tile)."""
    p1 = np.asarray(p1, np.int64)
    p2 = np.asarray(p2, np.int64)
    sizes = [int(s) for s in agent_sizes]
    n = sum(sizes)
    agent_of = np.repeat(np.arange(len(sizes)), sizes)
    starts, counts, agents = [], [], []
    off = 0
    for a, s in enumerate(sizes):
        for t0 in range(0, s, TILE):
            starts.append(off + t0)
            counts.append(min(TILE, s - t0))
            agents.append(a)
        off += s
    starts, counts = np.array(starts), np.array(counts)
    tile_of = np.repeat(np.arange(len(starts)), counts)
    private = agent_of[p1] == agent_of[p2]
    degree = np.bincount(p1[private], minlength=n) + np.bincount(p2[private], minlength=n)
    shared = np.bincount(p1[~private], minlength=n) + np.bincount(p2[~private], minlength=n)
    first = np.minimum(p1, p2)[private]
    return dict(agent=np.array(agents), start=starts, count=counts,
                ni=np.bincount(tile_of, weights=degree, minlength=len(starts)).astype(np.int64),
                ne=np.bincount(tile_of[first], minlength=len(starts)), degree=degree, shared=shared, tile=tile_of)


def tile_staged(prof, d):
    """Per tile: does the SpMM stage it in LDS (both lists fit)?"""
    return (prof["ni"] <= INC_STAGE) & (prof["ne"] <= REC_STAGE[d])


def describe_pose(prof, d, j):
    """'pose j (tile t, degree k, staged/unstaged)': where a per-pose failure points."""
    t = int(prof["tile"][j])
    return (f"pose {j} (tile {t}: ni {int(prof['ni'][t])}, ne {int(prof['ne'][t])}, "
            f"{'staged' if tile_staged(prof, d)[t] else 'unstaged'}; degree {int(prof['degree'][j])})")


def assert_profile(meas):
    """Every path condition of the graph, with the 5 % margins, from the profile alone (single agent)."""
    d = meas.d
    prof = tile_profile(meas.p1, meas.p2, [meas.num_poses])
    ni, ne, deg = prof["ni"], prof["ne"], prof["degree"]
    hi_i = INC_STAGE * MARGIN
    hi_e, lo_e = max(REC_STAGE.values()) * MARGIN, min(REC_STAGE.values())
    assert meas.num_poses == N_POSES and len(ni) == 11
    assert ni[TILE_BOTH] > hi_i and ne[TILE_BOTH] > hi_e
    assert ni[TILE_NI] > hi_i and ne[TILE_NI] <= lo_e / MARGIN
    assert ni[TILE_NE] <= INC_STAGE / MARGIN and ne[TILE_NE] > hi_e
    staged = tile_staged(prof, d)
    assert [t for t in range(11) if not staged[t]] == sorted((TILE_BOTH, TILE_NI, TILE_NE))
    for t in np.nonzero(staged)[0]:
        assert ni[t] <= INC_STAGE / MARGIN and ne[t] <= lo_e / MARGIN, t
    for h, k in HUBS.items():  # the kUniMax boundary, and an odd and an even ping-pong tail
        assert deg[h] == k and staged[prof["tile"][h]], h
        out_, in_ = int(np.sum(meas.p1 == h)), int(np.sum(meas.p2 == h))
        assert out_ >= 3 and in_ >= 3, (h, out_, in_)
        lower = int(np.sum((meas.p1 == h) & (meas.p2 < h)) + np.sum((meas.p2 == h) & (meas.p1 < h)))
        assert 3 <= lower <= k - 3, (h, lower)  # second and first visits both
    assert sorted(HUBS.values()) == [UNI_MAX, UNI_MAX + 1, UNI_MAX + 2, UNI_MAX + 3]
    assert max(deg[j] for j in range(N_POSES) if not staged[prof["tile"][j]]) >= UNI_MAX + 1
    assert deg[ISOLATED] == 0 and int(np.sum(deg == 0)) == 1
    assert prof["count"][-1] < 8
    pairs = {}
    for i, j in zip(meas.p1.tolist(), meas.p2.tolist()):
        pairs[(i, j)] = pairs.get((i, j), 0) + 1
    assert [k for k, v in pairs.items() if v > 1] == [PARALLEL] and pairs[PARALLEL] == 2
    assert [k for k in pairs if k[0] < k[1] and (k[1], k[0]) in pairs] == [ANTIPARALLEL]
    return prof


# ----------------------------------------------------------------------------------------
# Extended-precision reference, edge by edge
# ----------------------------------------------------------------------------------------
_L = np.longdouble


def _poses(V, r, b):
    return V.reshape(r, -1, b).transpose(1, 0, 2)


def _flat(P):
    n, r, b = P.shape
    return P.transpose(1, 0, 2).reshape(r, n * b)


def edge_apply(meas, V, p1=None, p2=None):
    """V Q (r x (d+1) n) in np.longdouble without assembling Q: per edge i -> j with T = [R t; 0 1] and
    Omega = w diag(kappa I, tau), block ii gets T Omega T^T, block jj Omega, block ij -T Omega and block ji
    -Omega T^T.  p1 / p2 override the endpoints; an endpoint of -1 is another agent's pose: such an edge keeps the
    diagonal block of its local endpoint only (PGOAgent::constructQMatrix)."""
    d = meas.d
    b = d + 1
    p1 = np.asarray(meas.p1 if p1 is None else p1, np.int64)
    p2 = np.asarray(meas.p2 if p2 is None else p2, np.int64)
    m = len(p1)
    r = V.shape[0]
    Vp = _poses(np.asarray(V).astype(_L), r, b)
    T = np.zeros((m, b, b), _L)
    T[:, :d, :d] = meas.R
    T[:, :d, d] = meas.t
    T[:, d, d] = 1
    om = np.zeros((m, b), _L)
    w = np.asarray(meas.weight).astype(_L)
    om[:, :d] = (w * np.asarray(meas.kappa).astype(_L))[:, None]
    om[:, d] = w * np.asarray(meas.tau).astype(_L)
    TOm = T * om[:, None, :]                     # T Omega
    Wii = TOm @ np.swapaxes(T, 1, 2)             # T Omega T^T
    has1, has2 = p1 >= 0, p2 >= 0
    both = has1 & has2
    i1, i2 = np.where(has1, p1, 0), np.where(has2, p2, 0)
    Vi = Vp[i1] * has1[:, None, None]
    Vj = Vp[i2] * has2[:, None, None]
    to_i = Vi @ Wii - (Vj * both[:, None, None]) @ np.swapaxes(TOm, 1, 2)   # V_i Q_ii + V_j Q_ji
    to_j = Vj * om[:, None, :] - (Vi * both[:, None, None]) @ TOm          # V_j Q_jj + V_i Q_ij
    out = np.zeros_like(Vp)
    np.add.at(out, i1[has1], to_i[has1])
    np.add.at(out, i2[has2], to_j[has2])
    return _flat(out)


def project_ext(X, V, d):
    """P_X(V) = V_Y - Y sym(Y^T V_Y) per pose, translations unchanged, in np.longdouble."""
    r = X.shape[0]
    Xp, Vp = _poses(np.asarray(X).astype(_L), r, d + 1), _poses(np.asarray(V).astype(_L), r, d + 1).copy()
    Y, VY = Xp[:, :, :d], Vp[:, :, :d].copy()
    S = np.swapaxes(Y, 1, 2) @ VY
    Vp[:, :, :d] = VY - Y @ ((S + np.swapaxes(S, 1, 2)) / 2)
    return _flat(Vp)


def edge_reference(meas, X, G=None, V=None, p1=None, p2=None):
    """The quadratic problem's evaluations at X (and along V) in np.longdouble, from the measurements alone:
    dict(f, egrad = X Q + G, riegrad = P_X(egrad), gradnorm [, ehvp = V Q, rhvp = P_X(V Q - [V_Y sym(Y^T egrad_Y) | 0])])."""
    d = meas.d
    b = d + 1
    r = X.shape[0]
    XL = np.asarray(X).astype(_L)
    GL = np.zeros_like(XL) if G is None else np.asarray(G).astype(_L)
    XQ = edge_apply(meas, XL, p1, p2)
    EG = XQ + GL
    RG = project_ext(XL, EG, d)
    out = dict(f=np.sum(XQ * XL, dtype=_L) / 2 + np.sum(XL * GL, dtype=_L), egrad=EG, riegrad=RG,
               gradnorm=np.sqrt(np.sum(RG * RG, dtype=_L)))
    if V is not None:
        VL = np.asarray(V).astype(_L)
        VQ = edge_apply(meas, VL, p1, p2)
        Xp, Vp, Gp, Hp = _poses(XL, r, b), _poses(VL, r, b), _poses(EG, r, b), _poses(VQ, r, b).copy()
        S = np.swapaxes(Xp[:, :, :d], 1, 2) @ Gp[:, :, :d]
        Hp[:, :, :d] = Hp[:, :, :d] - Vp[:, :, :d] @ ((S + np.swapaxes(S, 1, 2)) / 2)
        out.update(ehvp=VQ, rhvp=project_ext(XL, _flat(Hp), d))
    return out
