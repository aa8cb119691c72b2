"""Host model of the robust reweighting (test infrastructure): the weights, mu and the converged ratios that
PGOAgent::updateLoopClosuresWeights / computeConvergedLoopClosureRatio (src/PGOAgent.cpp:1174-1289) and RobustCost
(src/DPGO_robust.cpp) give along a colour schedule, edge by edge in np.longdouble, from a recorded history of X.

It is a second restatement, independent of oracle.dpgo_oracle.Agent: no agents, no dictionaries of poses, no Q -- the
global edge list, the owner rule and one table of "which iterate does agent a hold of its neighbours".
test_robust_reference.py checks the two against each other on the oracle's own history; test_gpu_robust.py then
compares the engine with this model on the engine's history.

Acceleration must be off: only then is an agent's X at the start of an iteration the recorded X after the previous
one (a non-selected agent's iterate(false) leaves X alone).
"""
import math

import numpy as np

from oracle import dpgo_oracle as O
from tests import _ragged as RG

_L = np.longdouble

ENGINE_AGENTS = [50, 130, 64, 97, 120, 65, 119]  # test_gpu_ragged.ENGINE_AGENTS (asserted equal on the CPU)
EXTRA_POSES = 5                                  # one more agent: an odometry chain in a component of its own
AGENTS = ENGINE_AGENTS + [EXTRA_POSES]
EXTRA_AGENT = len(ENGINE_AGENTS)
N_POSES = RG.N_POSES + EXTRA_POSES               # 650

_cache = {}


def robust_case(d):
    """(meas, agent_of_pose, T_true) of the robust tests, computed once per d and never modified: the ragged graph with
    10 % of its loop closures corrupted (translations + N(0, 5), default_rng(7): the recipe of
    test_gpu_ragged.engine_case), its seven unequal agents, and poses 645..649 -- a chain of four odometry edges with
    noise 0.05 that no edge joins to the rest, owned by an eighth agent without any loop closure."""
    if d in _cache:
        return _cache[d]
    meas, T = RG.ragged_graph(d)
    rng = np.random.default_rng(7)
    lc = np.nonzero(np.abs(meas.p2 - meas.p1) != 1)[0]
    bad = rng.choice(lc, size=max(1, int(0.1 * len(lc))), replace=False)
    t = meas.t.copy()
    t[bad] += rng.normal(0.0, 5.0, size=(len(bad), d))
    b = d + 1
    sm = O.SplitMix64(4200 + d)
    Rg = [RG._rot(sm, d) for _ in range(EXTRA_POSES)]
    tg = [np.array([10.0 * sm.uniform() - 5.0 for _ in range(d)]) for _ in range(EXTRA_POSES)]
    k = EXTRA_POSES - 1
    Rx, tx, kx, taux = np.zeros((k, d, d)), np.zeros((k, d)), np.zeros(k), np.zeros(k)
    for e in range(k):
        Rx[e] = Rg[e].T @ Rg[e + 1] @ RG._rot(sm, d, 0.05)
        tx[e] = Rg[e].T @ (tg[e + 1] - tg[e]) + 0.05 * np.array([sm.normal() for _ in range(d)])
        kx[e] = 0.5 + 49.5 * sm.uniform()
        taux[e] = 0.5 + 49.5 * sm.uniform()
    Tx = np.zeros((d, b * EXTRA_POSES))
    for j in range(EXTRA_POSES):
        Tx[:, j * b:j * b + d] = Rg[j]
        Tx[:, j * b + d] = tg[j]
    p1 = np.concatenate([meas.p1, RG.N_POSES + np.arange(k)]).astype(np.int64)
    p2 = np.concatenate([meas.p2, RG.N_POSES + 1 + np.arange(k)]).astype(np.int64)
    m = len(p1)
    z = np.zeros(m, np.int64)
    full = O.Measurements(d, z, z.copy(), p1, p2, np.concatenate([meas.R, Rx]), np.concatenate([t, tx]),
                          np.concatenate([meas.kappa, kx]), np.concatenate([meas.tau, taux]), np.ones(m), N_POSES)
    aop = np.repeat(np.arange(len(AGENTS)), AGENTS).astype(np.int32)
    assert len(aop) == N_POSES
    for a in (full.p1, full.p2, full.R, full.t, full.kappa, full.tau, aop):
        a.setflags(write=False)
    _cache[d] = (full, aop, np.concatenate([T, Tx], axis=1))
    return _cache[d]


def fresh(meas):
    """A copy of meas whose weights an oracle run may overwrite (Agent.update_loop_closure_weights writes through the
    subsets, never into meas itself, but the unit weights are cheap to guarantee)."""
    return O.Measurements(meas.d, meas.r1, meas.r2, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau,
                          np.ones(meas.m), meas.num_poses)


# ------------------------------------------------------------------------------------------ structure
class Structure:
    """Who reweights what.  Per edge: a1 / a2 the agents of its endpoints; owner (dpgo_rbcd_weight_owner's rule:
    -1 odometry = a private edge between consecutive local indices, a private loop closure its agent, a shared one the
    lower-ID agent); lc = the reweighted edges in edge order; per agent the copies its converged ratio counts."""

    def __init__(self, meas, agent_of_pose, num_agents):
        aop = np.asarray(agent_of_pose, np.int64)
        local = np.zeros(len(aop), np.int64)
        seen = np.zeros(num_agents, np.int64)
        for i, a in enumerate(aop):
            local[i] = seen[a]
            seen[a] += 1
        self.num_agents = num_agents
        self.a1, self.a2 = aop[meas.p1], aop[meas.p2]
        private = self.a1 == self.a2
        odo = private & (local[meas.p2] == local[meas.p1] + 1)
        self.owner = np.where(odo, -1, np.minimum(self.a1, self.a2))
        self.shared = ~private
        self.lc = np.nonzero(self.owner >= 0)[0]
        # the endpoint held by the owner's neighbour (0: p1, 1: p2, -1: a private edge)
        self.nbr_end = np.where(private, -1, np.where(self.a1 < self.a2, 1, 0))
        self.own_copies = [np.nonzero(self.owner == a)[0] for a in range(num_agents)]
        other = np.maximum(self.a1, self.a2)
        self.other_copies = [np.nonzero(self.shared & (other == a))[0] for a in range(num_agents)]

    def ratio(self, w, a):
        """computeConvergedLoopClosureRatio of agent a at the edge weights w: its own copies at w, the copies of shared
        loop closures it is the higher-ID end of at 1 (never updated, :1206 / :1221); 0/0 = NaN."""
        own = w[self.own_copies[a]]
        total = len(own) + len(self.other_copies[a])
        if total == 0:
            return float("nan")
        return float(int(np.sum((own == 1.0) | (own == 0.0))) + len(self.other_copies[a])) / float(total)


# ------------------------------------------------------------------------------------------ the cost
DEFAULTS = dict(gnc_max_iters=100, gnc_barc=10.0, gnc_mu_step=1.4, gnc_init_mu=1e-4, huber=3.0, tls=10.0)


def gnc_bounds(mu, barc, dtype=_L):
    mu, bc = dtype(mu), dtype(barc) * dtype(barc)
    return mu / (mu + 1) * bc, (mu + 1) / mu * bc  # (lower, upper) on r^2


def weight(kind, res, mu, p, dtype=_L):
    """RobustCost::weight (src/DPGO_robust.cpp:23-67) of an array of residuals, evaluated in dtype."""
    res = np.asarray(res, dtype)
    one, zero = dtype(1), dtype(0)
    if kind == "L2":
        return np.ones_like(res)
    if kind == "L1":
        return one / res
    if kind == "Huber":
        h = dtype(p["huber"])
        return np.where(res < h, one, h / res)
    if kind == "TLS":
        return np.where(res < dtype(p["tls"]), one, zero)
    if kind == "GM":
        a = one + res * res
        return one / (a * a)
    if kind == "GNC_TLS":
        rsq = res * res
        lower, upper = gnc_bounds(mu, p["gnc_barc"], dtype)
        m_, bc = dtype(mu), dtype(p["gnc_barc"]) * dtype(p["gnc_barc"])
        mid = np.sqrt(bc * m_ * (m_ + 1) / rsq) - m_
        return np.where(rsq >= upper, zero, np.where(rsq <= lower, one, mid))
    raise ValueError(kind)


def branch_gap(kind, res, mu, p):
    """Per residual: the relative distance from the nearest branch threshold of the cost (of r^2 for GNC_TLS, of r for
    Huber and TLS; inf for the costs without a branch), in np.longdouble."""
    res = np.asarray(res, _L)
    if kind == "GNC_TLS":
        rsq = res * res
        lower, upper = gnc_bounds(mu, p["gnc_barc"])
        return np.minimum(np.abs(rsq - lower) / lower, np.abs(rsq - upper) / upper).astype(float)
    if kind in ("Huber", "TLS"):
        thr = _L(p["huber"] if kind == "Huber" else p["tls"])
        return (np.abs(res - thr) / thr).astype(float)
    return np.full(res.shape, np.inf)


def gnc_branch(res, mu, p):
    """0: w = 1, 1: the middle formula, 2: w = 0 (np.longdouble)."""
    rsq = np.asarray(res, _L) ** 2
    lower, upper = gnc_bounds(mu, p["gnc_barc"])
    return np.where(rsq >= upper, 2, np.where(rsq <= lower, 0, 1))


def _blocks(X, poses, d, dtype):
    r, b = X.shape[0], d + 1
    return np.asarray(X, dtype).reshape(r, -1, b).transpose(1, 0, 2)[poses]


def residuals(meas, idx, P1, P2, dtype=_L):
    """sqrt(computeMeasurementError) (src/DPGO_utils.cpp:509-515) of the edges idx between the pose blocks P1, P2
    (len(idx) x r x (d+1)): sqrt(kappa |Y1 R - Y2|^2 + tau |p2 - p1 - Y1 t|^2)."""
    d = meas.d
    R, t = meas.R[idx].astype(dtype), meas.t[idx].astype(dtype)
    Y1, q1, Y2, q2 = P1[:, :, :d], P1[:, :, d], P2[:, :, :d], P2[:, :, d]
    rot = np.sum((Y1 @ R - Y2) ** 2, axis=(1, 2), dtype=dtype)
    tra = np.sum((q2 - q1 - (Y1 @ t[:, :, None])[:, :, 0]) ** 2, axis=1, dtype=dtype)
    return np.sqrt(meas.kappa[idx].astype(dtype) * rot + meas.tau[idx].astype(dtype) * tra)


def residuals_at(meas, st, X, dtype=_L):
    """Residual of every reweighted edge (st.lc) with both endpoints taken from X."""
    return residuals(meas, st.lc, _blocks(X, meas.p1[st.lc], meas.d, dtype), _blocks(X, meas.p2[st.lc], meas.d, dtype),
                     dtype)


# ------------------------------------------------------------------------------------------ the schedule
def run_model(meas, agent_of_pose, colors, kind, X_hist, inner_iters, params=None, dtype=_L):
    """The reweighting along the colour schedule.  X_hist[0] is the start, X_hist[t] the iterate after iteration t
    (t = 1..T, iteration t selects colour (t - 1) mod C).  Returns one dict per iteration:
      w      weight of every edge (edge order, the owner's copy; odometry 1)
      mu     the mu this iteration's reweighting used (None when it did not reweight), mu_next the one it left
      res    np.longdouble residual per edge of st.lc that this iteration reweighted (NaN where it did not)
      ratio  per agent the converged ratio as of its last selected iteration (None before it)
      selected  the agents selected so far
    dtype is the arithmetic of residuals and weights (np.longdouble the reference, np.float64 its plain-numpy twin that
    sets the bars); mu itself is the host's double product in both, as in RobustCost::update."""
    p = dict(DEFAULTS)
    p.update(params or {})
    colors = np.asarray(colors)
    K, C = len(colors), int(max(colors)) + 1
    st = Structure(meas, agent_of_pose, K)
    d = meas.d
    lc = st.lc
    own, shared, nbr_end = st.owner[lc], st.shared[lc], st.nbr_end[lc]
    w = np.ones(meas.m, dtype)
    held = np.full(K, -1)  # index into X_hist of the neighbour poses agent a holds (its last selection), -1: none
    mu, gnc_iter = float(p["gnc_init_mu"]), 0
    ratio = [None] * K
    out = []
    for t in range(1, len(X_hist)):
        c = (t - 1) % C
        sel = colors == c
        # updateNeighborPoses: the selected agents receive their neighbours' poses of this iteration, which no
        # update has touched since the end of iteration t - 1
        held[sel] = t - 1
        rec = dict(mu=None, res=np.full(len(lc), np.nan, _L))
        if kind != "L2" and (t + 1) % inner_iters == 0:  # shouldUpdateLoopClosureWeights with mIterationNumber = t
            Xs = X_hist[t - 1]
            h = held[own]
            can = ~shared | (h >= 0)  # a shared loop closure waits for its owner's first selection (:1212, :1227)
            P1 = _blocks(Xs, meas.p1[lc], d, dtype).copy()
            P2 = _blocks(Xs, meas.p2[lc], d, dtype).copy()
            for s in np.unique(h[shared & can]):  # neighbour endpoints from the iterate the owner holds
                Xh = X_hist[s]
                for end, P, poses in ((0, P1, meas.p1), (1, P2, meas.p2)):
                    pick = np.nonzero(shared & can & (h == s) & (nbr_end == end))[0]
                    P[pick] = _blocks(Xh, poses[lc[pick]], d, dtype)
            res = residuals(meas, lc[can], P1[can], P2[can], dtype)
            w[lc[can]] = weight(kind, res, mu, p, dtype)
            rec["res"][can] = res
            rec["mu"] = mu
            if kind == "GNC_TLS":  # RobustCost::update (:85-103)
                gnc_iter += 1
                if gnc_iter <= p["gnc_max_iters"]:
                    mu = p["gnc_mu_step"] * mu
        for a in np.nonzero(sel)[0]:
            ratio[a] = st.ratio(w, a) if kind == "GNC_TLS" else 1.0
        rec.update(w=w.copy(), mu_next=mu, ratio=list(ratio), selected=held >= 0)
        out.append(rec)
    return out


def ready_from_ratio(ratio, threshold):
    """readyToTerminate with an unlimited relative-change tolerance: not (ratio < threshold) (:706-712)."""
    return not (ratio < threshold)


# ------------------------------------------------------------------------------------------ oracle side
def oracle_edge_lists(meas, agent_of_pose, num_agents):
    """Per agent the global edge indices behind its private_lc / shared_lc, in the order O._split builds them."""
    st = Structure(meas, agent_of_pose, num_agents)
    priv = [np.nonzero(~st.shared & (st.owner == a))[0] for a in range(num_agents)]
    shared = [np.nonzero(st.shared & ((st.a1 == a) | (st.a2 == a)))[0] for a in range(num_agents)]
    return priv, shared


def oracle_weights(agents, meas, agent_of_pose):
    """The oracle's Agents' weights at the graph's edges under the weight_owner rule (the responsible copy); the other
    copy of every shared loop closure is asserted to be exactly 1."""
    priv, shared = oracle_edge_lists(meas, agent_of_pose, len(agents))
    st = Structure(meas, agent_of_pose, len(agents))
    w = np.ones(meas.m)
    for ag in agents:
        assert ag.private_lc.m == len(priv[ag.id]) and ag.shared_lc.m == len(shared[ag.id])
        w[priv[ag.id]] = ag.private_lc.weight
        mine = st.owner[shared[ag.id]] == ag.id
        w[shared[ag.id][mine]] = ag.shared_lc.weight[mine]
        assert np.all(ag.shared_lc.weight[~mine] == 1.0)
    return w


def thresholds_from(ratios):
    """The min_convergence_ratio values of the ready tests from the agents' finite ratios: one below the smallest, every
    midpoint between consecutive distinct values, every distinct value itself (ratio == threshold is ready) and one
    above 1."""
    vals = sorted({x for x in ratios if x is not None and not math.isnan(x)})
    assert vals and vals[0] > 0.0
    mids = [(a + b) / 2 for a, b in zip(vals[:-1], vals[1:])]
    return [vals[0] / 2] + mids + vals + [1.5]
