"""Host model of the robust reweighting with weights and known inliers given from outside (test infrastructure):
tests/_robust.run_model's loop in np.longdouble, started from an initial weight per edge instead of ones and with a mask
of fixed edges (the reference's RelativeSEMeasurement::weight and ::isKnownInlier, src/PGOAgent.cpp:1186, 1203, 1257,
1266).

Both copies of a shared edge start at the given weight; the responsible (lower-ID) copy is the one the reweighting
rewrites and the one `w` reports, the other copy keeps the initial weight.  A fixed edge is never rewritten, and both of
its copies are left out of the converged ratio, count and total.

W(d) is the weight recipe the weight tests share; oracle_weights_both reads both copies out of the oracle's Agents.
"""
import numpy as np

from tests import _robust as RB

_L = np.longdouble


def W(d):
    """The weights of the tests on robust_case(d): odometry uniform(0.25, 1); of the loop closures 20 % exactly 0,
    30 % exactly 1, the rest uniform(0.05, 1)."""
    meas, aop, _ = RB.robust_case(d)
    st = RB.Structure(meas, aop, len(RB.AGENTS))
    rng = np.random.default_rng(100 + d)
    w = np.ones(meas.m)
    odo = st.owner < 0
    w[odo] = rng.uniform(0.25, 1, int(odo.sum()))
    u = rng.random(len(st.lc))
    w[st.lc] = np.where(u < 0.2, 0.0, np.where(u < 0.5, 1.0, rng.uniform(0.05, 1, len(st.lc))))
    w.setflags(write=False)
    return w


MASK_AGENT = 2  # every loop closure touching this agent is fixed: its converged ratio is 0/0


def mask(st, m):
    """The known inliers of the tests: st.lc[::3] and every loop closure with an endpoint in agent MASK_AGENT."""
    fixed = np.zeros(m, bool)
    fixed[st.lc[::3]] = True
    fixed[st.lc[(st.a1[st.lc] == MASK_AGENT) | (st.a2[st.lc] == MASK_AGENT)]] = True
    return fixed


def weighted(meas, w):
    """A copy of meas carrying the weights w (the oracle writes through its subsets, never into this)."""
    from oracle import dpgo_oracle as O
    return O.Measurements(meas.d, meas.r1, meas.r2, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau,
                          np.array(w, dtype=float), meas.num_poses)


def ratio(st, w, w0, fixed, a):
    """computeConvergedLoopClosureRatio of agent a: its own copies at w, the copies it is the higher-ID end of at the
    initial weight w0 (never rewritten), fixed copies left out of both sums; 0/0 = NaN."""
    own = st.own_copies[a][~fixed[st.own_copies[a]]]
    other = st.other_copies[a][~fixed[st.other_copies[a]]]
    total = len(own) + len(other)
    if total == 0:
        return float("nan")
    conv = int(np.sum((w[own] == 1.0) | (w[own] == 0.0))) + int(np.sum((w0[other] == 1.0) | (w0[other] == 0.0)))
    return float(conv) / float(total)


def run_model(meas, agent_of_pose, colors, kind, X_hist, inner_iters, w0, fixed=None, params=None, dtype=_L):
    """tests/_robust.run_model from the initial weights w0 (one per edge) with the edges of `fixed` (bool per edge, or
    None) held.  The records are run_model's: w (the responsible copy's weight per edge; odometry at w0), mu, mu_next,
    res (NaN where the iteration left the weight alone, a fixed edge included), ratio, selected."""
    p = dict(RB.DEFAULTS)
    p.update(params or {})
    colors = np.asarray(colors)
    K, C = len(colors), int(max(colors)) + 1
    st = RB.Structure(meas, agent_of_pose, K)
    d = meas.d
    lc = st.lc
    own, shared, nbr_end = st.owner[lc], st.shared[lc], st.nbr_end[lc]
    w0 = np.asarray(w0, dtype)
    fixed = np.zeros(meas.m, bool) if fixed is None else np.asarray(fixed, bool)
    free = ~fixed[lc]
    w = w0.copy()
    held = np.full(K, -1)
    mu, gnc_iter = float(p["gnc_init_mu"]), 0
    ratios = [None] * K
    out = []
    for t in range(1, len(X_hist)):
        c = (t - 1) % C
        sel = colors == c
        held[sel] = t - 1
        rec = dict(mu=None, res=np.full(len(lc), np.nan, _L))
        if kind != "L2" and (t + 1) % inner_iters == 0:
            Xs = X_hist[t - 1]
            h = held[own]
            can = (~shared | (h >= 0)) & free
            P1 = RB._blocks(Xs, meas.p1[lc], d, dtype).copy()
            P2 = RB._blocks(Xs, meas.p2[lc], d, dtype).copy()
            for s in np.unique(h[shared & can]):
                Xh = X_hist[s]
                for end, P, poses in ((0, P1, meas.p1), (1, P2, meas.p2)):
                    pick = np.nonzero(shared & can & (h == s) & (nbr_end == end))[0]
                    P[pick] = RB._blocks(Xh, poses[lc[pick]], d, dtype)
            res = RB.residuals(meas, lc[can], P1[can], P2[can], dtype)
            w[lc[can]] = RB.weight(kind, res, mu, p, dtype)
            rec["res"][can] = res
            rec["mu"] = mu
            if kind == "GNC_TLS":
                gnc_iter += 1
                if gnc_iter <= p["gnc_max_iters"]:
                    mu = p["gnc_mu_step"] * mu
        for a in np.nonzero(sel)[0]:
            ratios[a] = ratio(st, w, w0, fixed, a) if kind == "GNC_TLS" else 1.0
        rec.update(w=w.copy(), mu_next=mu, ratio=list(ratios), selected=held >= 0)
        out.append(rec)
    return out


def oracle_weights_both(agents, meas, agent_of_pose):
    """(responsible copy, other copy) of every edge from the oracle's Agents: odometry and private loop closures appear
    once (the second array repeats them), a shared loop closure with the lower-ID agent's copy first."""
    K = len(agents)
    st = RB.Structure(meas, agent_of_pose, K)
    priv, shared = RB.oracle_edge_lists(meas, agent_of_pose, K)
    odo = [np.nonzero((st.owner < 0) & (st.a1 == a))[0] for a in range(K)]
    w, other = np.full(meas.m, np.nan), np.full(meas.m, np.nan)
    for ag in agents:
        assert ag.odometry.m == len(odo[ag.id])
        w[odo[ag.id]] = other[odo[ag.id]] = ag.odometry.weight
        w[priv[ag.id]] = other[priv[ag.id]] = ag.private_lc.weight
        mine = st.owner[shared[ag.id]] == ag.id
        w[shared[ag.id][mine]] = ag.shared_lc.weight[mine]
        other[shared[ag.id][~mine]] = ag.shared_lc.weight[~mine]
    assert not np.isnan(w).any() and not np.isnan(other).any()
    return w, other
