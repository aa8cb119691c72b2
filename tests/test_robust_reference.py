"""The references of the robust-reweighting tests, checked on the CPU: RobustCost.weight against closed forms, the
host model of tests/_robust.py against the oracle's Agents (two independent restatements of
src/PGOAgent.cpp:1174-1289), and every property of the 650-pose case that tests/test_gpu_robust.py relies on.

Measured here: host model (np.longdouble) against the oracle's float64 Agent weights over 2 C + 1 = 11 iterations of
GNC_TLS (barc 0.6, mu 0.05 x 3, capped after 3 updates): 3.6e-14 at (3, 5), 2.4e-14 at (2, 3), identical exact-0 / exact-1
decisions, mu and ratios.  Branch shares of the 944 reweighted loop closures at the lifted ground truth with barc 0.6,
mu = 1 (w = 1 / middle / w = 0): 24.7 / 56.8 / 18.5 % at d = 3, 59.1 / 28.8 / 12.1 % at d = 2.  Smallest relative distance of a
residual from a branch threshold over every compiled rank, GNC at mu in {0.05, 0.15, 0.45, 1.35, 1}, Huber 0.6 and TLS 0.8:
2.4e-4 at d = 3, 3.8e-5 at d = 2.
"""
import math

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _robust as RB

GNC = dict(gnc_barc=0.6, gnc_init_mu=0.05, gnc_mu_step=3.0, gnc_max_iters=3)
MUS = [0.05, 0.15, 0.45, 1.35]

_cache = {}


def _colors(d):
    meas, aop, _ = RB.robust_case(d)
    return O.greedy_colors(meas, aop, len(RB.AGENTS))


def oracle_history(d, r):
    """GNC_TLS with robust_opt_inner_iters = 1 over 2 C + 1 iterations without acceleration: (X history, the Agents'
    weights under the owner rule after every iteration, ratio and ready per agent after every iteration, colours)."""
    if (d, r) in _cache:
        return _cache[(d, r)]
    meas, aop, T = RB.robust_case(d)
    X0 = O.lifting_matrix(d, r) @ T
    colors = _colors(d)
    iters = 2 * (max(colors) + 1) + 1
    hist, ws, ratios, mus = [X0.copy()], [], [], []

    def grab(it, agents):
        b = d + 1
        X = np.zeros_like(X0)
        for a, ag in enumerate(agents):
            X[:, np.nonzero(np.repeat(aop == a, b))[0]] = ag.X
        hist.append(X)
        ws.append(RB.oracle_weights(agents, meas, aop))
        ratios.append([ag.converged_loop_closure_ratio() for ag in agents])
        mus.append([ag.robust.mu for ag in agents])

    O.colour_rbcd(RB.fresh(meas), aop, len(RB.AGENTS), X0, iters, r, acceleration=False, robust="GNC_TLS",
                  robust_opt_inner_iters=1, on_iteration=grab, **GNC)
    _cache[(d, r)] = (hist, ws, ratios, mus, colors)
    return _cache[(d, r)]


# ------------------------------------------------------------------------------------------ RobustCost.weight
def test_weight_closed_forms():
    """All six costs with non-default parameters against the formulas of src/DPGO_robust.cpp:23-67 written out."""
    rs = [1e-3, 0.3, 0.59, 0.6, 0.61, 0.8, 0.81, 2.5, 40.0]
    assert all(O.RobustCost("L2").weight(x) == 1.0 for x in rs)
    assert all(O.RobustCost("L1").weight(x) == 1.0 / x for x in rs)
    hub = O.RobustCost("Huber", huber=0.6)
    assert [hub.weight(x) for x in rs] == [1.0, 1.0, 1.0, 0.6 / 0.6, 0.6 / 0.61, 0.6 / 0.8, 0.6 / 0.81, 0.6 / 2.5,
                                            0.6 / 40.0]
    assert hub.weight(np.nextafter(0.6, 0)) == 1.0 and hub.weight(0.6) == 1.0  # r < threshold, and h / h at it
    tls = O.RobustCost("TLS", tls=0.8)
    assert [tls.weight(x) for x in rs] == [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]  # r < 0.8 strictly
    assert tls.weight(np.nextafter(0.8, 0)) == 1.0
    gm = O.RobustCost("GM")
    # 1 / (1 + r^2)^2 in np.longdouble; the float64 evaluation rounds four times
    assert all(abs(gm.weight(x) - float(1 / (1 + np.longdouble(x) ** 2) ** 2)) <= 4 * np.finfo(float).eps * gm.weight(x)
               for x in rs)
    # the defaults still are the reference's (include/DPGO/DPGO_robust.h)
    assert O.RobustCost("GNC_TLS").p == dict(max_iters=100, barc=10.0, mu_step=1.4, init_mu=1e-4, huber=3.0, tls=10.0)
    assert O.AgentParams(3, 5).robust_params == RB.DEFAULTS
    # the model's vectorised weight is the same function
    for kind in ("L1", "Huber", "TLS", "GM", "GNC_TLS"):
        c = O.RobustCost(kind, gnc_barc=0.6, gnc_init_mu=0.45, huber=0.6, tls=0.8)
        got = RB.weight(kind, np.array(rs), 0.45, dict(RB.DEFAULTS, gnc_barc=0.6, huber=0.6, tls=0.8), np.float64)
        assert np.array_equal(got, np.array([c.weight(x) for x in rs])), kind


@pytest.mark.parametrize("mu", [1e-4] + MUS)
@pytest.mark.parametrize("barc", [0.6, 10.0])
def test_gnc_branches_continuous_and_closed_form(mu, barc):
    """GNC_TLS: w = 1 up to r^2 = mu / (mu + 1) barc^2, w = 0 from (mu + 1) / mu barc^2, barc sqrt(mu (mu + 1)) / r - mu
    between; the middle formula meets both limits (continuity), to a few ulps of its largest term."""
    c = O.RobustCost("GNC_TLS", gnc_barc=barc, gnc_init_mu=mu)
    lo, hi = math.sqrt(mu / (mu + 1)) * barc, math.sqrt((mu + 1) / mu) * barc
    eps = 1e-9
    assert c.weight(lo * (1 - eps)) == 1.0 and c.weight(hi * (1 + eps)) == 0.0
    tol = 8 * np.finfo(float).eps * (1 + mu)
    assert 0 <= 1.0 - c.weight(lo * (1 + eps)) <= 2 * eps * (1 + mu) + tol
    assert 0 <= c.weight(hi * (1 - eps)) <= 2 * eps * (1 + mu) + tol
    for x in np.linspace(lo * 1.01, hi * 0.99, 7):
        assert abs(c.weight(x) - (barc * math.sqrt(mu * (mu + 1)) / x - mu)) <= tol
    ws = [c.weight(x) for x in np.linspace(lo * 0.5, hi * 1.5, 200)]
    assert all(a >= b for a, b in zip(ws[:-1], ws[1:])) and ws[0] == 1.0 and ws[-1] == 0.0  # monotone


def test_mu_schedule_and_cap():
    """RobustCost::update: mu is multiplied by mu_step at each of the first gnc_max_iters updates and then stays; the
    other costs have no state."""
    c = O.RobustCost("GNC_TLS", **GNC)
    seen = []
    for _ in range(6):
        seen.append(c.mu)
        c.update()
    assert seen == [0.05, 0.05 * 3.0, 0.05 * 3.0 * 3.0, 0.05 * 3.0 * 3.0 * 3.0] + [0.05 * 3.0 * 3.0 * 3.0] * 2
    assert np.allclose(seen[:4], MUS, rtol=1e-15)
    c.reset()
    assert c.mu == 0.05 and c.iteration == 0
    one = O.RobustCost("GNC_TLS", gnc_init_mu=0.45, gnc_mu_step=3.0, gnc_max_iters=1)
    one.update(); one.update()
    assert one.mu == 0.45 * 3.0
    h = O.RobustCost("Huber", huber=0.6)
    h.update()
    assert h.iteration == 0


# ------------------------------------------------------------------------------------------ the case
@pytest.mark.parametrize("d", [3, 2])
def test_case_structure(d):
    """The 650-pose case: the ragged engine case untouched, an eighth agent without loop closures in a component of
    its own, a shared loop closure whose owner is not of colour 0."""
    from tests import test_gpu_ragged as TG
    meas, aop, T = RB.robust_case(d)
    m0, aop0, X0 = TG.engine_case(d, 3, "GNC_TLS")
    assert RB.ENGINE_AGENTS == TG.ENGINE_AGENTS and meas.num_poses == RB.N_POSES == 650
    k = m0.m
    for f in ("p1", "p2", "R", "t", "kappa", "tau"):
        assert np.array_equal(getattr(meas, f)[:k], getattr(m0, f)), f
    assert np.array_equal(aop[:m0.num_poses], aop0)
    assert np.array_equal(O.lifting_matrix(d, 3) @ T[:, :X0.shape[1]], X0)
    st = RB.Structure(meas, aop, len(RB.AGENTS))
    x = RB.EXTRA_AGENT
    assert np.all(aop[meas.p1[k:]] == x) and np.all(aop[meas.p2[k:]] == x) and meas.m - k == RB.EXTRA_POSES - 1
    assert not np.any((aop[meas.p1[:k]] == x) | (aop[meas.p2[:k]] == x))
    assert np.all(st.owner[k:] == -1)
    assert len(st.own_copies[x]) == 0 and len(st.other_copies[x]) == 0  # zero loop closures
    assert math.isnan(st.ratio(np.ones(meas.m), x))
    colors = _colors(d)
    assert colors[x] == 0 and max(colors) + 1 >= 3
    late = st.shared & (np.asarray(colors)[np.maximum(st.owner, 0)] != 0)
    assert int(late.sum()) >= 10  # dict_ok == 0 at the first reweighting
    assert int((st.shared & ~late).sum()) >= 10 and int((~st.shared & (st.owner >= 0)).sum()) >= 100
    # the model's lists are the oracle's split
    parts = O._split(meas, aop, st_local(aop), len(RB.AGENTS))
    priv, shared = RB.oracle_edge_lists(meas, aop, len(RB.AGENTS))
    for a in range(len(RB.AGENTS)):
        assert parts[a][1].m == len(priv[a]) and parts[a][2].m == len(shared[a])
        assert np.array_equal(parts[a][1].kappa, meas.kappa[priv[a]])
        assert np.array_equal(parts[a][2].kappa, meas.kappa[shared[a]])


def st_local(aop):
    local = np.zeros(len(aop), np.int64)
    seen = {}
    for i, a in enumerate(aop):
        local[i] = seen.get(int(a), 0)
        seen[int(a)] = local[i] + 1
    return local


@pytest.mark.parametrize("d,want", [(3, (25, 57, 18)), (2, (59, 29, 12))])
def test_branch_shares_at_ground_truth(d, want):
    """barc 0.6, mu = 1 at the lifted ground truth: each GNC branch holds >= 10 % of the reweighted loop closures."""
    meas, aop, T = RB.robust_case(d)
    st = RB.Structure(meas, aop, len(RB.AGENTS))
    X0 = O.lifting_matrix(d, d + 2) @ T
    br = RB.gnc_branch(RB.residuals_at(meas, st, X0), 1.0, dict(RB.DEFAULTS, gnc_barc=0.6))
    share = [100.0 * float(np.mean(br == k)) for k in range(3)]
    print(f"d = {d}: w = 1 / middle / w = 0: {share[0]:.1f} / {share[1]:.1f} / {share[2]:.1f} % of {len(st.lc)}")
    assert min(share) >= 10.0
    assert all(abs(s - w_) <= 1.0 for s, w_ in zip(share, want))  # the figures the docstrings quote


@pytest.mark.parametrize("d", [3, 2])
def test_no_residual_on_a_threshold(d):
    """No residual at the lifted ground truth lies within 1e-9 (relative) of a branch threshold of any cost the GPU
    tests run there, at every compiled rank (the lift is an isometry, so the residuals of two ranks differ by the
    rounding of X0 alone: asserted at 1e-11)."""
    meas, aop, T = RB.robust_case(d)
    st = RB.Structure(meas, aop, len(RB.AGENTS))
    p = dict(RB.DEFAULTS, gnc_barc=0.6, huber=0.6, tls=0.8)
    first, smallest = None, np.inf
    for r in range(d, 9):
        res = RB.residuals_at(meas, st, O.lifting_matrix(d, r) @ T)
        first = res if first is None else first
        assert float(np.max(np.abs(res - first) / first)) <= 1e-11
        gaps = [RB.branch_gap("GNC_TLS", res, mu, p).min() for mu in MUS + [1.0]]
        gaps += [RB.branch_gap("Huber", res, None, p).min(), RB.branch_gap("TLS", res, None, p).min()]
        smallest = min(smallest, min(gaps))
        assert float(res.min()) > 1e-3  # L1's 1 / r is tame
    print(f"d = {d}: smallest relative distance from a threshold {smallest:.2e}")
    assert smallest > 1e-9
    assert np.isinf(RB.branch_gap("GM", first, None, p)).all()


# ------------------------------------------------------------------------------------------ model against the oracle
@pytest.mark.parametrize("d,r", [(3, 5), (2, 3)])
def test_host_model_matches_oracle_agents(d, r):
    """The model on the oracle's own X history: weights within 1e-12 of the Agents' after every iteration, the same
    exact zeros and ones, the same mu, the same converged ratios -- and the history does what the GPU tests need of it:
    the cap is reached, stale poses are used, three branches at the end, at least three distinct ratios."""
    meas, aop, _ = RB.robust_case(d)
    hist, ws, ratios, mus, colors = oracle_history(d, r)
    C = max(colors) + 1
    T = len(hist) - 1
    assert T == 2 * C + 1
    model = RB.run_model(meas, aop, colors, "GNC_TLS", hist, 1, GNC)
    st = RB.Structure(meas, aop, len(RB.AGENTS))
    worst = 0.0
    for t in range(T):
        rec, wo = model[t], ws[t]
        assert rec["mu"] == ([0.05, 0.05 * 3.0, 0.05 * 3.0 * 3.0] + [0.05 * 3.0 * 3.0 * 3.0] * T)[t]
        assert all(m == rec["mu_next"] for m in mus[t])
        wm = rec["w"].astype(float)
        assert np.array_equal(wm == 0.0, wo == 0.0) and np.array_equal(wm == 1.0, wo == 1.0), t
        worst = max(worst, float(np.max(np.abs(rec["w"] - wo.astype(np.longdouble)))))
        gap = RB.branch_gap("GNC_TLS", rec["res"], rec["mu"], dict(RB.DEFAULTS, **GNC))
        assert np.nanmin(gap) > 1e-9, (t, np.nanmin(gap))
        for a in range(len(RB.AGENTS)):
            if rec["selected"][a]:  # the model's ratio is the one of the agent's last selection; weights of a
                # non-selected agent move on, so compare at the iterations that select it
                if colors[a] == t % C:
                    ro = ratios[t][a]
                    assert rec["ratio"][a] == ro or (math.isnan(ro) and math.isnan(rec["ratio"][a])), (t, a)
    print(f"d = {d}: host model against the oracle's Agents over {T} iterations: max |dw| = {worst:.2e}")
    assert worst <= 1e-12
    # while an owner of another colour has not been selected its shared loop closures stay at exactly 1
    col = np.asarray(colors)
    late = np.nonzero(st.shared & (col[np.maximum(st.owner, 0)] != 0))[0]
    assert np.all(model[0]["w"][late] == 1.0) and np.isnan(model[0]["res"][np.isin(st.lc, late)]).all()
    assert not np.isnan(model[C - 1]["res"]).any()
    # the last iteration: all three branches, and the stale poses matter (a model that always read the newest
    # neighbour pose would differ by more than the bar)
    last = model[-1]
    br = RB.gnc_branch(last["res"], last["mu"], dict(RB.DEFAULTS, **GNC))
    share = [float(np.mean(br == k)) for k in range(3)]
    print(f"    final branches {share[0]:.2f} / {share[1]:.2f} / {share[2]:.2f}")
    assert min(share) >= 0.05
    newest = RB.weight("GNC_TLS", RB.residuals_at(meas, st, hist[T - 1]), last["mu"], dict(RB.DEFAULTS, **GNC))
    assert float(np.max(np.abs(newest - last["w"][st.lc]))) > 1e-6
    final = [x for x in last["ratio"] if x is not None and not math.isnan(x)]
    assert all(x is not None for x in last["ratio"]) and math.isnan(last["ratio"][RB.EXTRA_AGENT])
    print("    ratios", ["%.4f" % x for x in final])
    assert len(set(final)) >= 3
    assert len(RB.thresholds_from(last["ratio"])) >= 2 * len(set(final)) + 1
