"""The reference of the set-weights tests, checked on the CPU: tests/_weights.run_model (the reweighting started from
given weights, with known inliers held) against tests/_robust.run_model, against the oracle's Agents on a Measurements
whose `weight` field carries W(d), and its own fixed-edge rule.

Measured here: the model (np.longdouble) against the oracle's float64 Agent weights over 2 C + 1 iterations of GNC_TLS
from W(d): identical exact-0 / exact-1 decisions, max |dw| 2.2e-14 at (3, 5) and 3.3e-14 at (2, 3); the weighted oracle
run ends 0.18 / 0.13 (relative) away from the unit-weight one.
"""
import math

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _robust as RB
from tests import _weights as WT
from tests._common import rel
from tests.test_robust_reference import GNC, oracle_history

K = len(RB.AGENTS)
_cache = {}


def weighted_history(d, r):
    """test_robust_reference.oracle_history with the measurements' weights W(d): (X history, responsible copies'
    weights, other copies' weights, ratios per iteration, colours)."""
    if (d, r) in _cache:
        return _cache[(d, r)]
    meas, aop, T = RB.robust_case(d)
    X0 = O.lifting_matrix(d, r) @ T
    colors = O.greedy_colors(meas, aop, K)
    iters = 2 * (max(colors) + 1) + 1
    hist, ws, others, ratios = [X0.copy()], [], [], []

    def grab(it, agents):
        b = d + 1
        X = np.zeros_like(X0)
        for a, ag in enumerate(agents):
            X[:, np.nonzero(np.repeat(aop == a, b))[0]] = ag.X
        hist.append(X)
        w, other = WT.oracle_weights_both(agents, meas, aop)
        ws.append(w)
        others.append(other)
        ratios.append([ag.converged_loop_closure_ratio() for ag in agents])

    O.colour_rbcd(WT.weighted(meas, WT.W(d)), aop, K, X0, iters, r, acceleration=False, robust="GNC_TLS",
                  robust_opt_inner_iters=1, on_iteration=grab, **GNC)
    _cache[(d, r)] = (hist, ws, others, ratios, colors)
    return _cache[(d, r)]


@pytest.mark.parametrize("d", [3, 2])
def test_weight_recipe(d):
    """W(d): odometry in [0.25, 1), loop closures with exact zeros, exact ones and values between, every one in [0, 1]."""
    meas, aop, _ = RB.robust_case(d)
    st = RB.Structure(meas, aop, K)
    w = WT.W(d)
    assert w.shape == (meas.m,) and np.all((w >= 0) & (w <= 1)) and np.all(w[st.owner < 0] >= 0.25)
    lc = w[st.lc]
    share = [float(np.mean(lc == 0.0)), float(np.mean(lc == 1.0))]
    assert 0.15 <= share[0] <= 0.25 and 0.25 <= share[1] <= 0.35 and np.any((lc > 0) & (lc < 1))
    assert np.any(w[st.shared] == 0.0) and np.any((w[st.shared] > 0) & (w[st.shared] < 1))
    assert np.array_equal(w, WT.W(d))


@pytest.mark.parametrize("d,r", [(3, 5), (2, 3)])
def test_ones_and_no_mask_is_the_robust_model(d, r):
    """Started at ones without a mask the model is tests/_robust.run_model, record by record, bit by bit."""
    meas, aop, _ = RB.robust_case(d)
    hist, _, _, _, colors = oracle_history(d, r)
    a = RB.run_model(meas, aop, colors, "GNC_TLS", hist, 1, GNC)
    b = WT.run_model(meas, aop, colors, "GNC_TLS", hist, 1, np.ones(meas.m), None, GNC)
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra["mu"] == rb["mu"] and ra["mu_next"] == rb["mu_next"]
        assert np.array_equal(ra["w"], rb["w"]) and np.array_equal(ra["res"], rb["res"], equal_nan=True)
        assert np.array_equal(ra["selected"], rb["selected"])
        for x, y in zip(ra["ratio"], rb["ratio"]):
            assert x == y or (x is not None and y is not None and math.isnan(x) and math.isnan(y))


@pytest.mark.parametrize("d,r", [(3, 5), (2, 3)])
def test_weighted_model_matches_oracle_agents(d, r):
    """From W(d) without a mask, on the weighted oracle's own history: the responsible copies within 1e-12 of the
    Agents' after every iteration with the same exact zeros and ones, the other copies and the odometry still what was
    set, the same ratios; and the weights matter -- the run ends far from the unit-weight one."""
    meas, aop, _ = RB.robust_case(d)
    st = RB.Structure(meas, aop, K)
    w0 = WT.W(d)
    hist, ws, others, ratios, colors = weighted_history(d, r)
    C = max(colors) + 1
    model = WT.run_model(meas, aop, colors, "GNC_TLS", hist, 1, w0, None, GNC)
    worst = 0.0
    for t, rec in enumerate(model):
        wm, wo = rec["w"].astype(float), ws[t]
        assert np.array_equal(wo[st.owner < 0], w0[st.owner < 0])  # the oracle honours odometry weights
        assert np.array_equal(others[t][st.shared], w0[st.shared])  # and leaves the higher-ID copy as it was set
        assert np.array_equal(wm == 0.0, wo == 0.0) and np.array_equal(wm == 1.0, wo == 1.0), t
        worst = max(worst, float(np.max(np.abs(rec["w"] - wo.astype(np.longdouble)))))
        for a in range(K):
            if rec["selected"][a] and colors[a] == t % C:
                ro = ratios[t][a]
                assert rec["ratio"][a] == ro or (math.isnan(ro) and math.isnan(rec["ratio"][a])), (t, a)
    moved = rel(hist[-1], oracle_history(d, r)[0][-1])
    print(f"d = {d}: weighted model against the oracle's Agents: max |dw| = {worst:.2e}; X is {moved:.2f} from the "
          f"unit-weight run")
    assert worst <= 1e-12
    assert moved >= 0.1
    assert not np.array_equal(model[-1]["w"][st.lc], w0[st.lc])  # the reweighting did rewrite the set weights


@pytest.mark.parametrize("d,r", [(3, 5), (2, 3)])
def test_fixed_edges_keep_their_weight(d, r):
    """With a mask (every third loop closure and every one touching agent 2) the fixed edges keep their initial weight
    bitwise through every iteration, the free ones are what the unmasked model gives on the same history, agent 2's
    ratio is 0/0 = NaN, and a ratio counts only the free copies."""
    meas, aop, _ = RB.robust_case(d)
    st = RB.Structure(meas, aop, K)
    w0 = WT.W(d)
    fixed = WT.mask(st, meas.m)
    hist, _, _, _, colors = weighted_history(d, r)
    free = WT.run_model(meas, aop, colors, "GNC_TLS", hist, 1, w0, None, GNC)
    held = WT.run_model(meas, aop, colors, "GNC_TLS", hist, 1, w0, fixed, GNC)
    lcf = fixed[st.lc]
    assert lcf.sum() >= len(st.lc) // 3 and (~lcf).sum() >= 100
    for a, b in zip(free, held):
        assert np.array_equal(b["w"][fixed], w0[fixed].astype(np.longdouble))
        assert np.array_equal(b["w"][~fixed], a["w"][~fixed])
        assert np.isnan(b["res"][lcf]).all()
    last = held[-1]["ratio"]
    assert math.isnan(last[WT.MASK_AGENT]) and math.isnan(last[RB.EXTRA_AGENT])
    assert len(st.own_copies[WT.MASK_AGENT]) + len(st.other_copies[WT.MASK_AGENT]) >= 10  # all of them fixed
    finite = [x for x in last if not math.isnan(x)]
    assert len(set(finite)) >= 3
    assert any(x != y for x, y in zip(last, free[-1]["ratio"]) if not math.isnan(x))
