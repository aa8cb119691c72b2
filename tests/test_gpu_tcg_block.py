"""Blocked queueing of the merged tCG loop (tuning keys TUNE_TCG_BLOCK = 16, target tiles per block of consecutive
agents, and TUNE_TCG_BLOCK_STREAMS = 17, blocks in flight): a block runs all its tCG iterations before its stream's next
block starts.  Only which agents a launch covers and the order the launches are queued in change, and nothing inside
the tCG loop couples two agents of a colour, so iterates, counters, traces and status are bitwise those of the keys off.

Every case runs the engine with TUNE_TCG_LOOKAHEAD (key 7) = 2, the queued-at-once path the blocks apply to, with the
trace on, and compares X, stats(), every agent's trace and status() with np.array_equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY_FIRST_STEP, KEY_LOOKAHEAD, KEY_TAIL_FUSE, KEY_BLOCK, KEY_STREAMS = 4, 7, 14, 16, 17
# dpgo_hip_stats columns
ST_RUNS, ST_TCG_ITERS, ST_EXCREGION, ST_LCON, ST_SCON, ST_MAXITER, ST_CG_STEPS = 2, 3, 5, 6, 7, 8, 10


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _greedy(tiles, target):
    """Block sizes (agents) of the greedy rule: consecutive agents while the block stays within `target` tiles, at
    least one agent per block; [] when the whole batch fits in one block (the unblocked queueing)."""
    if target <= 0 or len(tiles) < 2 or sum(tiles) <= target:
        return []
    sizes, cur = [1], int(tiles[0])
    for t in tiles[1:]:
        if cur + int(t) > target:
            sizes.append(1)
            cur = int(t)
        else:
            sizes[-1] += 1
            cur += int(t)
    return sizes


def _run(hip, g, aop, X0, iters, keys, params=None, timing=False):
    """`iters` engine iterations with the process tuning defaults `keys` (restored afterwards).  Returns X, stats,
    the traces, status, the stats after every update, the blocks every update was queued in and the agents' tile
    counts per colour, and the per-mode kernel times when asked for."""
    K = int(aop.max()) + 1
    saved = {k: hip.get_tuning(k) for k in keys}
    try:
        for k, v in keys.items():
            hip.set_tuning(k, v)
        e = hip.Rbcd(g, aop, np.zeros(K, np.int32), 0, 1, hip.rbcd_params(**(params or dict(r=5, acceleration=1))))
        e.set_trace(1024)
        e.set_X(X0)
        if timing:
            e.set_kernel_timing(1)
        per_update, blocks = [], []
        for it in range(iters):
            c = it % e.num_colors
            e.pre_exchange(c)
            e.update(c, None)
            per_update.append(e.stats().copy())
            blocks.append(e.tcg_blocks(c)[0])
        X = np.zeros(X0.size)
        e.get_X_into(X)
        out = dict(X=X, stats=e.stats().copy(), trace=[e.get_trace(a) for a in range(K)], status=e.status(),
                   per_update=per_update, blocks=blocks, tiles=[e.tcg_blocks(c)[1].copy() for c in range(e.num_colors)],
                   colors=np.array(e.color_of_agent).copy(), num_colors=e.num_colors)
        if timing:
            out["ktimes"] = e.kernel_times(batch_equiv=True)
        return out
    finally:
        for k, v in saved.items():
            hip.set_tuning(k, v)


def _assert_bitwise(ref, o):
    assert np.array_equal(ref["X"], o["X"])
    assert np.array_equal(ref["stats"], o["stats"])
    for a, b in zip(ref["per_update"], o["per_update"]):
        assert np.array_equal(a, b)
    assert len(ref["trace"]) == len(o["trace"])
    for ta, tb in zip(ref["trace"], o["trace"]):
        assert len(ta) == len(tb)
        for x, y in zip(ta, tb):  # dicts of floats; NaN fields are written as NaN by both
            assert list(x) == list(y)
            assert np.array_equal(np.array(list(x.values())), np.array(list(y.values())), equal_nan=True)
    assert np.array_equal(ref["status"][0], o["status"][0], equal_nan=True)
    assert np.array_equal(ref["status"][1], o["status"][1])


def _assert_blocked(o, target, expect_sizes=None):
    """The blocked path ran (in every update that queued its tCG at once) with the greedy rule's blocks, and CG steps
    were taken."""
    want = [len(_greedy(o["tiles"][c], target)) for c in range(o["num_colors"])]
    assert all(w >= 2 for w in want), want
    if expect_sizes is not None:
        assert [_greedy(o["tiles"][c], target) for c in range(o["num_colors"])] == expect_sizes
    used = [b for b in o["blocks"] if b > 0]
    assert used, "the blocked path never ran"
    for it, b in enumerate(o["blocks"]):
        assert b in (0, want[it % o["num_colors"]]), (it, b, want)
    assert o["stats"][:, ST_CG_STEPS].sum() > 0


@pytest.fixture(scope="module")
def eight(hip):
    """grid3d(12) in 8 agents, 4 per colour; the start and the keys-off run the cases compare against."""
    g = hip.Graph.grid3d(12, seed=5)
    aop = g.grid_partition(2)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    ref = _run(hip, g, aop, X0, 40, {KEY_LOOKAHEAD: 2, KEY_BLOCK: 0})
    assert all(b == 0 for b in ref["blocks"])
    assert ref["num_colors"] == 2 and all(len(t) == 4 for t in ref["tiles"])
    return g, aop, X0, ref


@pytest.mark.parametrize("streams", [1, 2, 3])
@pytest.mark.parametrize("agents_per_block", [1, 2, 3, 4])
def test_block_bitwise_8_agents(hip, eight, agents_per_block, streams):
    """One, two and three (ragged: 3 + 1) agents per block, and a target of the colour's whole tile count, which must
    take the unblocked path; each on 1, 2 and 3 streams."""
    g, aop, X0, ref = eight
    tiles = ref["tiles"]
    assert all(len(set(t.tolist())) == 1 for t in tiles) and tiles[0][0] == tiles[1][0]  # equal agents
    target = agents_per_block * int(tiles[0][0])
    o = _run(hip, g, aop, X0, 40, {KEY_LOOKAHEAD: 2, KEY_BLOCK: target, KEY_STREAMS: streams})
    _assert_bitwise(ref, o)
    if agents_per_block == 4:
        assert target >= int(tiles[0].sum())
        assert all(b == 0 for b in o["blocks"])  # the unblocked path
        assert o["stats"][:, ST_CG_STEPS].sum() > 0
    else:
        _assert_blocked(o, target, [{1: [1, 1, 1, 1], 2: [2, 2], 3: [3, 1]}[agents_per_block]] * 2)


@pytest.mark.parametrize("target,sizes", [(4, [[4, 4, 4, 2], [4, 4, 4, 1]]), (3, [[3, 3, 3, 3, 2], [3, 3, 3, 3, 1]])])
def test_block_bitwise_27_agents(hip, target, sizes):
    """27 agents of one tile each in colours of 14 and 13 agents (unequal tile counts): ragged last blocks of two
    agents and of one agent, more blocks than streams."""
    g = hip.Graph.grid3d(12, seed=0)
    aop = g.grid_partition(3)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    ref = _run(hip, g, aop, X0, 40, {KEY_LOOKAHEAD: 2, KEY_BLOCK: 0})
    assert sorted(len(t) for t in ref["tiles"]) == [13, 14]
    if len(ref["tiles"][0]) == 13:
        sizes = sizes[::-1]
    o = _run(hip, g, aop, X0, 40, {KEY_LOOKAHEAD: 2, KEY_BLOCK: target, KEY_STREAMS: 3})
    _assert_bitwise(ref, o)
    _assert_blocked(o, target, sizes)


@pytest.mark.parametrize("tail_fuse", [0, 1])
def test_block_bitwise_tail_fusion(hip, eight, tail_fuse):
    """With the last iteration's k_tcg_updir launched (0) and left to the retraction (1, every block's last step
    pending until the unsplit retraction)."""
    g, aop, X0, ref = eight
    target = 2 * int(ref["tiles"][0][0])
    base = _run(hip, g, aop, X0, 40, {KEY_LOOKAHEAD: 2, KEY_BLOCK: 0, KEY_TAIL_FUSE: tail_fuse})
    o = _run(hip, g, aop, X0, 40, {KEY_LOOKAHEAD: 2, KEY_BLOCK: target, KEY_STREAMS: 2, KEY_TAIL_FUSE: tail_fuse})
    _assert_bitwise(base, o)
    _assert_blocked(o, target)


def test_block_per_launch_timing(hip, eight):
    """With HIP events around every SpMM launch: the sub-launches of a mode add up to the unblocked run's full-batch
    launch equivalents (tile counts are summed as integers, so exactly), and the results stay bitwise."""
    g, aop, X0, ref = eight
    target = int(ref["tiles"][0][0])
    base = _run(hip, g, aop, X0, 40, {KEY_LOOKAHEAD: 2, KEY_BLOCK: 0}, timing=True)
    o = _run(hip, g, aop, X0, 40, {KEY_LOOKAHEAD: 2, KEY_BLOCK: target, KEY_STREAMS: 2}, timing=True)
    _assert_bitwise(ref, base)
    _assert_bitwise(ref, o)
    _assert_blocked(o, target)
    assert set(base["ktimes"]) == set(o["ktimes"]) and "HESS_M" in o["ktimes"]
    for m, (_, n, eq) in base["ktimes"].items():
        assert eq == round(eq) and 0 < eq <= n, (m, n, eq)  # whole batches (the unblocked run: halves on two streams)
        assert o["ktimes"][m][2] == eq, (m, o["ktimes"][m], eq)
    assert o["ktimes"]["HESS_M"][1] > base["ktimes"]["HESS_M"][1]  # more, smaller launches


def test_block_bitwise_gnc_tls(hip):
    """GNC_TLS on a grid with 10 % corrupted loop closures, run past the reweighting after 30 iterations (Q and G
    rebuilt, the acceleration restarted)."""
    g0 = hip.Graph.grid3d(12, seed=5)
    a = g0.arrays()
    p1, p2 = a["p1"].astype(np.int64), a["p2"].astype(np.int64)
    t = a["t"].copy()
    rng = np.random.default_rng(7)
    lc = np.nonzero(np.abs(p2 - p1) != 1)[0]
    bad = rng.choice(lc, size=len(lc) // 10, replace=False)
    t[bad] += rng.normal(0.0, 5.0, size=(len(bad), 3))
    g = hip.Graph.from_arrays(3, g0.n, p1, p2, a["R"].copy(), t, a["kappa"], a["tau"])
    aop = g0.grid_partition(2)
    X0 = g0.chain_init_dev_layout(5, hip.lifting_matrix(3, 5))  # odometry edges are uncorrupted
    params = dict(r=5, acceleration=1, robust_cost=hip.ROBUST["GNC_TLS"])
    assert hip.rbcd_params(**params).robust_opt_inner_iters == 30
    ref = _run(hip, g, aop, X0, 44, {KEY_LOOKAHEAD: 2, KEY_BLOCK: 0}, params=params)
    target = 2 * int(ref["tiles"][0][0])
    o = _run(hip, g, aop, X0, 44, {KEY_LOOKAHEAD: 2, KEY_BLOCK: target, KEY_STREAMS: 2}, params=params)
    _assert_bitwise(ref, o)
    _assert_blocked(o, target)
    assert any(b > 0 for b in o["blocks"][31:]), "no blocked update after the reweighting"


def test_block_agents_stop_early(hip, eight):
    """Agents whose tCG stops before MAXITER while others of the same block go on: the stopped agents skip their
    tiles inside the block's later launches.  The first updates from the distributed initialisation are of that kind
    (linear-convergence exits after 7 to 9 iterations beside agents that run all 10); the per-update counters must
    show such a mix inside one block of an update the blocked path ran."""
    g, aop, X0, ref = eight
    target = 2 * int(ref["tiles"][0][0])
    o = _run(hip, g, aop, X0, 40, {KEY_LOOKAHEAD: 2, KEY_BLOCK: target, KEY_STREAMS: 2})
    _assert_bitwise(ref, o)
    _assert_blocked(o, target, [[2, 2], [2, 2]])
    max_inner = 10  # tr_max_inner of the engine's Runs (stats: the tCG iterations of a MAXITER exit)
    mixed = 0
    prev = np.zeros_like(o["per_update"][0])
    for it, st in enumerate(o["per_update"]):
        d = st - prev
        prev = st
        agents = np.nonzero(o["colors"] == it % o["num_colors"])[0]  # batch order: the colour's agents ascending
        if o["blocks"][it] == 0 or np.any(d[agents, ST_RUNS] != 1):
            continue
        for b0 in range(0, len(agents), 2):
            blk = agents[b0:b0 + 2]
            full = (d[blk, ST_MAXITER] == 1) & (d[blk, ST_TCG_ITERS] == max_inner)
            early = (d[blk, ST_EXCREGION] + d[blk, ST_LCON] + d[blk, ST_SCON] == 1) & (d[blk, ST_TCG_ITERS] < max_inner)
            mixed += int(full.any() and early.any())
    assert mixed > 0, "no block with both an early exit and a MAXITER exit"
