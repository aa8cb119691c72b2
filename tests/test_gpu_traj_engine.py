"""The engine's evaluation against a ground truth (dpgo_rbcd_set_truth / _truth_moments / _truth_errors,
Rbcd.evaluate): a k = 6 grid with 8 agents at r = 5 after a few GNC_TLS iterations, on one rank and on two (both
processes on the one visible GPU, gloo for the halo, the anchor and the moment sums).

The per-pose kernels work pose by pose, so under one Aa the engine's per-pose errors are bitwise hip.traj_errors of
the merged trajectory wherever a pose stands.  The moments are sums over the engine's pose order (agent by agent) and,
with two ranks, over two partial vectors: they agree with the graph-order sums within rounding, not bitwise, as
dpgo_rbcd_gram documents for its partials -- so Aa and the means are compared to 1e-12 relative."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import dpgo_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, A, R, D, ITERS, SEED = 6, 2, 5, 3, 6, 5
REL = 1e-12


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _params(H):
    return H.rbcd_params(r=R, acceleration=1, robust_cost=H.ROBUST["GNC_TLS"], robust_opt_inner_iters=3)


def _mask(n):
    use = (np.random.default_rng(n).uniform(size=n) < 0.8).astype(np.int32)
    use[0] = 1
    return use


@pytest.fixture(scope="module")
def one_rank(hip):
    """(graph, engine after ITERS colour updates, truth), shared and left unchanged by the tests below."""
    g = hip.Graph.grid3d(K, seed=SEED)
    aop = g.grid_partition(A)
    e = hip.Rbcd(g, aop, np.zeros(A ** 3, np.int32), 0, 1, _params(hip))
    e.set_X(g.chain_init(R, O.lifting_matrix(D, R)))
    for it in range(ITERS):
        c = it % e.num_colors
        e.pre_exchange(c)
        e.update(c, None)
    return g, e, g.truth()


def test_truth_calls_need_a_truth(hip, one_rank):
    g, e, truth = one_rank
    e.set_truth(None)
    with pytest.raises(hip.DPGOHipError):
        e.truth_moments()
    tra = np.full(g.n, 7.0)
    with pytest.raises(hip.DPGOHipError):
        e.truth_errors(tra_sq=tra)
    e.set_truth(truth)
    with pytest.raises(hip.DPGOHipError):
        e.truth_errors(sums=False)  # no output
    assert np.all(tra == 7.0)


@pytest.mark.parametrize("masked", [False, True])
def test_truth_errors_bitwise_traj_errors_of_the_trajectory(hip, one_rank, masked):
    g, e, truth = one_rank
    use = _mask(g.n) if masked else None
    e.set_truth(truth, use)
    T = np.full(g.n * (D + 1) * D, np.nan)
    e.trajectory_into(T)
    Aa = np.concatenate([O.project_to_rotation(np.random.default_rng(1).normal(size=(D, D))),
                         np.array([[0.5], [-2.0], [3.0]])], axis=1)
    for M in (None, Aa):
        tra, rot = np.full(g.n, -1.0), np.full(g.n, -1.0)
        s = e.truth_errors(None, M, tra, rot)
        ref = hip.traj_errors(T, truth, D, use, M)
        assert np.array_equal(tra, ref["tra_sq"], equal_nan=True)
        assert np.array_equal(rot, ref["rot_sq"], equal_nan=True)
        assert s[0] == ref["sums"][0] and np.array_equal(s[3:], ref["sums"][3:])
        assert np.all(np.abs(s[1:3] - ref["sums"][1:3]) <= REL * ref["sums"][1:3])
        only = np.full(g.n, -1.0)
        assert e.truth_errors(None, M, None, only, sums=False) is None and np.array_equal(only, rot, equal_nan=True)
    # the moments: the engine's pose order against the graph's, entry by entry within rounding of the terms' size
    shift = np.concatenate([np.zeros(D), np.full(D, 2.5)])
    for sh in (None, shift):
        got = e.truth_moments(None, sh)
        ref = hip.traj_moments(T, truth, D, use, sh)
        scale = np.abs(hip.traj_moments(np.abs(T), np.abs(truth), D, use, None)) + 1.0
        assert got[0] == ref[0] and np.all(np.abs(got - ref) <= 1e-13 * scale), (got, ref)
    e.set_truth(truth)


def test_rbcd_evaluate_equals_graph_evaluate(hip, one_rank):
    g, e, truth = one_rank
    e.set_truth(truth)
    ev = e.evaluate()
    X = np.empty(g.n * (D + 1) * R)
    e.get_X_into(X)
    gv = g.evaluate(X, R, truth, align="lsq", pose=0)
    print(f"ATE rmse {ev['ate_rmse']:.4f} max {ev['ate_max']:.4f}, rot rmse {ev['rot_rmse']:.4f}; "
          f"RPE tra {gv['rpe_tra_rmse']:.4f} rot {gv['rpe_rot_rmse']:.4f}")
    assert ev["count"] == gv["count"] == g.n and ev["rank"] == gv["rank"] == D
    assert np.max(np.abs(ev["Aa"] - gv["Aa"])) <= REL * (1.0 + K)
    for k in ("ate_rmse", "ate_max", "rot_rmse", "rot_max"):
        assert abs(ev[k] - gv[k]) <= REL * gv[k], k
    assert np.all(np.abs(ev["sigma"] - gv["sigma"]) <= REL * gv["sigma"][0])
    # per pose: bitwise under one Aa -- the graph's entry given the engine's trajectory and the engine's Aa
    T = np.full(g.n * (D + 1) * D, np.nan)
    e.trajectory_into(T)
    ref = hip.traj_errors(T, truth, D, None, ev["Aa"])
    assert np.array_equal(ev["tra_sq"], ref["tra_sq"]) and np.array_equal(ev["rot_sq"], ref["rot_sq"])
    # and Graph.evaluate's own per-pose arrays are those of the same trajectory under its Aa
    ref = hip.traj_errors(T, truth, D, None, gv["Aa"])
    assert np.array_equal(gv["tra_sq"], ref["tra_sq"]) and np.array_equal(gv["rot_sq"], ref["rot_sq"])
    # (six colour updates from the odometry chain are far from converged: the figures printed above are large)
    assert gv["edges_used"] == g.m and np.isfinite([gv["rpe_tra_rmse"], gv["rpe_rot_rmse"]]).all()


def test_noise_free_graph_evaluates_to_rounding_level(hip):
    """rot_sigma = trans_sigma = 0 and a start at the truth: the truth satisfies every measurement of the graph on
    the device (which ties dpgo_graph_grid3d_truth to dpgo_graph_grid3d's measurements), and evaluates to rounding
    level against itself through the engine and through the graph."""
    k = 4
    g = hip.Graph.grid3d(k, seed=9, rot_sigma=0.0, trans_sigma=0.0)
    truth = g.truth()
    X = hip.to_dev_layout(O.lifting_matrix(D, R) @ truth)
    res = g.edge_errors(X, R, outputs=("rot_sq", "tra_sq"))
    assert float(np.max(res["rot_sq"])) <= (1e-14) ** 2 and float(np.max(res["tra_sq"])) <= (1e-14 * k) ** 2
    e = hip.Rbcd(g, g.grid_partition(A), np.zeros(A ** 3, np.int32), 0, 1, hip.rbcd_params(r=R))
    e.set_X(X)
    e.set_truth(truth)
    ev = e.evaluate()
    gv = g.evaluate(X, R, truth)
    for v in (ev, gv):
        assert v["ate_max"] <= 1e-13 * k and v["rot_max"] <= 1e-14, (v["ate_max"], v["rot_max"])
    assert gv["rpe_tra_rmse"] <= 1e-14 * k and gv["rpe_rot_rmse"] <= 1e-14


# ---------------------------------------------------------------------------------------- two ranks
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dpgo_amd import hip as H
        g = H.Graph.grid3d(K, seed=SEED)
        aop = g.grid_partition(A)
        ranks = (np.arange(A ** 3) * world // A ** 3).astype(np.int32)
        e = H.Rbcd(g, aop, ranks, rank, world, _params(H))
        e.set_X(g.chain_init(R, O.lifting_matrix(D, R)))
        dev = torch.device("cuda", 0)
        s = torch.cuda.Stream(dev)
        e.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            send = torch.zeros(max(int(e.send_counts.sum()), 1), dtype=torch.float64, device=dev)
            recv = torch.zeros(max(int(e.recv_counts.sum()), 1), dtype=torch.float64, device=dev)
            rsplit = [int(x) for x in e.recv_counts]
            ssplit = [int(x) for x in e.send_counts]
            for it in range(ITERS):
                c = it % e.num_colors
                e.pre_exchange(c)
                e.pack(send.data_ptr())
                hs = send.cpu()
                hr = torch.empty_like(recv, device="cpu")
                dist.all_to_all_single(hr, hs, rsplit, ssplit)
                recv.copy_(hr)
                e.update(c, recv.data_ptr())
            owner = int(ranks[aop[0]])
            a = e.anchor(0)
            at = torch.from_numpy(H.to_dev_layout(a)) if a is not None else torch.empty((D + 1) * R, dtype=torch.float64)
            dist.broadcast(at, src=owner)
            anchor = H.from_dev_layout(at.numpy(), R)
            e.set_truth(g.truth())
            refused = False
            if rank != owner:  # get_trajectory's refusal: without an anchor only the owner of pose 0 defines the frame
                try:
                    e.truth_moments()
                except H.DPGOHipError:
                    refused = True
            # the moments, summed over the ranks between the two launches
            m0 = torch.from_numpy(e.truth_moments(anchor))
            dist.all_reduce(m0)
            m0 = m0.numpy()
            shift = m0[3:3 + 2 * D] / m0[0]
            m1 = torch.from_numpy(e.truth_moments(anchor, shift))
            dist.all_reduce(m1)
            Aa, info = H.align_moments(D, m1.numpy(), shift)
            tra, rot = np.full(g.n, np.nan), np.full(g.n, np.nan)
            sums = e.truth_errors(anchor, Aa, tra, rot)
        q.put((rank, tra, rot, sums, Aa, info["rank"], rank == owner or refused))
    finally:
        dist.destroy_process_group()


def test_two_ranks_merge_to_the_one_rank_engine(hip, one_rank):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=240) for _ in range(2)], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=60)
    assert all(o[6] for o in outs)
    g, e1, truth = one_rank
    aop = g.grid_partition(A)
    ranks = np.arange(A ** 3) * 2 // A ** 3
    # both ranks hold the same alignment (the summed moments are the same bits on both)
    assert np.array_equal(outs[0][4], outs[1][4]) and outs[0][5] == outs[1][5] == D
    Aa = outs[0][4]
    # every pose by exactly one rank: the rank of its agent
    wr = [~np.isnan(o[1]) for o in outs]
    assert np.all(wr[0].astype(int) + wr[1].astype(int) == 1)
    assert np.array_equal(wr[1], ranks[aop] == 1)
    assert all(np.array_equal(~np.isnan(o[2]), w) for o, w in zip(outs, wr))
    tra = np.where(wr[0], outs[0][1], outs[1][1])
    rot = np.where(wr[0], outs[0][2], outs[1][2])
    # merged per-pose errors: bitwise the one-rank engine's under the same Aa
    e1.set_truth(truth)
    tra1, rot1 = np.full(g.n, np.nan), np.full(g.n, np.nan)
    s1 = e1.truth_errors(None, Aa, tra1, rot1)
    assert np.array_equal(tra, tra1) and np.array_equal(rot, rot1)
    merged = hip.merge_traj_sums([o[3] for o in outs])
    assert merged[0] == s1[0] == g.n and np.array_equal(merged[3:], s1[3:])
    ate2, ate1 = np.sqrt(merged[1] / merged[0]), np.sqrt(s1[1] / s1[0])
    assert abs(ate2 - ate1) <= REL * ate1 and abs(merged[2] - s1[2]) <= REL * s1[2]
    # and the alignment is the one-rank engine's own within rounding
    ev = e1.evaluate()
    assert np.max(np.abs(ev["Aa"] - Aa)) <= REL * (1.0 + K)
    assert abs(ev["ate_rmse"] - ate2) <= REL * ate1
