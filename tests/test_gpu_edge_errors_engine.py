"""Edge errors out of the RBCD engine (dpgo_rbcd_get_errors / Rbcd.errors_into): on one rank bitwise the whole-graph
Graph.edge_errors of the engine's own X and of its rounded trajectory; on two ranks (both processes on the one
visible GPU, gloo for the halo and the anchor, the harness of tests/test_gpu_readout_multirank.py) every edge written
by exactly the rank dpgo_rbcd_weight_owner names, and the merged arrays bitwise the one-rank engine's -- the rounded
ones too, though only lifted poses were exchanged."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import dpgo_oracle as O
from tests._common import load_meas

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, A, R, D, ITERS = 6, 2, 5, 3, 6


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _params(H):
    return H.rbcd_params(r=R, acceleration=1, robust_cost=H.ROBUST["GNC_TLS"], robust_opt_inner_iters=3)


# ---------------------------------------------------------------------------------------- one rank
@pytest.fixture(scope="module")
def small(hip):
    """smallGrid3D, 5 agents, GNC_TLS reweighting every 3 iterations, six iterations: (graph, engine, flat X)."""
    meas = load_meas("smallGrid3D")
    d, n = meas.d, meas.num_poses
    assert d == D
    g = hip.Graph.from_arrays(d, n, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    aop = np.minimum(np.arange(n) // (n // 5), 4).astype(np.int32)
    e = hip.Rbcd(g, aop, np.zeros(5, np.int32), 0, 1, _params(hip))
    e.set_X(O.lifting_matrix(d, R) @ O.chordal_initialization(d, n, meas))
    for it in range(ITERS):
        e.pre_exchange(it % e.num_colors)
        e.update(it % e.num_colors, None)
    X = np.full(n * (d + 1) * R, np.nan)
    e.get_X_into(X)
    return g, e, X


def test_one_rank_lifted_is_the_whole_graph_call(hip, small):
    g, e, X = small
    err, rot, tra = (np.full(g.m, np.nan) for _ in range(3))
    e.errors_into(err, rot_sq=rot, tra_sq=tra)
    assert np.isfinite(err).all() and np.isfinite(rot).all() and np.isfinite(tra).all()  # every edge written
    whole = g.edge_errors(X, R)
    assert np.array_equal(err, whole["err"])
    assert np.array_equal(rot, whole["rot_sq"]) and np.array_equal(tra, whole["tra_sq"])
    only_rot = np.full(g.m, np.nan)
    e.errors_into(None, rot_sq=only_rot)
    assert np.array_equal(only_rot, rot)
    with pytest.raises(hip.DPGOHipError):
        e.errors_into(None)
    again = np.full(g.m, np.nan)
    e.errors_into(again)
    assert np.array_equal(again, err)


def test_one_rank_rounded_is_the_trajectory_s_errors(hip, small):
    g, e, X = small
    d = g.d
    T = np.full(g.n * (d + 1) * d, np.nan)
    e.trajectory_into(T)
    err = np.full(g.m, np.nan)
    e.errors_into(err, rounded=True)
    assert np.isfinite(err).all()
    assert np.array_equal(err, g.edge_errors(T, d)["err"])
    # an explicit anchor that is not pose 0
    anchor = e.anchor(17)
    assert anchor is not None
    T17 = np.full_like(T, np.nan)
    e.trajectory_into(T17, anchor=anchor)
    assert not np.array_equal(T17, T)
    err17 = np.full(g.m, np.nan)
    e.errors_into(err17, rounded=True, anchor=anchor)
    assert np.array_equal(err17, g.edge_errors(T17, d)["err"])
    # the use the feature is for: the cost the robust run minimised, next to the unit-weight one
    w = np.full(g.m, np.nan)
    e.weights_into(w)
    weighted, unit = np.dot(w, err) / 2, np.sum(err) / 2
    assert np.isfinite(weighted) and np.all((w >= 0) & (w <= 1))
    assert np.any(w < 1.0), "no weight left 1: the reweighting did not act on this run"
    assert weighted < unit
    assert abs(g.edge_errors(T, d, w=w)["cost"] - weighted) <= 1e-12 * weighted


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
        g = H.Graph.grid3d(K, seed=5)
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

            def exchange():
                e.pack(send.data_ptr())
                hs = send.cpu()
                hr = torch.empty_like(recv, device="cpu")
                dist.all_to_all_single(hr, hs, rsplit, ssplit)
                recv.copy_(hr)

            for it in range(ITERS):
                c = it % e.num_colors
                e.pre_exchange(c)
                exchange()
                e.update(c, recv.data_ptr())
            exchange()  # the public poses after the last update: what the shared edges' errors read
            owner = int(ranks[aop[0]])
            a = e.anchor(0)
            at = torch.from_numpy(H.to_dev_layout(a)) if a is not None else torch.empty((D + 1) * R, dtype=torch.float64)
            dist.broadcast(at, src=owner)
            anchor = H.from_dev_layout(at.numpy(), R)
            assert int(e.recv_counts.sum()) > 0
            refused = {}
            probe = np.full(g.m, np.nan)
            try:
                e.errors_into(probe, recv_ptr=None)
                refused["recv"] = False
            except H.DPGOHipError:
                refused["recv"] = np.isnan(probe).all()
            if rank != owner:  # without an anchor only the owner of pose 0 can define the frame
                try:
                    e.errors_into(probe, recv_ptr=recv.data_ptr(), rounded=True)
                    refused["anchor"] = False
                except H.DPGOHipError:
                    refused["anchor"] = np.isnan(probe).all()
            lifted = np.full(g.m, np.nan)
            e.errors_into(lifted, recv_ptr=recv.data_ptr())
            rounded = np.full(g.m, np.nan)
            e.errors_into(rounded, recv_ptr=recv.data_ptr(), rounded=True, anchor=anchor)
        q.put((rank, lifted, rounded, all(refused.values()), sorted(refused)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_errors_bitwise_one_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=240) for _ in range(2)], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=60)
    assert all(o[3] for o in outs)
    assert sorted(len(o[4]) for o in outs) == [1, 2]  # the anchor refusal was tried on exactly one rank
    from dpgo_amd import hip as H
    g = H.Graph.grid3d(K, seed=5)
    aop = g.grid_partition(A)
    ranks = (np.arange(A ** 3) * 2 // A ** 3)
    owner = H.weight_owner(g, aop, A ** 3)
    p1 = g.arrays()["p1"].astype(np.int64)
    resp = np.where(owner >= 0, owner, aop[p1])
    # one rank, same schedule
    e1 = H.Rbcd(g, aop, np.zeros(A ** 3, np.int32), 0, 1, _params(H))
    e1.set_X(g.chain_init(R, O.lifting_matrix(D, R)))
    for it in range(ITERS):
        c = it % e1.num_colors
        e1.pre_exchange(c)
        e1.update(c, None)
    for which, kw in ((1, {}), (2, dict(rounded=True))):
        es = [o[which] for o in outs]
        wr = [~np.isnan(x) for x in es]
        # every edge by exactly one rank: the rank of the agent responsible for it (odometry: of its agent)
        assert np.all(wr[0].astype(int) + wr[1].astype(int) == 1)
        assert np.array_equal(wr[1], ranks[resp] == 1)
        assert wr[0].any() and wr[1].any()
        merged = np.where(wr[0], es[0], es[1])
        one = np.full(g.m, np.nan)
        e1.errors_into(one, **kw)
        assert np.array_equal(merged, one), which
    shared = aop[p1] != aop[g.arrays()["p2"].astype(np.int64)]
    assert np.any(shared & (ranks[aop[p1]] != ranks[aop[g.arrays()["p2"].astype(np.int64)]]))  # edges across ranks
