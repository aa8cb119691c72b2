"""Solution readout across ranks: two processes (both on the one visible GPU, gloo for the halo and the anchor)
each fill their share of NaN-initialised global trajectory / weight arrays.  Every pose and every edge is written by
exactly one rank, and the merged arrays are bitwise those of a one-rank engine on the same schedule (the rounding
kernel works per pose, and the weights are the engine's, which do not depend on the rank count)."""
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
K, A, R, D, ITERS = 6, 2, 5, 3, 6


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _params(H):
    return H.rbcd_params(r=R, acceleration=1, robust_cost=H.ROBUST["GNC_TLS"], robust_opt_inner_iters=3)


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
        X0 = g.chain_init(R, O.lifting_matrix(D, R))
        e.set_X(X0)
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
            # the global anchor: pose 0's lifted pose from the rank that owns it, broadcast to the others
            owner = int(ranks[aop[0]])
            a = e.anchor(0)
            assert (a is not None) == (rank == owner)
            at = torch.from_numpy(H.to_dev_layout(a)) if a is not None else torch.empty((D + 1) * R, dtype=torch.float64)
            dist.broadcast(at, src=owner)
            anchor = H.from_dev_layout(at.numpy(), R)
            T = np.full(g.n * (D + 1) * D, np.nan)
            no_anchor_refused = False
            if rank != owner:  # without an anchor only the owner of pose 0 can define the frame
                try:
                    e.trajectory_into(T)
                except H.DPGOHipError:
                    no_anchor_refused = True
                assert np.isnan(T).all()
            e.trajectory_into(T, anchor=anchor)
            w = np.full(g.m, np.nan)
            e.weights_into(w)
        q.put((rank, T, w, rank == owner or no_anchor_refused))
    finally:
        dist.destroy_process_group()


def test_two_ranks_readout_bitwise_one_rank():
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
    from dpgo_amd import hip as H
    g = H.Graph.grid3d(K, seed=5)
    aop = g.grid_partition(A)
    # every pose by exactly one rank, whole
    Ts = [o[1].reshape(g.n, (D + 1) * D) for o in outs]
    written = [~np.isnan(T) for T in Ts]
    assert all(np.array_equal(wr.all(axis=1), wr.any(axis=1)) for wr in written)
    assert np.all(written[0].all(axis=1).astype(int) + written[1].all(axis=1).astype(int) == 1)
    ranks = (np.arange(A ** 3) * 2 // A ** 3)
    assert np.array_equal(written[1].all(axis=1), ranks[aop] == 1)
    # every edge by exactly one rank: the rank of the agent responsible for it (odometry: of its agent)
    ws = [o[2] for o in outs]
    wwr = [~np.isnan(w) for w in ws]
    assert np.all(wwr[0].astype(int) + wwr[1].astype(int) == 1)
    owner = H.weight_owner(g, aop, A ** 3)
    p1 = g.arrays()["p1"].astype(np.int64)
    resp = np.where(owner >= 0, owner, aop[p1])
    assert np.array_equal(wwr[1], ranks[resp] == 1)
    assert (owner >= 0).sum() > 0 and wwr[0].any() and wwr[1].any()
    Tm = np.where(written[0], Ts[0], Ts[1]).ravel()
    wm = np.where(wwr[0], ws[0], ws[1])
    # one rank, same schedule
    X0 = g.chain_init(R, O.lifting_matrix(D, R))
    e1 = H.Rbcd(g, aop, np.zeros(A ** 3, np.int32), 0, 1, _params(H))
    e1.set_X(X0)
    for it in range(ITERS):
        c = it % e1.num_colors
        e1.pre_exchange(c)
        e1.update(c, None)
    T1 = np.full(g.n * (D + 1) * D, np.nan)
    e1.trajectory_into(T1)
    w1 = np.full(g.m, np.nan)
    e1.weights_into(w1)
    assert np.array_equal(Tm, T1)
    assert np.array_equal(wm, w1)
    assert np.all(w1[owner < 0] == 1.0)
    assert np.any((w1 > 0.0) & (w1 < 1.0))  # the reweighting happened
