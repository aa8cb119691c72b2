"""GPU tests of the rank reduction on the engine and on the whole graph: Rbcd.gram / Rbcd.get_X_reduced_into on one
rank and on two, a rank-k engine started from the reduced X, and Graph.rank_reduce (Gram -> spectrum -> numerical
rank -> reduce) on an exactly low-rank point of the ragged graph.  Reference: tests/_rank.py."""
import os
import socket

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _ragged as RA
from tests import _rank as RK
from tests._common import load_meas, random_point

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_L = np.longdouble
R, D, STEPS = 5, 3, 20


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _assert_gram(got, X, d, m):
    Cl, A = RK.gram(X, d)
    err = np.abs(got.astype(_L) - Cl)
    assert np.all(err <= RK.gamma(m) * A), float((err / (RK.U_ROUND * A)).max())


@pytest.fixture(scope="module")
def engine(hip):
    """smallGrid3D, 5 agents, r = 5, after 20 colour steps: the engine, its X and numpy's spectrum of X's Gram."""
    meas = load_meas("smallGrid3D")
    d, n = meas.d, meas.num_poses
    assert d == D
    g = hip.Graph.from_arrays(d, n, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    aop = np.minimum(np.arange(n) // (n // 5), 4).astype(np.int32)
    e = hip.Rbcd(g, aop, np.zeros(5, np.int32), 0, 1, hip.rbcd_params(r=R, acceleration=1))
    e.set_X(O.lifting_matrix(d, R) @ O.chordal_initialization(d, n, meas))
    for it in range(STEPS):
        e.pre_exchange(it % e.num_colors)
        e.update(it % e.num_colors, None)
    Xf = np.zeros(R * (d + 1) * n)
    e.get_X_into(Xf)
    X = hip.from_dev_layout(Xf, R)
    X.setflags(write=False)
    w, U = RK.spectrum(RK.gram(X, d)[0])
    return dict(meas=meas, g=g, aop=aop, e=e, X=X, U=U, n=n, Q=O.connection_laplacian(meas, n))


def test_engine_gram_matches_longdouble(hip, engine):
    """The owned buffer is the engine's pose order, not the global one, so the value is not bitwise hip.gram(get_X);
    the rounding depth of k_gram's order (tests/_rank.py gram_depth) bounds it all the same."""
    got = engine["e"].gram()
    assert np.array_equal(got, got.T)
    _assert_gram(got, engine["X"], D, RK.gram_depth(D, engine["n"]))
    assert np.array_equal(engine["e"].gram(), got)


@pytest.mark.parametrize("k", [3, 4])
def test_engine_reduced_readout_is_bitwise_and_starts_a_rank_k_engine(hip, engine, k):
    e, g, X, n = engine["e"], engine["g"], engine["X"], engine["n"]
    W = engine["U"][:, :k]
    Xk = np.full(k * (D + 1) * n, np.nan)
    e.get_X_reduced_into(W, Xk)
    want = hip.rank_reduce(X, D, W)
    assert np.array_equal(hip.from_dev_layout(Xk, k), want)
    ek = hip.Rbcd(g, engine["aop"], np.zeros(5, np.int32), 0, 1, hip.rbcd_params(r=k, acceleration=1))
    ek.set_X(Xk)
    f, _ = ek.central_eval()
    fn = 0.5 * float(np.sum(np.asarray((engine["Q"] @ want.T).T) * want))
    assert abs(f - fn) <= 1e-12 * abs(fn), (f, fn)
    back = np.zeros_like(Xk)
    ek.get_X_into(back)
    assert np.array_equal(back, Xk)
    with pytest.raises(hip.DPGOHipError, match="d <= k < r"):
        e.get_X_reduced_into(np.eye(R), np.zeros(R * (D + 1) * n))
    with pytest.raises(ValueError, match="rank"):
        e.get_X_reduced_into(W, np.zeros(8))


# ---------------------------------------------------------------------------------------- two ranks, one device
KG, AG, ITERS = 6, 2, 6
W2 = np.linalg.qr(np.random.default_rng(0).standard_normal((R, 3)))[0]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dpgo_amd import hip as H
        g = H.Graph.grid3d(KG, seed=5)
        aop = g.grid_partition(AG)
        ranks = (np.arange(AG ** 3) * world // AG ** 3).astype(np.int32)
        e = H.Rbcd(g, aop, ranks, rank, world, H.rbcd_params(r=R, acceleration=1))
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
            Xk = np.full(g.n * (D + 1) * 3, np.nan)
            e.get_X_reduced_into(W2, Xk)
            C = e.gram()
        q.put((rank, Xk, C))
    finally:
        dist.destroy_process_group()


def test_two_ranks_reduced_readout_bitwise_one_rank(hip):
    """Each rank writes its owned poses of the reduced X and its partial Gram; the merged X is bitwise the one-rank
    engine's (the kernel works per pose), the summed Gram is within the rounding bound of the one-rank X's (each
    partial's depth for at most n poses, and one host addition) but covers other spans, so it is not compared
    bitwise."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=240) for _ in range(2)], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=60)
    g = hip.Graph.grid3d(KG, seed=5)
    aop = g.grid_partition(AG)
    Xs = [o[1].reshape(g.n, (D + 1) * 3) for o in outs]
    written = [~np.isnan(x) for x in Xs]
    assert all(np.array_equal(wr.all(axis=1), wr.any(axis=1)) for wr in written)
    assert np.all(written[0].all(axis=1).astype(int) + written[1].all(axis=1).astype(int) == 1)
    ranks = np.arange(AG ** 3) * 2 // AG ** 3
    assert np.array_equal(written[1].all(axis=1), ranks[aop] == 1)
    merged = np.where(written[0], Xs[0], Xs[1]).ravel()
    e1 = hip.Rbcd(g, aop, np.zeros(AG ** 3, np.int32), 0, 1, hip.rbcd_params(r=R, acceleration=1))
    e1.set_X(g.chain_init(R, O.lifting_matrix(D, R)))
    for it in range(ITERS):
        e1.pre_exchange(it % e1.num_colors)
        e1.update(it % e1.num_colors, None)
    X1k = np.full(g.n * (D + 1) * 3, np.nan)
    e1.get_X_reduced_into(W2, X1k)
    assert np.array_equal(merged, X1k)
    X1 = np.zeros(g.n * (D + 1) * R)
    e1.get_X_into(X1)
    _assert_gram(outs[0][2] + outs[1][2], hip.from_dev_layout(X1, R), D, RK.gram_depth(D, g.n) + 1)


# ---------------------------------------------------------------------------------------- whole graph
@pytest.fixture(scope="module", params=[2, 3])
def ragged(request, hip):
    d = request.param
    meas, _ = RA.ragged_graph(d)
    g = hip.Graph.from_arrays(d, meas.num_poses, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    return dict(d=d, meas=meas, g=g, n=meas.num_poses)


@pytest.mark.parametrize("r,k", [(5, 3), (5, 4), (8, 3)])
def test_graph_rank_reduce_recovers_the_rank(hip, ragged, r, k):
    """X = G T, T seeded on the rank-k manifold over the ragged graph's 645 poses: k is recovered at tol 1e-6, f is
    kept to 1e-12 relative, and the dropped eigenvalues are at rounding level (<= 1e-13 d n)."""
    d, g, n, meas = ragged["d"], ragged["g"], ragged["n"], ragged["meas"]
    G = np.linalg.qr(np.random.default_rng(10 * r + k).standard_normal((r, k)))[0]
    X = G @ random_point(k, d, n, 7 + 10 * k + r)
    kk, Xk, info = g.rank_reduce(X, r, 1e-6)
    assert kk == k and Xk.shape == (k * (d + 1) * n,)
    assert info["w"].shape == (r,) and np.all(np.diff(info["w"]) <= 0)
    assert abs(info["w"].sum() - d * n) <= 1e-12 * d * n
    fb = float(RA.edge_reference(meas, X)["f"])
    assert abs(info["f_before"] - fb) <= 1e-12 * abs(fb)
    assert abs(info["f_after"] - info["f_before"]) <= 1e-12 * abs(info["f_before"]), info
    assert 0.0 <= abs(info["dropped"]) <= 1e-13 * d * n
    assert info["dropped"] == info["w"][k:][::-1].cumsum()[-1]
    Xm = hip.from_dev_layout(Xk, k)
    assert np.array_equal(Xm, hip.rank_reduce(X, d, hip.gram_eig(hip.gram(X, d))[1][:, :k]))
    assert np.abs(Xm.T @ Xm - X.T @ X).max() <= 1e-13 * max(1.0, np.abs(X.T @ X).max())


def test_graph_rank_reduce_full_rank_copies(hip, ragged):
    d, g, n = ragged["d"], ragged["g"], ragged["n"]
    X = random_point(5, d, n, 99)
    kk, Xk, info = g.rank_reduce(X, 5, 1e-6)
    assert kk == 5 and np.array_equal(Xk, hip.to_dev_layout(X))
    assert info["dropped"] == 0.0 and info["f_after"] == info["f_before"]
    with pytest.raises(hip.DPGOHipError, match="tol"):
        g.rank_reduce(X, 5, 1.0)
    with pytest.raises(hip.DPGOHipError, match="tol"):
        g.rank_reduce(X, 5, -1e-3)
