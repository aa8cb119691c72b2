"""The engine's trajectory read-in (dpgo_rbcd_set_trajectory): the owned poses' d x (d+1) blocks and one frame per
agent go to the device, k_frame_lift writes X, and the Nesterov / iteration state is reset exactly as by set_X.  On
the corrupted fixtures of tests/_frames.py (robust multi-robot initialisation: odometry local trajectories + GNC-TLS
frames), with GNC_TLS reweighting every 3 iterations as tests/test_gpu_readout_multirank.py."""
import os

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _frames as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 6


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _params(H, r):
    return H.rbcd_params(r=r, acceleration=1, robust_cost=H.ROBUST["GNC_TLS"], robust_opt_inner_iters=3)


def _engine(H, fx, r, g=None):
    g = g or F.graph_of(H, fx)
    return H.Rbcd(g, fx["aop"], np.zeros(fx["K"], np.int32), 0, 1, _params(H, r)), g


def _X(e):
    out = np.full(e.graph.n * (e.graph.d + 1) * e.params.r, np.nan)
    e.get_X_into(out)
    return out


def _run(e, iters):
    for it in range(iters):
        c = it % e.num_colors
        e.pre_exchange(c)
        e.update(c, None)


def _state(e):
    w = np.full(e.graph.m, np.nan)
    e.weights_into(w)
    rc, rd = e.status()
    return _X(e), e.stats(), rc, rd, w


def _same_state(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("fixture,r", [(F.fixture3d, 5), (F.fixture2d, 3)])
def test_set_trajectory_is_the_frame_lift(hip, fixture, r):
    fx = fixture()
    d = fx["d"]
    Y = O.lifting_matrix(d, r)
    frames = fx["robust"]["frames"]
    e, _ = _engine(hip, fx, r)
    e.set_trajectory(fx["T_local"], Y, frames)
    got = hip.from_dev_layout(_X(e), r)
    assert np.array_equal(got, hip.frame_lift(fx["T_local"], Y, frames, fx["aop"]))
    want, mag = F.host_lift(fx["T_local"], Y, frames, fx["aop"])
    assert np.all(np.abs(got.astype(np.longdouble) - want) <= F.gamma(2 * d + 2) * mag)


def test_start_equals_set_X_start(hip):
    """Engine A started by set_trajectory, engine B by set_X(A's X): bitwise the same X, solver counters, status and
    weights after 6 colour-schedule iterations (two reweightings), so the reset is set_X's."""
    fx = F.fixture3d()
    Y = O.lifting_matrix(3, 5)
    A, g = _engine(hip, fx, 5)
    A.set_trajectory(fx["T_local"], Y, fx["robust"]["frames"])
    B, _ = _engine(hip, fx, 5, g)
    B.set_X(_X(A))
    _run(A, ITERS)
    _run(B, ITERS)
    sa, sb = _state(A), _state(B)
    assert _same_state(sa, sb)
    assert np.any((sa[4] > 0.0) & (sa[4] < 1.0))  # the reweighting happened


def test_restart_of_a_running_engine(hip):
    """set_trajectory on a running engine.  After 4 iterations (one reweighting behind it) X is bitwise a fresh
    engine's after the same call, and everything that follows is bitwise what set_X of that X gives on an engine with
    the same 4 iterations behind it: like set_X -- and PGOAgent::setX -- the call resets the iterate and the Nesterov
    / iteration state, not the robust cost's weights and mu.  After 1 iteration (the first reweighting comes with the
    second) the restarted engine is therefore a fresh one altogether: X, status and weights stay bitwise equal over 6
    more iterations."""
    fx = F.fixture3d()
    Y = O.lifting_matrix(3, 5)
    frames = fx["robust"]["frames"]
    fresh, g = _engine(hip, fx, 5)
    fresh.set_trajectory(fx["T_local"], Y, frames)
    X0 = _X(fresh)
    A, _ = _engine(hip, fx, 5, g)
    A.set_trajectory(fx["T_local"], Y, frames)
    _run(A, 4)
    A.set_trajectory(fx["T_local"], Y, frames)
    C, _ = _engine(hip, fx, 5, g)
    C.set_X(X0)
    _run(C, 4)
    C.set_X(X0)
    assert np.array_equal(_X(A), X0) and np.array_equal(_X(C), X0)
    _run(A, ITERS)
    _run(C, ITERS)
    assert _same_state(_state(A), _state(C))
    B, _ = _engine(hip, fx, 5, g)
    B.set_trajectory(fx["T_local"], Y, frames)
    _run(B, 1)
    B.set_trajectory(fx["T_local"], Y, frames)
    _run(B, ITERS)
    _run(fresh, ITERS)
    sb, sf = _state(B), _state(fresh)
    assert all(np.array_equal(sb[k], sf[k], equal_nan=True) for k in (0, 2, 3, 4))  # stats are cumulative


def test_warm_start_from_a_readout(hip):
    """frames = None with a trajectory from trajectory_into: the lifted rotation blocks are orthonormal to 1e-14."""
    fx = F.fixture3d()
    d, r = 3, 5
    Y = O.lifting_matrix(d, r)
    A, g = _engine(hip, fx, r)
    A.set_trajectory(fx["T_local"], Y, fx["robust"]["frames"])
    _run(A, 3)
    T = np.full(g.n * (d + 1) * d, np.nan)
    A.trajectory_into(T)
    B, _ = _engine(hip, fx, r, g)
    B.set_trajectory(T, Y)
    X = hip.from_dev_layout(_X(B), r)
    assert np.array_equal(X, hip.frame_lift(hip.from_dev_layout(T, d), Y))
    Yb = O.to_poses(X, r, d)[:, :, :d]
    assert np.abs(np.swapaxes(Yb, 1, 2) @ Yb - np.eye(d)).max() <= 1e-14


def test_null_arguments_are_refused(hip):
    fx = F.fixture3d()
    e, _ = _engine(hip, fx, 5)
    L = hip.lib()
    import ctypes as C
    dp = C.POINTER(C.c_double)
    t = hip.to_dev_layout(fx["T_local"])
    y = np.ascontiguousarray(O.lifting_matrix(3, 5).T).ravel()
    assert L.dpgo_rbcd_set_trajectory(e.h, None, y.ctypes.data_as(dp), None) == -1
    assert L.dpgo_rbcd_set_trajectory(e.h, t.ctypes.data_as(dp), None, None) == -1
    assert L.dpgo_rbcd_set_trajectory(None, t.ctypes.data_as(dp), y.ctypes.data_as(dp), None) == -1


def _worker(rank, world, q):
    import sys
    sys.path.insert(0, ROOT)
    from dpgo_amd import hip as H
    fx = F.fixture3d()
    g = F.graph_of(H, fx)
    ranks = (np.arange(fx["K"]) * world // fx["K"]).astype(np.int32)
    e = H.Rbcd(g, fx["aop"], ranks, rank, world, _params(H, 5))
    e.set_trajectory(fx["T_local"], O.lifting_matrix(3, 5), fx["robust"]["frames"])
    q.put((rank, _X(e)))


def test_two_ranks_write_their_own_poses(hip):
    """Two processes on the one device, each an engine rank that owns half of the agents: every pose is written by
    exactly one rank, and the merged X is bitwise the one-rank engine's."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=240) for _ in range(2)], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=60)
    fx = F.fixture3d()
    rb = 5 * 4
    Xs = [o[1].reshape(fx["n"], rb) for o in outs]
    written = [~np.isnan(X) for X in Xs]
    assert all(np.array_equal(w.all(axis=1), w.any(axis=1)) for w in written)
    assert np.all(written[0].all(axis=1).astype(int) + written[1].all(axis=1).astype(int) == 1)
    ranks = np.arange(fx["K"]) * 2 // fx["K"]
    assert np.array_equal(written[1].all(axis=1), ranks[fx["aop"]] == 1)
    e1, _ = _engine(hip, fx, 5)
    e1.set_trajectory(fx["T_local"], O.lifting_matrix(3, 5), fx["robust"]["frames"])
    assert np.array_equal(np.where(written[0], Xs[0], Xs[1]).ravel(), _X(e1))
