"""dpgo_rbcd_weight_owner (host only, no GPU): which agent's weight dpgo_rbcd_get_weights reports per edge -- -1 for
odometry, the agent itself for a private loop closure, the lower-ID agent for a shared one (the only copy
PGOAgent::updateLoopClosuresWeights ever updates, src/PGOAgent.cpp:1201-1235)."""
import ctypes as C

import numpy as np
import pytest

from tests._common import load_meas


@pytest.fixture(scope="module")
def H():
    from dpgo_amd import hip
    return hip


def _owner_numpy(p1, p2, aop, num_agents):
    """The rule restated: local index = rank of the pose among its agent's poses in global order."""
    aop = np.asarray(aop, np.int64)
    local = np.zeros(len(aop), np.int64)
    for a in range(num_agents):
        idx = np.nonzero(aop == a)[0]
        local[idx] = np.arange(len(idx))
    a1, a2 = aop[p1], aop[p2]
    same = a1 == a2
    odo = same & (local[p2] == local[p1] + 1)
    return np.where(odo, -1, np.where(same, a1, np.minimum(a1, a2))).astype(np.int32)


def _check_rule(owner, p1, p2, aop):
    a1, a2 = np.asarray(aop)[p1], np.asarray(aop)[p2]
    shared = a1 != a2
    assert shared.any() and (~shared).any()
    assert np.array_equal(owner[shared], np.minimum(a1, a2)[shared])  # shared: the lower ID
    assert np.all((owner[~shared] == -1) | (owner[~shared] == a1[~shared]))  # private: the agent, or -1 (chain)
    return shared


def test_weight_owner_grid_cubes(H):
    g = H.Graph.grid3d(4, seed=3)
    aop = g.grid_partition(2)
    a = g.arrays()
    p1, p2 = a["p1"].astype(np.int64), a["p2"].astype(np.int64)
    owner = H.weight_owner(g, aop, 8)
    assert owner.shape == (g.m,)
    assert np.array_equal(owner, _owner_numpy(p1, p2, aop, 8))
    shared = _check_rule(owner, p1, p2, aop)
    # a cube's poses are not contiguous in the global order: chain edges are those between consecutive *local* indices
    assert (owner == -1).sum() > 0
    assert ((owner >= 0) & ~shared).sum() > 0


def test_weight_owner_contiguous_robots(H):
    meas = load_meas("smallGrid3D")
    n = meas.num_poses
    g = H.Graph.from_arrays(meas.d, n, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    aop = np.minimum(np.arange(n) // (n // 5), 4).astype(np.int32)
    owner = H.weight_owner(g, aop, 5)
    p1, p2 = np.asarray(meas.p1, np.int64), np.asarray(meas.p2, np.int64)
    assert np.array_equal(owner, _owner_numpy(p1, p2, aop, 5))
    shared = _check_rule(owner, p1, p2, aop)
    # contiguous ranges: the chain edges inside a robot are exactly p2 = p1 + 1
    assert np.array_equal(owner == -1, ~shared & (p2 == p1 + 1))


def test_weight_owner_bad_arguments(H):
    g = H.Graph.grid3d(3, seed=0)
    aop = np.zeros(g.n, np.int32)
    out = np.empty(g.m, np.int32)
    L = H.lib()
    ip = C.POINTER(C.c_int)
    ap, op = aop.ctypes.data_as(ip), out.ctypes.data_as(ip)
    assert L.dpgo_rbcd_weight_owner(None, 1, ap, op) == -1  # DPGO_HIP_EINVAL
    assert L.dpgo_rbcd_weight_owner(g.h, 1, None, op) == -1  # DPGO_HIP_EINVAL
    assert L.dpgo_rbcd_weight_owner(g.h, 1, ap, None) == -1  # DPGO_HIP_EINVAL
    assert L.dpgo_rbcd_weight_owner(g.h, 0, ap, op) == -1  # DPGO_HIP_EINVAL
    assert L.dpgo_hip_last_error().decode()
    bad = aop.copy()
    bad[5] = 3
    with pytest.raises(H.DPGOHipError, match="out of range"):
        H.weight_owner(g, bad, 2)
    bad[5] = -1
    with pytest.raises(H.DPGOHipError, match="out of range"):
        H.weight_owner(g, bad, 2)
    with pytest.raises(ValueError):
        H.weight_owner(g, aop[:-1], 1)
    assert np.array_equal(H.weight_owner(g, aop, 1) == -1, np.asarray(g.arrays()["p2"]) == np.asarray(g.arrays()["p1"]) + 1)
