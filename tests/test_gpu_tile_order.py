"""Tile order of the pose-tiled launches (tuning key TUNE_TILE_ORDER = 13): which tile a block takes, and in which
direction consecutive launches walk the tiles, is placement only.  Each tile's arithmetic does not depend on when it
runs and the finalize reduces the tile partials in a fixed order, so every value gives bitwise the same iterates,
counters, traces and agent status: 0 the separate maps (SpMM remapped per XCD, vector passes tile = block), 1 the
unified map forward, 2 serpentine, 3 the value that added non-temporal one-use streams to 2 (measured slower and taken
out of the kernels, DESIGN.md 3.6: it now runs as 2 and stays in the comparison)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE_ORDER, CLASSIC_TCG = 13, 5
VALUES = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _run(hip, g, aop, X0, accel):
    e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=5, acceleration=accel))
    e.set_trace(512)
    e.set_X(X0)
    for it in range(40):
        e.pre_exchange(it % e.num_colors)
        e.update(it % e.num_colors, None)
    X = np.zeros(X0.size)
    e.get_X_into(X)
    tr = [np.array([[rec[k] for k in hip.TRACE_FIELDS] for rec in e.get_trace(a)]) for a in range(8)]
    rc, rd = e.status()
    return X, e.stats().copy(), tr, rc.copy(), rd.copy()


def _partition2(g, k):
    """Two agents per axis over grid3d(k).  Graph.grid_partition takes only sides the agent count divides, so an odd
    side is cut here, after its first ceil(k / 2) planes (uneven agents), from the generator's pose order: plane by
    plane, rows and planes traversed boustrophedon."""
    i = np.arange(k ** 3)
    z, idx = i // (k * k), i % (k * k)
    idx = np.where(z & 1, k * k - 1 - idx, idx)
    y, x = idx // k, idx % k
    x = np.where(y & 1, k - 1 - x, x)
    s = (k + 1) // 2
    aop = (x // s + 2 * (y // s + 2 * (z // s))).astype(np.int32)
    if k % 2 == 0:
        assert np.array_equal(aop, g.grid_partition(2))
    return aop


def _check_all_orders(hip, k, accel=1, classic=0):
    g = hip.Graph.grid3d(k, seed=5)
    aop = _partition2(g, k)
    X0, _, _ = g.distributed_init(aop, 5, hip.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    default = hip.get_tuning(TILE_ORDER)
    out = []
    try:
        hip.set_tuning(CLASSIC_TCG, classic)
        for v in VALUES:
            hip.set_tuning(TILE_ORDER, v)
            out.append(_run(hip, g, aop, X0, accel))
    finally:
        hip.set_tuning(TILE_ORDER, default)
        hip.set_tuning(CLASSIC_TCG, 0)
    X, stats, tr, rc, rd = out[0]
    assert sum(len(t) for t in tr) > 0  # the trace is on and recorded something
    for v, o in zip(VALUES[1:], out[1:]):
        assert np.array_equal(X, o[0]), v
        assert np.array_equal(stats, o[1]), v
        for a in range(8):
            assert np.array_equal(tr[a], o[2][a]), (v, a)
        assert np.array_equal(rc, o[3]), v
        assert np.array_equal(rd, o[4]), v


# k = 7: colour launches of fewer than 8 tiles; 10: 8 tiles; 11: uneven agents, partial tiles and a tile count that
# is no multiple of 8; 12: 16 tiles
@pytest.mark.parametrize("k", [7, 10, 11, 12])
def test_tile_order_bitwise(hip, k):
    _check_all_orders(hip, k)


def test_tile_order_bitwise_no_acceleration(hip):
    _check_all_orders(hip, 11, accel=0)


def test_tile_order_bitwise_classic_tcg(hip):
    _check_all_orders(hip, 11, classic=1)
