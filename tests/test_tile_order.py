"""The block -> tile map of the pose-tiled launches (tile_of_block, kernels.h; tuning key TUNE_TILE_ORDER), checked on
the host through dpgo_hip_tile_map / dpgo_hip_tile_of_block: for every launch size it is a permutation, a block keeps
its XCD's tile range in both directions, and the reverse direction walks every range from its end.  No GPU."""
import numpy as np
import pytest

MAX_NWG = 4100


@pytest.fixture(scope="module")
def H():
    from dpgo_amd import hip
    return hip


def _ranges(n):
    """First tile and tile count of the 8 XCD slots' ranges for a launch of n blocks."""
    q, r = divmod(n, 8)
    cnt = np.array([q + 1 if x < r else q for x in range(8)])
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return first, cnt


def test_permutation(H):
    for n in range(1, MAX_NWG + 1):
        want = np.arange(n)
        for reverse in (0, 1):
            assert np.array_equal(np.sort(H.tile_map(n, reverse)), want), (n, reverse)


def test_block_keeps_its_xcd_range(H):
    for n in range(1, MAX_NWG + 1):
        first, cnt = _ranges(n)
        xcd = np.arange(n) & 7
        for reverse in (0, 1):
            t = H.tile_map(n, reverse)
            assert np.all(t >= first[xcd]) and np.all(t < first[xcd] + cnt[xcd]), (n, reverse)


def test_forward_ascends_reverse_descends(H):
    for n in range(1, MAX_NWG + 1):
        first, cnt = _ranges(n)
        b = np.arange(n)
        xcd, rank = b & 7, b >> 3
        assert np.array_equal(H.tile_map(n, 0), first[xcd] + rank), n  # the map the SpMM has always used
        rev = H.tile_map(n, 1)
        assert np.array_equal(rev, first[xcd] + cnt[xcd] - 1 - rank), n
        for x in range(min(n, 8)):  # blocks x, x + 8, ... : strictly descending tiles
            assert np.all(np.diff(rev[x::8]) == -1), (n, x)


def test_single_block_entry(H):
    for n in (1, 5, 8, 13, 4100):
        for reverse in (0, 1):
            t = H.tile_map(n, reverse)
            assert [H.tile_of_block(b, n, reverse) for b in range(n)] == t.tolist()
    assert H.tile_of_block(0, 0, 0) == -1
    assert H.tile_of_block(-1, 8, 0) == -1
    assert H.tile_of_block(8, 8, 1) == -1
    assert H.tile_of_block(3, 5, 1) == 3  # fewer blocks than XCDs: every range is one tile
