"""GPU parity of the rank staircase's streaming kernel k_lift_escape (dpgo_hip_lift_escape / _dev): the lift of
rank-r poses to rank r + 1 with a QF retraction along alpha [0; v^T].  Build-defined (the reference has no
staircase): pinned against the oracle's retract_qf on the zero-row lift, at the project's 1e-13 bar for manifold
operations (tests/test_gpu_parity.py), and bitwise where no arithmetic is involved.

Shapes: every (d, r) whose rank r + 1 is compiled; n = 1, 63, 64, 65, 200 (a partial block, one full block, a full
block followed by a one-pose block, several blocks).  For d = 2 exactly one of r (d+1) and (r+1)(d+1) is odd, so the
16-byte and the 8-byte streaming paths both run on every d = 2 shape with n >= 64."""
import functools

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests._common import random_point, rel

pytestmark = pytest.mark.gpu

PAIRS = [(2, r) for r in range(2, 8)] + [(3, r) for r in range(3, 8)]
SIZES = [1, 63, 64, 65, 200]
ALPHAS = [0.3, 4.0]


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


@functools.lru_cache(maxsize=None)
def _inputs(d, r, n):
    """X = random_point, v Gaussian with a few poses zeroed (a pose the direction does not move)."""
    b = d + 1
    X = random_point(r, d, n, 100 * d + 10 * r + n)
    v = np.random.default_rng(7 * n + r).standard_normal(b * n)
    for j in range(0, n, 5):
        v[j * b:(j + 1) * b] = 0.0
    X.setflags(write=False)
    v.setflags(write=False)
    return X, v


def _reference(X, v, alpha, d):
    Xl = np.vstack([X, np.zeros((1, X.shape[1]))])
    D = np.zeros_like(Xl)
    D[-1] = alpha * v
    return Xl, O.retract_qf(Xl, D, d)


@pytest.mark.parametrize("d,r", PAIRS)
def test_lift_escape_matches_oracle(hip, d, r):
    for n in SIZES:
        X, v = _inputs(d, r, n)
        for alpha in ALPHAS:
            Xl, want = _reference(X, v, alpha, d)
            got = hip.lift_escape(X, d, v, alpha)
            assert got.shape == (r + 1, (d + 1) * n)
            err = rel(got, want)
            assert err <= 1e-13, (d, r, n, alpha, err)
            # translations: (p; alpha v_p) exactly
            assert np.array_equal(got[:r, d::d + 1], X[:, d::d + 1])
            assert np.array_equal(got[r, d::d + 1], alpha * v[d::d + 1])
            Y = O.to_poses(got, r + 1, d)[:, :, :d]
            assert np.abs(np.swapaxes(Y, 1, 2) @ Y - np.eye(d)).max() <= 1e-14


@pytest.mark.parametrize("d,r", PAIRS)
def test_plain_lift_is_bitwise(hip, d, r):
    for n in SIZES:
        X, _ = _inputs(d, r, n)
        got = hip.lift_escape(X, d, None)
        assert np.array_equal(got, np.vstack([X, np.zeros((1, X.shape[1]))])), (d, r, n)


def _dev(H, X, v, alpha, d, misalign):
    """dpgo_hip_lift_escape_dev on torch device buffers (misalign: X, v and X_out start 8 bytes off a 16-byte
    boundary: the kernel's scalar paths)."""
    import torch
    r, b = X.shape[0], d + 1
    n = X.shape[1] // b
    off = 1 if misalign else 0
    xt = torch.empty(off + X.size, dtype=torch.float64, device="cuda")
    xt[off:].copy_(torch.from_numpy(H.to_dev_layout(X)))
    vt = None
    if v is not None:
        vt = torch.empty(off + v.size, dtype=torch.float64, device="cuda")
        vt[off:].copy_(torch.from_numpy(np.array(v)))
    ot = torch.full((off + n * (r + 1) * b,), float("nan"), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    H.lift_escape_dev(r, d, n, xt.data_ptr() + 8 * off, vt.data_ptr() + 8 * off if vt is not None else None, alpha,
                      ot.data_ptr() + 8 * off, s.cuda_stream)
    s.synchronize()
    return H.from_dev_layout(ot[off:].cpu().numpy(), r + 1)


@pytest.mark.parametrize("d,r", PAIRS)
def test_misaligned_device_pointers_are_bitwise(hip, d, r):
    """The _dev entry with every pointer offset by one double (the 8-byte streaming paths) gives bitwise the aligned
    result, which is bitwise the host entry's."""
    for n in (64, 200):
        X, v = _inputs(d, r, n)
        host = hip.lift_escape(X, d, v, 0.3)
        assert np.array_equal(_dev(hip, X, v, 0.3, d, False), host)
        assert np.array_equal(_dev(hip, X, v, 0.3, d, True), host)
        assert np.array_equal(_dev(hip, X, None, 0.0, d, True), np.vstack([X, np.zeros((1, X.shape[1]))]))


@pytest.mark.parametrize("d", [2, 3])
def test_rank_8_is_refused(hip, d):
    X = np.zeros((8, (d + 1) * 3))
    with pytest.raises(hip.DPGOHipError, match="not compiled"):
        hip.lift_escape(X, d, None)
    with pytest.raises(hip.DPGOHipError, match="not compiled"):
        hip.lift_escape_dev(8, d, 3, 8, None, 1.0, 8)  # refused before any pointer is read
    with pytest.raises(hip.DPGOHipError):
        hip.lift_escape(np.zeros((1, (d + 1) * 3)), d, None)  # r < d
