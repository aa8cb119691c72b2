"""GPU parity of the read-in kernel k_frame_lift (dpgo_hip_frame_lift / _dev), the inverse of k_round_se: per pose
X_j = YLift [F_R R_j | F_R t_j + F_t] with F the pose's frame, or X_j = YLift T_j without frames.

Every compiled (d, r); n = 1, 63, 64, 65, 130 (a partial block, one full block, a full block followed by a one-pose
block, two full blocks and a partial one).  Three frames at spans 1 / 64 / rest, so the first 64-pose block straddles
two frames and the second starts inside the second frame's span.  For d = 2 the input span width d (d+1) = 6 is even
and the output width 3 r is odd when r is odd, so the 16-byte and the 8-byte streaming paths both run on d = 2; the
_dev entry with pointers offset by 8 bytes reaches the 8-byte paths on every shape.

The bound is derived, not measured: entry by entry against an np.longdouble product,
  |err| <= gamma_{2d+2} (|YLift| (|F_R| |T| + |F_t|)),  gamma_k = k u / (1 - k u), u = 2^-53
(d products and d additions for the frame, d and d - 1 for the lift; fused multiply-adds only drop roundings), and
gamma_d |YLift| |T| without frames."""
import functools

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _frames as F

pytestmark = pytest.mark.gpu

PAIRS = [(2, r) for r in range(2, 9)] + [(3, r) for r in range(3, 9)]
SIZES = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


@functools.lru_cache(maxsize=None)
def _inputs(d, n):
    """Seeded SE(d) poses (translations of a few units), three frames, and the pose -> frame map."""
    rng = np.random.default_rng(1000 * d + n)
    b = d + 1
    T = np.zeros((d, n * b))
    for j in range(n):
        T[:, j * b:j * b + d] = F._random_rotation(rng, d)
        T[:, j * b + d] = rng.normal(0.0, 3.0, d)
    frames = np.zeros((3, d, b))
    for f in range(3):
        frames[f, :, :d] = F._random_rotation(rng, d)
        frames[f, :, d] = rng.normal(0.0, 10.0, d)
    frame_of = np.where(np.arange(n) < 1, 0, np.where(np.arange(n) < 65, 1, 2)).astype(np.int32)
    for a in (T, frames, frame_of):
        a.setflags(write=False)
    return T, frames, frame_of


@functools.lru_cache(maxsize=None)
def _reference(d, r, n, with_frames):
    T, frames, frame_of = _inputs(d, n)
    Y = O.lifting_matrix(d, r)
    X, Xa = F.host_lift(T, Y, frames if with_frames else None, frame_of if with_frames else None)
    bound = (F.gamma(2 * d + 2) if with_frames else F.gamma(d)) * Xa
    X.setflags(write=False)
    bound.setflags(write=False)
    return Y, X, bound


@pytest.mark.parametrize("d,r", PAIRS)
def test_frame_lift_within_rounding_bound(hip, d, r):
    for n in SIZES:
        T, frames, frame_of = _inputs(d, n)
        for with_frames in (True, False):
            Y, want, bound = _reference(d, r, n, with_frames)
            got = hip.frame_lift(T, Y, frames, frame_of) if with_frames else hip.frame_lift(T, Y)
            assert got.shape == (r, (d + 1) * n)
            err = np.abs(got.astype(np.longdouble) - want)
            worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
            assert np.all(err <= bound), (d, r, n, with_frames, worst)


def _dev(H, d, r, n, with_frames, off_in, off_out):
    """dpgo_hip_frame_lift_dev on torch device buffers; off_in / off_out: T and X_out start 8 bytes off a 16-byte
    boundary (the kernel's 8-byte streaming paths)."""
    import torch
    T, frames, frame_of = _inputs(d, n)
    Y = O.lifting_matrix(d, r)
    b = d + 1
    tt = torch.empty(off_in + T.size, dtype=torch.float64, device="cuda")
    tt[off_in:].copy_(torch.from_numpy(H.to_dev_layout(T)))
    ot = torch.full((off_out + n * r * b,), float("nan"), dtype=torch.float64, device="cuda")
    fp = fop = None
    if with_frames:
        ft = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 2, 1)).ravel()).cuda()
        fo = torch.from_numpy(np.array(frame_of)).cuda()
        fp, fop = ft.data_ptr(), fo.data_ptr()
    s = torch.cuda.current_stream()
    H.frame_lift_dev(r, d, n, tt.data_ptr() + 8 * off_in, Y, fp, 3, fop, ot.data_ptr() + 8 * off_out, s.cuda_stream)
    s.synchronize()
    return H.from_dev_layout(ot[off_out:].cpu().numpy(), r)


@pytest.mark.parametrize("d,r", PAIRS)
def test_misaligned_device_pointers_are_bitwise(hip, d, r):
    for n in (64, 130):
        T, frames, frame_of = _inputs(d, n)
        Y = O.lifting_matrix(d, r)
        for with_frames in (True, False):
            host = hip.frame_lift(T, Y, frames, frame_of) if with_frames else hip.frame_lift(T, Y)
            for off_in, off_out in [(0, 0), (1, 0), (0, 1), (1, 1)]:
                got = _dev(hip, d, r, n, with_frames, off_in, off_out)
                assert np.array_equal(got, host), (d, r, n, with_frames, off_in, off_out)


@pytest.mark.parametrize("d,r", PAIRS)
def test_round_trip_through_round_se(hip, d, r):
    """round_se in the frame of the anchor YLift [I | 0] undoes the plain lift, at the suite's 1e-12 bar for the
    per-pose kernels."""
    Y = O.lifting_matrix(d, r)
    anchor = Y @ np.hstack([np.eye(d), np.zeros((d, 1))])
    for n in (1, 65, 130):
        T, _, _ = _inputs(d, n)
        back = hip.round_se(hip.frame_lift(T, Y), d, anchor=anchor)
        assert np.abs(back - T).max() <= 1e-12, (d, r, n)


def test_bad_arguments_are_refused(hip):
    d, r, n = 3, 5, 4
    T, frames, frame_of = _inputs(d, n)
    Y = O.lifting_matrix(d, r)
    E = hip.DPGOHipError
    with pytest.raises(E, match="unsupported"):
        hip.frame_lift(T, np.zeros((9, d)))  # rank 9 is not compiled
    with pytest.raises(E, match="unsupported"):
        hip.frame_lift(np.zeros((2, 3 * n)), np.zeros((1, 2)))  # r < d
    with pytest.raises(E, match="n >= 1"):
        hip.frame_lift(np.zeros((d, 0)), Y)
    with pytest.raises(E, match="both or neither"):
        hip.frame_lift(T, Y, frames, None)
    with pytest.raises(E, match="both or neither"):
        hip.frame_lift(T, Y, None, frame_of)
    for bad in (-1, 3):
        fo = np.array(frame_of)
        fo[2] = bad
        with pytest.raises(E, match="out of range"):
            hip.frame_lift(T, Y, frames, fo)
    import ctypes as C
    L = hip.lib()
    dp = C.POINTER(C.c_double)
    ok = np.zeros(r * (d + 1) * n)
    y = np.ascontiguousarray(Y.T).ravel()
    t = hip.to_dev_layout(T)
    for tp, yp, op in [(None, y.ctypes.data_as(dp), ok.ctypes.data_as(dp)),
                       (t.ctypes.data_as(dp), None, ok.ctypes.data_as(dp)),
                       (t.ctypes.data_as(dp), y.ctypes.data_as(dp), None)]:
        assert L.dpgo_hip_frame_lift(r, d, n, tp, yp, None, 0, None, op) == -1
    # the device entry refuses the same before any pointer is read (8: a non-null placeholder)
    for args in [(9, d, n, 8, np.zeros((9, d)), None, 0, None, 8),  # unsupported (r, d)
                 (r, d, 0, 8, Y, None, 0, None, 8),  # n <= 0
                 (r, d, n, None, Y, None, 0, None, 8),  # null T
                 (r, d, n, 8, Y, None, 0, None, None),  # null X_out
                 (r, d, n, 8, Y, 8, 3, None, 8),  # frames without frame_of
                 (r, d, n, 8, Y, None, 3, 8, 8)]:  # frame_of without frames
        with pytest.raises(E):
            hip.frame_lift_dev(*args)
    assert L.dpgo_hip_frame_lift_dev(r, d, n, C.c_void_p(8), None, None, 0, None, C.c_void_p(8), None) == -1  # null YLift
