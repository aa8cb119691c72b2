"""One measurement of the read-in kernel (k_frame_lift) and of the engine's trajectory read-in at the headline shape:
grid3d k = 100 (10^6 poses), r = 5, 64 cube agents, started from the robust multi-robot initialisation (odometry local
trajectories + GNC-TLS two-stage frames, on the host).

  kernel      HIP events around each dpgo_hip_frame_lift_dev launch on device buffers of this script, --reps launches
              after --warmup, the median with min .. max; algorithmic bytes 8 n (d b + r b) + 4 n of frame indices
              (the 64-entry frame table stays on-die).  Timed with the frames and without (W = T).
  yardstick   the plain lift of k_lift_escape (v = NULL, rank r -> r + 1: the same streaming shape, 8 n (r b + (r+1) b)
              bytes) on the lifted X, in the same process with the same launch counts
  end to end  host clock around Rbcd.set_trajectory (gather of the owned d x b blocks, upload, kernel, the Nesterov
              copies; it synchronises) against Rbcd.set_X of the same X (host-lifted r x b blocks), alternating, the
              median of --e2e-reps calls each with min .. max

Needs a gfx950 device; prints one JSON line last."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpgo_amd import hip as H  # noqa: E402


def _timed(launch, stream, warmup, reps):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--agents-per-axis", type=int, default=4)
    ap.add_argument("--r", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-reps", type=int, default=5)
    args = ap.parse_args()
    assert H.device_count() >= 1, "no gfx950 device visible"
    d, r = 3, args.r
    b = d + 1
    g = H.Graph.grid3d(args.k, seed=0, rot_sigma=0.01, trans_sigma=0.01)
    A = args.agents_per_axis
    K = A ** 3
    aop = g.grid_partition(A)
    n = g.n
    t0 = time.time()
    T_local, frames, info = g.distributed_init_ex(aop, local="odometry", align="robust")
    print(f"robust initialisation on the host: {time.time() - t0:.2f} s ({int(info['candidates'].sum())} candidates, "
          f"{int(info['inliers'].sum())} inliers over {K - 1} frames)", flush=True)
    Y = H.lifting_matrix(d, r)
    eng = H.Rbcd(g, aop, np.zeros(K, np.int32), 0, 1, H.rbcd_params(r=r, acceleration=1))

    Tflat = H.to_dev_layout(T_local)
    Td = torch.from_numpy(Tflat).cuda()
    Fd = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 2, 1)).ravel()).cuda()
    fo = torch.from_numpy(np.ascontiguousarray(aop, dtype=np.int32)).cuda()
    Xd = torch.empty(n * r * b, dtype=torch.float64, device="cuda")
    Xn = torch.empty_like(Xd)
    Xl = torch.empty(n * (r + 1) * b, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    ms_f = _timed(lambda: H.frame_lift_dev(r, d, n, Td.data_ptr(), Y, Fd.data_ptr(), K, fo.data_ptr(), Xd.data_ptr(),
                                           s.cuda_stream), s, args.warmup, args.reps)
    ms_n = _timed(lambda: H.frame_lift_dev(r, d, n, Td.data_ptr(), Y, None, 0, None, Xn.data_ptr(), s.cuda_stream),
                  s, args.warmup, args.reps)
    ms_l = _timed(lambda: H.lift_escape_dev(r, d, n, Xd.data_ptr(), None, 0.0, Xl.data_ptr(), s.cuda_stream),
                  s, args.warmup, args.reps)
    bytes_f = 8.0 * n * (d * b + r * b) + 4.0 * n
    bytes_n = 8.0 * n * (d * b + r * b)
    bytes_l = 8.0 * n * (r * b + (r + 1) * b)

    def rate(nbytes, ms):
        return nbytes / (statistics.median(ms) * 1e-3) / 1e12

    # end to end: set_trajectory against set_X of the same X, alternating (one warm-up call each allocates the staging)
    eng.set_trajectory(Tflat, Y, frames)
    X0 = np.empty(n * r * b)
    eng.get_X_into(X0)
    same = bool(np.array_equal(X0, Xd.cpu().numpy()))
    eng.set_X(X0)
    e_traj, e_x = [], []
    for _ in range(args.e2e_reps):
        t0 = time.perf_counter()
        eng.set_trajectory(Tflat, Y, frames)
        e_traj.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        eng.set_X(X0)
        e_x.append((time.perf_counter() - t0) * 1e3)
    out = {"poses": n, "r": r, "d": d, "agents": K, "reps": args.reps, "warmup": args.warmup,
           "frame_lift_ms_median": statistics.median(ms_f), "frame_lift_ms_min": min(ms_f),
           "frame_lift_ms_max": max(ms_f), "frame_lift_bytes": bytes_f, "frame_lift_TB_per_s": rate(bytes_f, ms_f),
           "frame_lift_noframes_ms_median": statistics.median(ms_n), "frame_lift_noframes_ms_min": min(ms_n),
           "frame_lift_noframes_ms_max": max(ms_n), "frame_lift_noframes_bytes": bytes_n,
           "frame_lift_noframes_TB_per_s": rate(bytes_n, ms_n),
           "plain_lift_ms_median": statistics.median(ms_l), "plain_lift_ms_min": min(ms_l),
           "plain_lift_ms_max": max(ms_l), "plain_lift_bytes": bytes_l, "plain_lift_TB_per_s": rate(bytes_l, ms_l),
           "set_trajectory_ms_median": statistics.median(e_traj), "set_trajectory_ms_all": e_traj,
           "set_X_ms_median": statistics.median(e_x), "set_X_ms_all": e_x,
           "set_trajectory_upload_bytes": 8.0 * n * d * b, "set_X_upload_bytes": 8.0 * n * r * b,
           "engine_equals_kernel_bitwise": same}
    for name, ms, nb in [("k_frame_lift (64 frames)", ms_f, bytes_f), ("k_frame_lift (no frames)", ms_n, bytes_n),
                         ("k_lift_escape plain lift", ms_l, bytes_l)]:
        print(f"{name}: {statistics.median(ms) * 1e3:.1f} us median of {args.reps} ({min(ms) * 1e3:.1f} .. "
              f"{max(ms) * 1e3:.1f}), {nb / 1e6:.0f} MB -> {rate(nb, ms):.2f} TB/s", flush=True)
    print(f"Rbcd.set_trajectory: {statistics.median(e_traj):.1f} ms median of {args.e2e_reps} ({min(e_traj):.1f} .. "
          f"{max(e_traj):.1f}), {8.0 * n * d * b / 1e6:.0f} MB uploaded; Rbcd.set_X: {statistics.median(e_x):.1f} ms "
          f"({min(e_x):.1f} .. {max(e_x):.1f}), {8.0 * n * r * b / 1e6:.0f} MB uploaded; engine X bitwise the "
          f"kernel's: {same}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
