"""One measurement of the SE(d) rounding kernel (k_round_se) and of the engine's trajectory readout at the headline
shape: grid3d k = 100 (10^6 poses), r = 5, 64 cube agents, the engine at its distributed initialisation.

  kernel      HIP events around each dpgo_hip_round_se_dev launch on the engine's X (copied to a device buffer of
              this script), --reps launches after --warmup, the median; algorithmic bytes 8 n (r b + d b).  The
              initialisation is rank d (Y_a^T Y_j already a rotation), so a second timing adds --sigma noise to X
  end to end  host clock around Rbcd.trajectory_into (kernel + the d x b copy-back + the scatter to global order;
              it synchronises), the median of --e2e-reps calls

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--agents-per-axis", type=int, default=4)
    ap.add_argument("--r", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.1, help="noise of the second, perturbed timing")
    args = ap.parse_args()
    assert H.device_count() >= 1, "no gfx950 device visible"
    d, r = 3, args.r
    b = d + 1
    g = H.Graph.grid3d(args.k, seed=0)
    A = args.agents_per_axis
    aop = g.grid_partition(A)
    eng = H.Rbcd(g, aop, np.zeros(A ** 3, np.int32), 0, 1, H.rbcd_params(r=r, acceleration=1))
    t0 = time.time()
    X0, it, rr = g.distributed_init(aop, r, H.lifting_matrix(d, r), gpu=True, rtol=1e-12, max_iters=50000,
                                    dev_layout=True)
    print(f"distributed initialisation: {time.time() - t0:.1f} s ({it} PCG iterations)", flush=True)
    eng.set_X(X0)
    n = g.n
    X = torch.from_numpy(np.ascontiguousarray(X0)).cuda()
    T = torch.empty(n * d * b, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    for _ in range(args.warmup):
        H.round_se_dev(r, d, n, X.data_ptr(), None, T.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        H.round_se_dev(r, d, n, X.data_ptr(), None, T.data_ptr(), s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    kernel_ms = statistics.median(ms)
    nbytes = 8.0 * n * (r * b + d * b)
    # the same launch on poses pushed off the rank-d set (Y_a^T Y_j no longer a rotation: more Jacobi sweeps)
    Xn = X + args.sigma * torch.randn(X.shape, dtype=torch.float64, device="cuda",
                                      generator=torch.Generator(device="cuda").manual_seed(0))
    Tn = torch.empty_like(T)
    ms_n = []
    for i in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        H.round_se_dev(r, d, n, Xn.data_ptr(), None, Tn.data_ptr(), s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        if i >= args.warmup:
            ms_n.append(e0.elapsed_time(e1))
    noisy_ms = statistics.median(ms_n)
    # the engine's own path gives the same poses
    Tflat = np.full(n * d * b, np.nan)
    eng.trajectory_into(Tflat)  # warm-up: allocates the engine's buffer
    same = bool(np.array_equal(Tflat, T.cpu().numpy()))
    e2e = []
    for _ in range(args.e2e_reps):
        t0 = time.perf_counter()
        eng.trajectory_into(Tflat)
        e2e.append((time.perf_counter() - t0) * 1e3)
    out = {"poses": n, "r": r, "d": d, "kernel_ms_median": kernel_ms, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
           "reps": args.reps, "warmup": args.warmup, "algorithmic_bytes": nbytes,
           "kernel_TB_per_s": nbytes / (kernel_ms * 1e-3) / 1e12, "perturbed_sigma": args.sigma,
           "perturbed_kernel_ms_median": noisy_ms, "perturbed_kernel_TB_per_s": nbytes / (noisy_ms * 1e-3) / 1e12,
           "get_trajectory_ms_median": statistics.median(e2e),
           "get_trajectory_ms_all": e2e, "copy_back_bytes": 8.0 * n * d * b, "engine_equals_kernel_bitwise": same}
    print(f"k_round_se: {kernel_ms * 1e3:.1f} us median of {args.reps} ({min(ms) * 1e3:.1f} .. {max(ms) * 1e3:.1f}), "
          f"{nbytes / 1e6:.0f} MB -> {out['kernel_TB_per_s']:.2f} TB/s", flush=True)
    print(f"k_round_se on X + {args.sigma} noise: {noisy_ms * 1e3:.1f} us median -> "
          f"{out['perturbed_kernel_TB_per_s']:.2f} TB/s", flush=True)
    print(f"Rbcd.trajectory_into: {out['get_trajectory_ms_median']:.1f} ms median of {args.e2e_reps} "
          f"({8.0 * n * d * b / 1e6:.0f} MB copied back); bitwise the kernel's poses: {same}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
