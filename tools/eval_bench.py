"""One measurement of the trajectory-evaluation kernels at the headline shape: grid3d k = 100 (10^6 poses, about
3 10^6 edges), d = 3, the estimate a rigidly moved, noisy copy of the grid's ground truth.

  kernels     HIP events around each launch pair on device buffers of this script, --reps launches after --warmup,
              the median and min .. max:
                k_traj_moments (+ finish)     algorithmic bytes 2 * 8 d (d+1) per pose read
                k_traj_errors (+ finish)      the same, plus 16 per pose written
                k_relative_poses              2 * 8 d (d+1) gathered + 8 (d^2 + d) written per edge
                k_edge_errors at r = d (RPE)  its own model: 8 (indices) + 8 (d^2 + d + 2) (measurement) + 2 * 8 d (d+1)
                                              gathered + 16 written per edge
  yardstick   k_round_se (r = 5) timed in the same process on its own 256 MB
  end to end  host clock around Rbcd.evaluate (two roundings + moment launches, the host alignment, one rounding +
              error launch, 16 MB copied back and scattered; it synchronises), the median of --e2e-reps calls on a
              64-agent engine holding the lifted estimate

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


def timed(fn, s, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
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
    ap.add_argument("--no-engine", action="store_true", help="skip the Rbcd.evaluate timing")
    args = ap.parse_args()
    assert H.device_count() >= 1, "no gfx950 device visible"
    d, r = 3, args.r
    b = d + 1
    g = H.Graph.grid3d(args.k, seed=0)
    n, m = g.n, g.m
    truth = g.truth()
    rng = np.random.default_rng(0)
    # the estimate: the truth moved by a rigid map, translations with noise 0.1
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    A0 = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    That = A0.T @ truth
    That[:, d::b] += A0.T @ (0.1 * rng.standard_normal((d, n)) - np.array([[30.0], [-20.0], [10.0]]))
    dev = "cuda"
    Th = torch.from_numpy(H.to_dev_layout(That)).to(dev)
    Tt = torch.from_numpy(H.to_dev_layout(truth)).to(dev)
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    out = {"poses": n, "edges": m, "d": d, "reps": args.reps, "warmup": args.warmup}

    def report(name, ms, nbytes):
        med = statistics.median(ms)
        out[name] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "algorithmic_bytes": nbytes,
                     "TB_per_s": nbytes / (med * 1e-3) / 1e12}
        print(f"{name}: {med * 1e3:.1f} us median of {len(ms)} ({min(ms) * 1e3:.1f} .. {max(ms) * 1e3:.1f}), "
              f"{nbytes / 1e6:.0f} MB -> {out[name]['TB_per_s']:.2f} TB/s", flush=True)

    # yardstick: k_round_se on the lifted estimate
    X = torch.from_numpy(H.to_dev_layout(H.lifting_matrix(d, r) @ That)).to(dev)
    Tr = torch.empty(n * d * b, dtype=torch.float64, device=dev)
    report("k_round_se", timed(lambda: H.round_se_dev(r, d, n, X.data_ptr(), None, Tr.data_ptr(), sp), s,
                               args.warmup, args.reps), 8.0 * n * (r * b + d * b))
    del X, Tr
    pose_bytes = 2 * 8.0 * d * b * n
    P = H.traj_moments_len(d)
    mw = torch.empty(P + H.traj_moments_work_doubles(d, n), dtype=torch.float64, device=dev)
    shift = np.concatenate([That[:, d::b].mean(axis=1), truth[:, d::b].mean(axis=1)])
    report("k_traj_moments", timed(lambda: H.traj_moments_dev(d, n, Th.data_ptr(), Tt.data_ptr(), None, shift,
                                                              mw.data_ptr(), mw.data_ptr() + 8 * P, sp), s,
                                   args.warmup, args.reps), pose_bytes)
    Aa, info = H.traj_align(That, truth, d)
    ew = torch.empty(2 * n + 5 + H.traj_errors_work_doubles(d, n), dtype=torch.float64, device=dev)
    e0 = ew.data_ptr()
    report("k_traj_errors", timed(lambda: H.traj_errors_dev(d, n, Th.data_ptr(), Tt.data_ptr(), None, Aa, e0,
                                                            e0 + 8 * n, e0 + 16 * n, e0 + 16 * n + 40, sp), s,
                                  args.warmup, args.reps), pose_bytes + 16.0 * n)
    sums = ew[2 * n:2 * n + 5].cpu().numpy()
    out["ate_rmse"] = float(np.sqrt(sums[1] / sums[0]))
    E = g.arrays()
    p1 = torch.from_numpy(E["p1"]).to(dev)
    p2 = torch.from_numpy(E["p2"]).to(dev)
    Rr = torch.empty(m * d * d, dtype=torch.float64, device=dev)
    tr = torch.empty(m * d, dtype=torch.float64, device=dev)
    report("k_relative_poses", timed(lambda: H.relative_poses_dev(d, n, Tt.data_ptr(), m, p1.data_ptr(), p2.data_ptr(),
                                                                  Rr.data_ptr(), tr.data_ptr(), sp), s,
                                     args.warmup, args.reps), (2 * 8.0 * d * b + 8.0 * (d * d + d)) * m)
    one = torch.ones(m, dtype=torch.float64, device=dev)
    eo = torch.empty(2 * m + 1 + H.edge_errors_work_doubles(m), dtype=torch.float64, device=dev)
    o0 = eo.data_ptr()
    report("k_edge_errors_rpe", timed(lambda: H.edge_errors_dev(d, d, n, m, p1.data_ptr(), p2.data_ptr(), Rr.data_ptr(),
                                                                tr.data_ptr(), one.data_ptr(), one.data_ptr(), None,
                                                                Th.data_ptr(), None, o0, o0 + 8 * m, o0 + 16 * m,
                                                                o0 + 16 * m + 8, sp), s, args.warmup, args.reps),
           (8.0 + 8.0 * (d * d + d + 2) + 2 * 8.0 * d * b + 16.0) * m)
    out["rpe_tra_rmse"] = float(torch.sqrt(eo[m:2 * m].mean()).item())
    if not args.no_engine:
        A = args.agents_per_axis
        aop = g.grid_partition(A)
        t0 = time.time()
        eng = H.Rbcd(g, aop, np.zeros(A ** 3, np.int32), 0, 1, H.rbcd_params(r=r, acceleration=1))
        eng.set_X(H.to_dev_layout(H.lifting_matrix(d, r) @ That))
        eng.set_truth(truth)
        print(f"engine of {A ** 3} agents: {time.time() - t0:.1f} s", flush=True)
        ev = eng.evaluate()  # warm-up: allocates the engine's buffers
        e2e = []
        for _ in range(args.e2e_reps):
            t0 = time.perf_counter()
            ev = eng.evaluate()
            e2e.append((time.perf_counter() - t0) * 1e3)
        out["rbcd_evaluate_ms_median"] = statistics.median(e2e)
        out["rbcd_evaluate_ms_all"] = e2e
        out["rbcd_evaluate_ate_rmse"] = ev["ate_rmse"]
        print(f"Rbcd.evaluate: {out['rbcd_evaluate_ms_median']:.1f} ms median of {args.e2e_reps} "
              f"(ATE rmse {ev['ate_rmse']:.4f}; the kernels' own: {out['ate_rmse']:.4f})", flush=True)
    for k in ("k_traj_moments", "k_traj_errors"):
        out[k]["share_of_round_se_rate"] = out[k]["TB_per_s"] / out["k_round_se"]["TB_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
