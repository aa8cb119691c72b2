"""One measurement of the edge-error kernel (k_edge_errors + k_edge_cost_finish) and of the engine's error readout
at the headline shape: grid3d k = 100 (10^6 poses), r = 5, 64 cube agents, the engine at its distributed
initialisation (tools/readout_bench.py's protocol).

  lifted      HIP events around each dpgo_hip_edge_errors_dev launch pair over the whole graph's edges on the
              engine's X (copied to device buffers of this script), --reps launches after --warmup, the median with
              min and max; once with err and the cost as outputs, once with all four
  rounded     the same at r = d on the trajectory dpgo_hip_round_se_dev gives
  algorithmic bytes per launch: per edge 8 (d^2 + d + 2) + 8 for the measurement and the two indices, plus 8 per
              per-edge output array; per pose 8 r (d + 1), counted once
  end to end  host clock around Rbcd.errors_into (kernel + the copy-back + the scatter to the graph's edge order; it
              synchronises), lifted and rounded, the median of --e2e-reps calls

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

CEILING_TB_S = 6.3  # the streaming ceiling measured on this part


def _time(launch, s, warmup, reps):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        launch()
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
    n, m = g.n, g.m
    arr = g.arrays()
    dev = {k: torch.from_numpy(np.ascontiguousarray(arr[k]).ravel()).cuda() for k in ("p1", "p2", "R", "t", "kappa", "tau")}
    X = torch.from_numpy(np.ascontiguousarray(X0)).cuda()
    T = torch.empty(n * d * b, dtype=torch.float64, device="cuda")
    outs = [torch.empty(m, dtype=torch.float64, device="cuda") for _ in range(3)]
    cost = torch.empty(1, dtype=torch.float64, device="cuda")
    work = torch.empty(H.edge_errors_work_doubles(m), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    H.round_se_dev(r, d, n, X.data_ptr(), None, T.data_ptr(), s.cuda_stream)

    def launcher(rank, P, all_outputs):
        extra = dict(rot_sq_dev=outs[1].data_ptr(), tra_sq_dev=outs[2].data_ptr()) if all_outputs else {}
        return lambda: H.edge_errors_dev(rank, d, n, m, dev["p1"].data_ptr(), dev["p2"].data_ptr(), dev["R"].data_ptr(),
                                         dev["t"].data_ptr(), dev["kappa"].data_ptr(), dev["tau"].data_ptr(), None,
                                         P.data_ptr(), err_dev=outs[0].data_ptr(), cost_dev=cost.data_ptr(),
                                         work_dev=work.data_ptr(), stream_ptr=s.cuda_stream, **extra)

    out = {"poses": n, "edges": m, "r": r, "d": d, "agents": A ** 3, "reps": args.reps, "warmup": args.warmup,
           "ceiling_TB_per_s": CEILING_TB_S}
    legs = (("lifted", r, X, False), ("lifted_all_outputs", r, X, True), ("rounded", d, T, False),
            ("rounded_all_outputs", d, T, True))
    for name, rank, P, all_outputs in legs:
        ms = _time(launcher(rank, P, all_outputs), s, args.warmup, args.reps)
        arrays = 3 if all_outputs else 1
        nbytes = m * (8.0 * (d * d + d + 2) + 8.0 + 8.0 * arrays) + 8.0 * rank * b * n
        med = statistics.median(ms)
        tbs = nbytes / (med * 1e-3) / 1e12
        out[name] = {"us_median": med * 1e3, "us_min": min(ms) * 1e3, "us_max": max(ms) * 1e3,
                     "algorithmic_bytes": nbytes, "TB_per_s": tbs, "cost": float(cost.cpu()[0])}
        print(f"k_edge_errors {name} (r = {rank}): {med * 1e3:.1f} us median of {args.reps} ({min(ms) * 1e3:.1f} .. "
              f"{max(ms) * 1e3:.1f}), {nbytes / 1e6:.0f} MB -> {tbs:.2f} TB/s ({100 * tbs / CEILING_TB_S:.0f} % of "
              f"{CEILING_TB_S} TB/s)", flush=True)
    # the engine's own path gives the same errors
    err_k = outs[0].cpu().numpy().copy()  # the rounded leg's, computed last
    for name, kw in (("lifted", {}), ("rounded", dict(rounded=True))):
        e = np.full(m, np.nan)
        eng.errors_into(e, **kw)  # warm-up: builds the engine's table on the device
        times = []
        for _ in range(args.e2e_reps):
            t0 = time.perf_counter()
            eng.errors_into(e, **kw)
            times.append((time.perf_counter() - t0) * 1e3)
        out[f"errors_into_{name}_ms_median"] = statistics.median(times)
        out[f"errors_into_{name}_ms_all"] = times
        print(f"Rbcd.errors_into {name}: {statistics.median(times):.1f} ms median of {args.e2e_reps} "
              f"({min(times):.1f} .. {max(times):.1f}), {8.0 * m / 1e6:.0f} MB copied back", flush=True)
    out["engine_rounded_equals_kernel_bitwise"] = bool(np.array_equal(e, err_k))
    print(f"engine's rounded errors bitwise the kernel's: {out['engine_rounded_equals_kernel_bitwise']}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
