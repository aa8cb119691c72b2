"""One measurement of the rank reduction's kernels (k_gram + k_gram_finish, k_rank_project) and of the engine's reduced
readout at the headline shape: grid3d k = 100 (10^6 poses), d = 3, r = 5, 64 cube agents, X = the engine's iterate
after --steps colour updates from the chain initialisation.

  kernels     HIP events around each dpgo_hip_gram_dev (two launches) and each dpgo_hip_rank_reduce_dev (to k = 3 and
              k = 4, W = the leading eigenvectors of the Gram) on device buffers of this script, --reps launches after
              --warmup, the median with min .. max; algorithmic bytes 8 r b n for the Gram and 8 (r + k) b n for the
              reduce
  yardstick   the plain lift of k_lift_escape (v = NULL, rank r -> r + 1: the same streaming shape, 8 n (r b + (r+1) b)
              bytes) on the same X, in the same process with the same launch counts
  end to end  host clock around Rbcd.get_X_reduced_into (kernel, k b doubles per pose to the host, scatter to the
              global order; it synchronises) against Rbcd.get_X_into (r b doubles per pose), alternating, the median
              of --e2e-reps calls each with min .. max

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

CEILING_TB_S = 6.3  # the streaming ceiling of DESIGN 3.8 - 3.10


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
    ap.add_argument("--steps", type=int, default=2)
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
    eng = H.Rbcd(g, aop, np.zeros(K, np.int32), 0, 1, H.rbcd_params(r=r, acceleration=1))
    eng.set_X(g.chain_init(r, H.lifting_matrix(d, r)))
    for it in range(args.steps):
        eng.pre_exchange(it % eng.num_colors)
        eng.update(it % eng.num_colors, None)
    X0 = np.empty(n * r * b)
    eng.get_X_into(X0)

    Xd = torch.from_numpy(X0).cuda()
    Cd = torch.empty(r * r, dtype=torch.float64, device="cuda")
    Wk = torch.empty(H.gram_work_doubles(r, d, n), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    ms_g = _timed(lambda: H.gram_dev(r, d, n, Xd.data_ptr(), Cd.data_ptr(), Wk.data_ptr(), s.cuda_stream), s,
                  args.warmup, args.reps)
    Cm = Cd.cpu().numpy().reshape(r, r).T.copy()
    w, U = H.gram_eig(Cm)
    print(f"Gram spectrum / w_1: {(w / w[0]).tolist()}; tr C / (d n) - 1 = {Cm.trace() / (d * n) - 1:.2e}", flush=True)
    rows = [("k_gram + k_gram_finish", ms_g, 8.0 * r * b * n)]
    outs = {}
    for k in (3, 4):
        Ok = torch.empty(n * k * b, dtype=torch.float64, device="cuda")
        W = U[:, :k]
        ms = _timed(lambda: H.rank_reduce_dev(r, d, n, Xd.data_ptr(), W, Ok.data_ptr(), s.cuda_stream), s,
                    args.warmup, args.reps)
        rows.append((f"k_rank_project {r} -> {k}", ms, 8.0 * (r + k) * b * n))
        outs[k] = Ok.cpu().numpy()
        del Ok
    Xl = torch.empty(n * (r + 1) * b, dtype=torch.float64, device="cuda")
    ms_l = _timed(lambda: H.lift_escape_dev(r, d, n, Xd.data_ptr(), None, 0.0, Xl.data_ptr(), s.cuda_stream), s,
                  args.warmup, args.reps)
    rows.append(("k_lift_escape plain lift (yardstick)", ms_l, 8.0 * n * (r * b + (r + 1) * b)))

    def rate(nbytes, ms):
        return nbytes / (statistics.median(ms) * 1e-3) / 1e12

    # end to end: get_X_reduced_into (k = 3) against get_X_into, alternating (one warm-up call each allocates staging)
    W3 = U[:, :3]
    Xk = np.empty(n * 3 * b)
    eng.get_X_reduced_into(W3, Xk)
    same = bool(np.array_equal(Xk, outs[3]))
    eng.get_X_into(X0)
    e_red, e_x = [], []
    for _ in range(args.e2e_reps):
        t0 = time.perf_counter()
        eng.get_X_reduced_into(W3, Xk)
        e_red.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        eng.get_X_into(X0)
        e_x.append((time.perf_counter() - t0) * 1e3)
    out = {"poses": n, "r": r, "d": d, "agents": K, "steps": args.steps, "reps": args.reps, "warmup": args.warmup,
           "gram_spectrum": w.tolist(), "get_X_reduced_ms_median": statistics.median(e_red),
           "get_X_reduced_ms_all": e_red, "get_X_ms_median": statistics.median(e_x), "get_X_ms_all": e_x,
           "get_X_reduced_download_bytes": 8.0 * n * 3 * b, "get_X_download_bytes": 8.0 * n * r * b,
           "engine_equals_kernel_bitwise": same, "kernels": {}}
    for name, ms, nb in rows:
        out["kernels"][name] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "bytes": nb,
                                "TB_per_s": rate(nb, ms), "of_ceiling": rate(nb, ms) / CEILING_TB_S}
        print(f"{name}: {statistics.median(ms) * 1e3:.1f} us median of {args.reps} ({min(ms) * 1e3:.1f} .. "
              f"{max(ms) * 1e3:.1f}), {nb / 1e6:.0f} MB -> {rate(nb, ms):.2f} TB/s "
              f"({100 * rate(nb, ms) / CEILING_TB_S:.0f} % of {CEILING_TB_S} TB/s)", flush=True)
    print(f"Rbcd.get_X_reduced_into (k = 3): {statistics.median(e_red):.1f} ms median of {args.e2e_reps} "
          f"({min(e_red):.1f} .. {max(e_red):.1f}), {8.0 * n * 3 * b / 1e6:.0f} MB downloaded; Rbcd.get_X_into: "
          f"{statistics.median(e_x):.1f} ms ({min(e_x):.1f} .. {max(e_x):.1f}), {8.0 * n * r * b / 1e6:.0f} MB "
          f"downloaded; engine's reduced X bitwise the kernel's: {same}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
