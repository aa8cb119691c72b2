"""One measurement of setting measurement weights into an RBCD engine at the headline shape: grid3d k = 100 (10^6
poses), r = 5, 64 cube agents, the engine at the chain initialisation (tools/edge_errors_bench.py's protocol: --reps
timed after --warmup, the median with min and max).

  kernel      HIP events around one k_set_weights launch per colour (dpgo_rbcd_bench_set_weights repeats the launch of
              the host-form call just made, with flags: all four destination ranges)
  host        host clock around Rbcd.set_weights(w, fixed): validation, the two uploads, per colour the gather, the Q
              rebuild and the block-Jacobi inverses; it synchronises
  device      host clock around Rbcd.set_weights_dev on device arrays plus a stream synchronisation
  recreate    beside them, in the same process, the only route there was before: a second engine created over the
              same graph (dpgo_rbcd_create is untouched by this feature), --create-reps times

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


def _stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def _show(name, s, unit="ms", scale=1.0):
    print(f"{name}: {s['ms_median'] * scale:.3f} {unit} median ({s['ms_min'] * scale:.3f} .. {s['ms_max'] * scale:.3f})",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--agents-per-axis", type=int, default=4)
    ap.add_argument("--r", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--create-reps", type=int, default=3)
    args = ap.parse_args()
    assert H.device_count() >= 1, "no gfx950 device visible"
    d, r = 3, args.r
    g = H.Graph.grid3d(args.k, seed=0)
    A = args.agents_per_axis
    aop = g.grid_partition(A)
    ranks = np.zeros(A ** 3, np.int32)
    params = H.rbcd_params(r=r, acceleration=1, robust_cost=H.ROBUST["GNC_TLS"])
    t0 = time.perf_counter()
    eng = H.Rbcd(g, aop, ranks, 0, 1, params)
    first_create = (time.perf_counter() - t0) * 1e3
    eng.set_X(g.chain_init(r, H.lifting_matrix(d, r)))
    m = g.m
    owner = H.weight_owner(g, aop, A ** 3)
    rng = np.random.default_rng(0)
    w = rng.uniform(0.25, 1.0, m)
    fixed = ((owner >= 0) & (np.arange(m) % 3 == 0)).astype(np.uint8)
    out = {"poses": g.n, "edges": m, "r": r, "d": d, "agents": A ** 3, "colours": int(eng.num_colors),
           "reps": args.reps, "warmup": args.warmup, "create_first_ms": first_create}

    # end to end, host form
    ms = []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        eng.set_weights(w, fixed)
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    out["set_weights_host"] = _stats(ms)
    _show("Rbcd.set_weights(w, fixed), host arrays, end to end", out["set_weights_host"])
    back = np.full(m, np.nan)
    eng.weights_into(back)
    assert np.array_equal(back, w)

    # the kernel alone, per colour
    out["kernel"] = []
    for c in range(eng.num_colors):
        for _ in range(args.warmup):
            eng.bench_set_weights(c, 1)
        ms = [eng.bench_set_weights(c, 1) for _ in range(args.reps)]
        s = _stats(ms)
        s["colour"] = c
        out["kernel"].append(s)
        _show(f"k_set_weights colour {c}", s, "us", 1e3)

    # end to end, device form
    wd, fd = torch.from_numpy(w).cuda(), torch.from_numpy(fixed).cuda()
    torch.cuda.synchronize()
    ms = []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        eng.set_weights_dev(wd.data_ptr(), fd.data_ptr())
        torch.cuda.synchronize()  # the engine's stream included
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    out["set_weights_dev"] = _stats(ms)
    _show("Rbcd.set_weights_dev + synchronise, end to end", out["set_weights_dev"])
    eng.weights_into(back)
    assert np.array_equal(back, w)

    # the route that existed before: another engine over the same graph
    ms = []
    for _ in range(args.create_reps):
        t0 = time.perf_counter()
        e2 = H.Rbcd(g, aop, ranks, 0, 1, params)
        ms.append((time.perf_counter() - t0) * 1e3)
        e2.close()
    out["recreate"] = _stats(ms)
    _show(f"a second engine over the same graph (dpgo_rbcd_create, {args.create_reps} times)", out["recreate"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
