#!/usr/bin/env python3
"""The block certificate (Graph.certify_block: LOBPCG on the r lifted rows, with precon 0 and 1) against the
thick-restarted Lanczos one (Graph.certify, basis 500 and seed_x as tools/certify_c4.py runs it) on the same
converged iterate of a grid3d problem.  The iterate is the RBCD engine's at tools/certify_c4.py's stop rule (central
|RieGrad| < --gradnorm-tol, or --max-seconds), as tools/certify_chol_vs_lanczos.py takes it.

Usage on the GPU box:  python tools/certify_block_vs_lanczos.py --k 20 [--skip-lanczos] [--out FILE]
Prints one JSON object: per certifier wall seconds, operator passes, theta_C, lower_bound against -eta, iterations
that dropped P (restarts), and the device memory each path allocates for its vectors, from the allocation sizes (the
block path: six r-row blocks, U and the Gram partials; Lanczos: its basis), not from a probe of the device."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--agents-per-axis", type=int, default=2)
    ap.add_argument("--r", type=int, default=5)
    ap.add_argument("--gradnorm-tol", type=float, default=0.1)
    ap.add_argument("--check", type=int, default=50, help="colour sweeps between central evaluations")
    ap.add_argument("--max-seconds", type=float, default=120.0)
    ap.add_argument("--eta", type=float, default=0.0, help="0: tools/certify_c4.py's 1e-6 |f(X)| / n")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--block-iters", type=int, default=2000)
    ap.add_argument("--lanczos-iters", type=int, default=30000)
    ap.add_argument("--lanczos-basis", type=int, default=500)
    ap.add_argument("--skip-lanczos", action="store_true")
    ap.add_argument("--precons", default="0,1", help="the block path's precon settings to run, comma-separated")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from dpgo_amd import hip as H

    torch.cuda.set_device(0)
    g = H.Graph.grid3d(a.k, seed=0)
    aop = g.grid_partition(a.agents_per_axis)
    eng = H.Rbcd(g, aop, np.zeros(a.agents_per_axis ** 3, np.int32), 0, 1,
                 H.rbcd_params(r=a.r, acceleration=1, robust_cost=H.ROBUST["L2"], precon=H.PRECON_BLOCK_JACOBI))
    X0, _, _ = g.distributed_init(aop, a.r, H.lifting_matrix(3, a.r), gpu=True, rtol=1e-12, max_iters=50000,
                                  dev_layout=True)
    eng.set_X(X0)
    t0, steps = time.time(), 0
    while True:
        f, gn = eng.central_eval(None)
        gn = float(np.sqrt(np.sum(gn)))
        print(f"step {steps:7d}  t {time.time() - t0:7.1f} s  f {f:.10e}  |RG| {gn:.4e}", flush=True)
        if gn < a.gradnorm_tol or time.time() - t0 > a.max_seconds:
            break
        for _ in range(a.check):
            for c in range(eng.num_colors):
                eng.pre_exchange(c)
                eng.update_color(c, None)
        steps += a.check
    torch.cuda.synchronize()
    X = np.zeros(X0.size)
    eng.get_X_into(X)
    del eng
    eta = a.eta if a.eta > 0.0 else 1e-6 * abs(float(f)) / max(g.n, 1)
    out = {"workload": f"grid3d k={a.k} ({g.n} poses, {g.m} edges), r={a.r}, {a.agents_per_axis ** 3} agents",
           "steps": steps, "solve_seconds": round(time.time() - t0, 2), "f": float(f), "gradnorm": gn, "eta": eta}

    def timed(fn):
        torch.cuda.synchronize()
        tc = time.time()
        c = fn()
        sec = time.time() - tc
        c = {k: v for k, v in c.items() if k not in ("T_rounded", "eigvec")}
        return dict(c, seconds=round(sec, 3), certified=bool(c["lower_bound"] >= -eta))

    for precon in [int(x) for x in a.precons.split(",") if x != ""]:
        out[f"block_precon{precon}"] = timed(lambda p=precon: g.certify_block(
            X, a.r, want_vector=False, tol=a.tol, max_iters=a.block_iters, precon=p))
        print(json.dumps({f"block_precon{precon}": out[f"block_precon{precon}"]}), flush=True)
    # what the block path holds on the device: six r-row blocks, U, the Gram partials
    L = a.r * 4 * g.n
    out["block_device_bytes_model"] = 8 * (6 * L + (a.r + 1) * 4 * g.n + 1024 * 3 * a.r * (6 * a.r + 1))
    if not a.skip_lanczos:
        out["lanczos"] = timed(lambda: g.certify(X, a.r, max_iters=a.lanczos_iters, tol=a.tol,
                                                       basis=a.lanczos_basis, seed_x=True))
        out["lanczos_basis_bytes_model"] = 8 * (a.lanczos_basis + a.r + 2) * 4 * g.n
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
