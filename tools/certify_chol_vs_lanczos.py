#!/usr/bin/env python3
"""Both certificates on the same converged iterate of a grid3d problem: the thick-restarted Lanczos one
(Graph.certify, basis 500 and seed_x as tools/certify_c4.py runs it) and the one by factorisation
(Graph.certify_chol: Cholesky test of S(X) + eta I, bracket, inverse iteration).  The iterate is the RBCD engine's at
tools/certify_c4.py's stop rule (central |RieGrad| < --gradnorm-tol, or --max-seconds).

Usage on the GPU box:  python tools/certify_chol_vs_lanczos.py --k 20 [--eta 1e-3] [--out FILE]
Prints one JSON object: per certifier wall seconds, lambda_min, iterations / factorisations; a factor refused for
its size is reported as such with the refusal's text (and no speed-up)."""
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
    ap.add_argument("--chol-tol", type=float, default=0.0, help="inverse iteration's tol (0: the default, 1e-8)")
    ap.add_argument("--lanczos-iters", type=int, default=30000)
    ap.add_argument("--lanczos-basis", type=int, default=500)
    ap.add_argument("--lanczos-tol", type=float, default=1e-8)
    ap.add_argument("--skip-lanczos", action="store_true", help="only ask whether the factor is accepted, and time it")
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
    ckw = dict(tol=a.chol_tol) if a.chol_tol > 0.0 else {}
    tc = time.time()
    try:
        c = g.certify_chol(X, a.r, eta, want_vector=True, **ckw)
        c.pop("eigvec", None)
        out["chol"] = dict(c, seconds=round(time.time() - tc, 3), panel_gib=8.0 * c["panel_doubles"] / 2.0 ** 30)
        tc = time.time()  # again: the symbolic analysis is per handle, the second call shows what a warm library costs
        c2 = g.certify_chol(X, a.r, eta, want_vector=False, **ckw)
        out["chol_second_call_seconds"] = round(time.time() - tc, 3)
        assert c2["certified"] == c["certified"]
    except H.DPGOHipError as e:
        out["chol"] = {"refused": str(e), "seconds": round(time.time() - tc, 3)}
    print(json.dumps(out), flush=True)
    if not a.skip_lanczos:
        tc = time.time()
        c = g.certify(X, a.r, max_iters=a.lanczos_iters, tol=a.lanczos_tol, basis=a.lanczos_basis, seed_x=True)
        out["lanczos"] = dict({k: v for k, v in c.items() if k not in ("T_rounded", "eigvec")},
                              seconds=round(time.time() - tc, 3))
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
