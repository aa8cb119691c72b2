"""One measurement of the rank staircase's streaming kernel (k_lift_escape) alone at the headline size: the poses of
grid3d k = 100 (10^6 poses, d = 3), r = 5 -> 6.

  escape      HIP events around each dpgo_hip_lift_escape_dev launch, --reps launches after --warmup, the median;
              algorithmic bytes 8 n (r b + b + (r + 1) b) = 384 MB: X and v in, the lifted poses out
  plain lift  the same with v = NULL (a relayout: no v, no QF), 8 n (r b + (r + 1) b) = 352 MB

The kernel has no data-dependent branch (Gram-Schmidt twice per pose), so the poses are seeded random points of
St(3, r)^n x R^(r n) made on the device and the direction a seeded unit vector; no graph is built.

Needs a gfx950 device; prints one JSON line last."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpgo_amd import hip as H  # noqa: E402


def timed(fn, stream, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--r", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert H.device_count() >= 1, "no gfx950 device visible"
    d, r, n = 3, args.r, args.k ** 3
    b = d + 1
    gen = torch.Generator(device="cuda").manual_seed(0)
    P = torch.randn((n, b, r), dtype=torch.float64, device="cuda", generator=gen)  # pose j: b columns of r (column-major)
    Qf, _ = torch.linalg.qr(P[:, :d, :].transpose(1, 2))  # n x r x d, orthonormal columns
    P[:, :d, :] = Qf.transpose(1, 2)
    X = P.reshape(-1).contiguous()
    v = torch.randn(n * b, dtype=torch.float64, device="cuda", generator=gen)
    v /= torch.linalg.norm(v)
    v *= float(n) ** 0.5  # per-pose entries of order 1 / sqrt(b), as a direction spread over the graph has after scaling
    out = torch.empty(n * (r + 1) * b, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    ms = timed(lambda: H.lift_escape_dev(r, d, n, X.data_ptr(), v.data_ptr(), args.alpha, out.data_ptr(), s.cuda_stream),
               s, args.warmup, args.reps)
    lifted = out.reshape(n, b, r + 1)
    gram = lifted[:, :d, :] @ lifted[:, :d, :].transpose(1, 2)
    orth = float((gram - torch.eye(d, dtype=torch.float64, device="cuda")).abs().max())
    ms0 = timed(lambda: H.lift_escape_dev(r, d, n, X.data_ptr(), None, 0.0, out.data_ptr(), s.cuda_stream),
                s, args.warmup, args.reps)
    plain_ok = bool(torch.equal(out.reshape(n, b, r + 1)[:, :, :r], P) and
                    float(out.reshape(n, b, r + 1)[:, :, r].abs().max()) == 0.0)
    nbytes = 8.0 * n * (r * b + b + (r + 1) * b)
    nbytes0 = 8.0 * n * (r * b + (r + 1) * b)
    med, med0 = statistics.median(ms), statistics.median(ms0)
    res = {"poses": n, "r": r, "d": d, "reps": args.reps, "warmup": args.warmup,
           "kernel_ms_median": med, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "algorithmic_bytes": nbytes,
           "kernel_TB_per_s": nbytes / (med * 1e-3) / 1e12,
           "plain_lift_ms_median": med0, "plain_lift_ms_min": min(ms0), "plain_lift_ms_max": max(ms0),
           "plain_lift_bytes": nbytes0, "plain_lift_TB_per_s": nbytes0 / (med0 * 1e-3) / 1e12,
           "max_orthonormality_defect": orth, "plain_lift_bitwise": plain_ok}
    print(f"k_lift_escape r = {r} -> {r + 1}, {n} poses: {med * 1e3:.1f} us median of {args.reps} "
          f"({min(ms) * 1e3:.1f} .. {max(ms) * 1e3:.1f}), {nbytes / 1e6:.0f} MB -> {res['kernel_TB_per_s']:.2f} TB/s; "
          f"max |Y^T Y - I| = {orth:.1e}", flush=True)
    print(f"plain lift (v = NULL): {med0 * 1e3:.1f} us median ({min(ms0) * 1e3:.1f} .. {max(ms0) * 1e3:.1f}), "
          f"{nbytes0 / 1e6:.0f} MB -> {res['plain_lift_TB_per_s']:.2f} TB/s; bitwise [X; 0]: {plain_ok}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
