"""One measurement of the pair-test kernel of the pairwise consistency check (k_pair_consistency, d = 3) at two
shapes: one group of 16,384 candidates (2.7 10^8 pair tests, 65,536 tiles) and 150 groups of 625 (5.9 10^7 pair
tests, 15,000 tiles: the headline graph's touching sub-cube pairs).  40 % of every group are inliers of one frame,
the rest outliers of the three kinds (tests/_pcm.py's generator, restated here so the tool stands alone).

  kernel     dpgo_hip_pair_consistency_bench: the tile table uploaded once, then --reps launches (degree memset +
             kernel) after --warmup, each between two HIP events; the median and min .. max, pair tests per second
             and the fp64 operations per second of the pair test's count (no FMA is formed: 34 multiplications and 46
             additions or subtractions per pair at d = 3)
  host twin  dpgo_pair_consistency_host on the same input, one thread, the host clock, once (the large shape takes
             seconds); the kernel's words and degrees are compared with it bit for bit

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

FLOPS_PER_PAIR = {3: 34 + 46, 2: 17 + 23}


def rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def small_rotations(rng, n, noise):
    v = rng.standard_normal((n, 3)) * noise
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], \
        -v[:, 1], v[:, 0]
    th = np.linalg.norm(v, axis=1)[:, None, None]
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def group(rng, m):
    """m candidates [m, 12] column-major frames and [m, 3] lever points: 40 % inliers, three kinds of outliers"""
    Rt, tt = rotations(rng, 1)[0], rng.uniform(-5, 5, 3)
    R = Rt @ small_rotations(rng, m, 0.01)
    t = tt + rng.normal(0.0, 0.02, (m, 3))
    kind = rng.integers(0, 3, m)
    out = rng.random(m) >= 0.4
    rot = out & (kind != 1)
    R[rot] = rotations(rng, int(rot.sum()))
    tra = out & (kind != 0)
    t[tra] += rng.normal(0.0, 5.0, (int(tra.sum()), 3))
    F = np.concatenate([R.transpose(0, 2, 1).reshape(m, 9), t], axis=1)
    return F, rng.uniform(-5, 5, (m, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host twin (and the comparison with it)")
    args = ap.parse_args()
    assert H.device_count() >= 1, "no gfx950 device visible"
    d, c_R, c_t = 3, 2.0 * np.sqrt(2.0) * np.sin(0.25), 1.0
    rng = np.random.default_rng(0)
    out = {"d": d, "reps": args.reps, "warmup": args.warmup}
    for name, sizes in (("one_group_16384", [16384]), ("150_groups_625", [625] * 150)):
        parts = [group(rng, mg) for mg in sizes]
        F = np.ascontiguousarray(np.concatenate([p[0] for p in parts]))
        x = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
        go = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        m = len(x)
        words = int(H.pair_consistency_words(go)[-1])
        pairs = float(sum(s * s for s in sizes))
        dev = "cuda"
        tF, tx = torch.from_numpy(F).to(dev), torch.from_numpy(x).to(dev)
        adj = torch.empty(words, dtype=torch.int64, device=dev)
        deg = torch.empty(m, dtype=torch.int32, device=dev)
        ms = list(H.pair_consistency_bench(d, m, tF.data_ptr(), tx.data_ptr(), go, c_R, c_t, adj.data_ptr(), words,
                                           deg.data_ptr(), args.warmup, args.reps))
        med = statistics.median(ms)
        rec = {"candidates": m, "groups": len(sizes), "pair_tests": pairs, "tiles": sum(((s + 63) // 64) ** 2 for s in sizes),
               "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "pair_tests_per_s": pairs / (med * 1e-3),
               "fp64_Tops_per_s": pairs * FLOPS_PER_PAIR[d] / (med * 1e-3) / 1e12,
               "adjacency_bytes": 8.0 * words, "mean_degree": float(deg.double().mean().item())}
        print(f"{name}: {med * 1e3:.1f} us median of {len(ms)} ({min(ms) * 1e3:.1f} .. {max(ms) * 1e3:.1f}), "
              f"{rec['pair_tests_per_s'] / 1e9:.1f} G pair tests/s, {rec['fp64_Tops_per_s']:.2f} T fp64 op/s", flush=True)
        if not args.no_host:
            t0 = time.perf_counter()
            host = H.pair_consistency_host(F, x, d, go, c_R, c_t)
            rec["host_twin_ms"] = (time.perf_counter() - t0) * 1e3
            rec["host_over_kernel"] = rec["host_twin_ms"] / med
            same = (np.array_equal(adj.cpu().numpy().view(np.uint64), host["adj"]) and
                    np.array_equal(deg.cpu().numpy(), host["degree"]))
            rec["bits_equal_host"] = bool(same)
            print(f"  host twin: {rec['host_twin_ms']:.0f} ms ({rec['host_over_kernel']:.0f} x the kernel), "
                  f"bits equal: {same}", flush=True)
            assert same
        out[name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
