"""bench.py --dump-outputs / --full: what a run writes and which legs it runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["X", "X_pose", "status_rel_change", "status_ready"]


def _load(d):
    return {n: np.load(os.path.join(str(d), n + ".npy")) for n in NAMES}


def test_dump_small_is_whole_and_large_is_a_fixed_sample(tmp_path, monkeypatch):
    n, rb = 50, 20
    X = np.arange(n * rb, dtype=np.float64)
    st = np.linspace(0.0, 1.0, 8)
    bench.dump_outputs(str(tmp_path / "a"), n, X, st, np.ones(8))
    a = _load(tmp_path / "a")
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["X"], X.reshape(n, rb)) and np.array_equal(a["X_pose"], np.arange(n))
    assert np.array_equal(a["status_rel_change"], st)
    # above the size cap: the same sorted sample of pose rows on every call
    monkeypatch.setattr(bench, "DUMP_X_BYTES", 8 * rb * 7)
    bench.dump_outputs(str(tmp_path / "b"), n, X, st, np.ones(8))
    bench.dump_outputs(str(tmp_path / "c"), n, X + 1.0, st, np.ones(8))
    b, c = _load(tmp_path / "b"), _load(tmp_path / "c")
    pose = b["X_pose"].astype(int)
    assert len(pose) == 7 and np.all(np.diff(pose) > 0) and np.array_equal(b["X_pose"], c["X_pose"])
    assert np.array_equal(b["X"], X.reshape(n, rb)[pose]) and np.array_equal(c["X"], b["X"] + 1.0)


def test_default_dump_fits_64_mb():
    """The flagship run's dump: the sample of X plus its pose list stay under 64 MB."""
    rb, n = 20, 100 ** 3
    keep = bench.DUMP_X_BYTES // (8 * rb)
    assert keep < n and keep * (8 * rb + 8) + 2 * 8 * 64 + 4 * 128 <= 64 << 20


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--k", "12", "--agents-per-axis", "2",
           "--burnin", "4", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_time_the_same_steps(tmp_path):
    """A plain run reports the headline alone; --full adds the other legs and leaves the timed path's result as it
    was: both dump the same iterate, bitwise."""
    plain = _bench(tmp_path / "plain")
    full = _bench(tmp_path / "full", "--full", "--exact-leg", "0")
    moved = {"central", "xq_spmm", "xq_guard", "hvp", "cpu_baseline", "boundary_regime"}
    for d in (plain, full):
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["tcg"]["updates"] == 3 * 8
        assert d["value"] == pytest.approx(8 * 1e3 / d["ms_per_step"])
    assert not moved & set(plain) and moved <= set(full)
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert a["X"].shape == (12 ** 3, 20) and np.all(np.isfinite(a["X"]))
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
