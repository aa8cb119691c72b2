"""GPU tests of the trajectory-evaluation kernels (dpgo_hip_traj_moments / _traj_errors / _relative_poses, their _dev
forms, dpgo_hip_traj_align and dpgo_graph_evaluate) against the np.longdouble restatement and the bounds of
tests/_traj.py (tests/test_traj_reference.py checks that ground on the CPU).  Build-defined, DESIGN 3.16."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _edges as EE
from tests import _traj as TJ

pytestmark = pytest.mark.gpu
_L = np.longdouble
CASES = [(d, n) for d in (2, 3) for n in TJ.POSE_SIZES]
N_EDGE_POSES = 50


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _flat(T):
    return np.ascontiguousarray(np.asarray(T).T).ravel()


@functools.lru_cache(maxsize=None)
def _shift(d, n):
    """The float64 means of the fixture's translations (all poses): a non-zero shift.  Read-only."""
    F = TJ.fixture(d, n)
    s = np.concatenate([TJ.split(F["That"], d)[1].mean(axis=0), TJ.split(F["T"], d)[1].mean(axis=0)])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _Aa(d, n):
    """A generic rigid map in float64: the restated alignment of the fixture, or the known one for n = 1."""
    F = TJ.fixture(d, n)
    Aa = (np.concatenate([F["A0"], F["a0"][:, None]], axis=1) if n < 4
          else TJ.align(F["That"], F["T"], d)[0].astype(np.float64))
    Aa = np.ascontiguousarray(Aa)
    Aa.setflags(write=False)
    return Aa


def _dev(H, arrays, offset):
    """Device copies of float64 / int32 host arrays, each starting `offset` bytes into its own allocation (offset a
    multiple of the item size; torch allocations are aligned far beyond 16 bytes).  (tensors, pointers)."""
    import torch
    keep, ptrs = [], []
    for a in arrays:
        if a is None:
            ptrs.append(None)
            continue
        a = np.array(a)  # a writable contiguous copy: the fixtures are read-only
        k = offset // a.itemsize
        t = torch.zeros(a.size + k + 2, dtype=torch.float64 if a.dtype == np.float64 else torch.int32, device="cuda:0")
        t[k:k + a.size] = torch.from_numpy(a)
        keep.append(t)
        ptrs.append(t.data_ptr() + offset)
    return keep, ptrs


def _moments_dev(H, d, That, T, use, shift, offset):
    import torch
    n = That.shape[1] // (d + 1)
    keep, (pa, pb, pu) = _dev(H, [_flat(That), _flat(T), use], offset)
    P = H.traj_moments_len(d)
    out = torch.zeros(P + H.traj_moments_work_doubles(d, n) + 2, dtype=torch.float64, device="cuda:0")
    k = offset // 8
    base = out.data_ptr() + 8 * k
    H.traj_moments_dev(d, n, pa, pb, pu, shift, base, base + 8 * P)
    torch.cuda.synchronize()
    return out[k:k + P].cpu().numpy()


def _errors_dev(H, d, That, T, use, Aa, offset):
    import torch
    n = That.shape[1] // (d + 1)
    keep, (pa, pb, pu) = _dev(H, [_flat(That), _flat(T), use], offset)
    out = torch.zeros(2 * n + 5 + H.traj_errors_work_doubles(d, n) + 2, dtype=torch.float64, device="cuda:0")
    k = offset // 8
    base = out.data_ptr() + 8 * k
    H.traj_errors_dev(d, n, pa, pb, pu, Aa, base, base + 8 * n, base + 16 * n, base + 16 * n + 40)
    torch.cuda.synchronize()
    o = out[k:k + 2 * n + 5].cpu().numpy()
    return dict(tra_sq=o[:n], rot_sq=o[n:2 * n], sums=o[2 * n:])


# ---------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("d,n", CASES)
def test_moments_within_bound(hip, d, n):
    """Entry by entry within gamma_m sum|terms| of the restatement, m = the depth of the kernel's own summation order
    (<= d + 8 + ceil(n / 64)): with zero and non-zero shift, with and without the mask; the masked result equals the
    compacted arrays' within the same bound; the count is exact."""
    F = TJ.fixture(d, n)
    m = TJ.moments_depth(d, n)
    assert m <= d + 8 + -(-n // 64)
    g = _L(TJ.gamma(m))
    worst = 0.0
    for shift in (None, _shift(d, n)):
        for use in (None, F["use"]):
            got = hip.traj_moments(F["That"], F["T"], d, use, shift)
            ref, mabs = TJ.moments(F["That"], F["T"], d, use, shift)
            err = np.abs(got.astype(_L) - ref)
            assert np.all(err <= g * mabs), (shift is None, use is None, err, g * mabs)
            assert got[0] == (n if use is None else np.count_nonzero(use))
            worst = max(worst, float(np.max(err[1:] / (g * mabs[1:] + _L(1e-300)))))
            if use is not None:
                u = use != 0
                Rh, th = TJ.split(F["That"], d)
                Rt, tt = TJ.split(F["T"], d)
                comp = hip.traj_moments(TJ.join(Rh[u], th[u]), TJ.join(Rt[u], tt[u]), d, None, shift)
                assert comp[0] == got[0]
                assert np.all(np.abs(comp.astype(_L) - got.astype(_L)) <= 2 * g * mabs)
    print(f"moments d={d} n={n}: m = {m}, worst |mom - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("d,n", CASES)
def test_moments_bitwise(hip, d, n):
    """Repeatable, and bitwise the same from device pointers that are 16-byte aligned and from pointers 8 bytes on."""
    F = TJ.fixture(d, n)
    s = _shift(d, n)
    a = hip.traj_moments(F["That"], F["T"], d, F["use"], s)
    assert np.array_equal(a, hip.traj_moments(F["That"], F["T"], d, F["use"], s))
    for off in (0, 8):
        assert np.array_equal(a, _moments_dev(hip, d, F["That"], F["T"], F["use"], s, off)), off
    b = hip.traj_moments(F["That"], F["T"], d)
    assert np.array_equal(b, _moments_dev(hip, d, F["That"], F["T"], None, None, 8))


# ---------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("d,n", CASES)
def test_errors_within_bound(hip, d, n):
    """Per pose within tests/_traj.py's bounds under a generic Aa; an unused pose is NaN; identity Aa equals None
    bitwise; a permutation of the poses permutes the outputs bitwise."""
    F = TJ.fixture(d, n)
    Aa = _Aa(d, n)
    for use in (None, F["use"]):
        out = hip.traj_errors(F["That"], F["T"], d, use, Aa)
        ref = TJ.errors(F["That"], F["T"], d, Aa, use)
        u = TJ._used(n, use)
        assert np.all(np.isnan(out["tra_sq"][~u])) and np.all(np.isnan(out["rot_sq"][~u]))
        et = np.abs(out["tra_sq"][u].astype(_L) - ref["tra"][u])
        er = np.abs(out["rot_sq"][u].astype(_L) - ref["rot"][u])
        print(f"errors d={d} n={n} masked={use is not None}: worst tra {float(np.max(et / ref['tra_bound'][u])):.3f}, "
              f"rot {float(np.max(er / ref['rot_bound'][u])):.3f} of the bound")
        assert np.all(et <= ref["tra_bound"][u]) and np.all(er <= ref["rot_bound"][u])
    a = hip.traj_errors(F["That"], F["T"], d, F["use"], None)
    b = hip.traj_errors(F["That"], F["T"], d, F["use"], np.eye(d, d + 1))
    for k in ("tra_sq", "rot_sq", "sums"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    perm = np.random.default_rng(n).permutation(n)
    Rh, th = TJ.split(F["That"], d)
    Rt, tt = TJ.split(F["T"], d)
    full = hip.traj_errors(F["That"], F["T"], d, None, Aa)
    p = hip.traj_errors(TJ.join(Rh[perm], th[perm]), TJ.join(Rt[perm], tt[perm]), d, None, Aa)
    assert np.array_equal(p["tra_sq"], full["tra_sq"][perm]) and np.array_equal(p["rot_sq"], full["rot_sq"][perm])
    # only some outputs
    one = hip.traj_errors(F["That"], F["T"], d, None, Aa, outputs=("rot_sq",))
    assert list(one) == ["rot_sq"] and np.array_equal(one["rot_sq"], full["rot_sq"])


@pytest.mark.parametrize("d,n", CASES)
def test_sums(hip, d, n):
    """The sums within gamma_m sum|terms| of the np.longdouble sums of the kernel's own per-pose outputs (which the
    test above ties to the restatement), m = tree_depth(n); the maxima are exactly the per-pose maxima; repeatable
    bitwise, and bitwise the same from pointers offset by 8 bytes."""
    F = TJ.fixture(d, n)
    Aa = _Aa(d, n)
    g = _L(TJ.gamma(max(TJ.tree_depth(n), 1)))
    for use in (None, F["use"]):
        out = hip.traj_errors(F["That"], F["T"], d, use, Aa)
        ref, sabs = TJ.sums(out["tra_sq"], out["rot_sq"], use)
        s = out["sums"]
        assert s[0] == ref[0]
        assert np.all(np.abs(s[1:3].astype(_L) - ref[1:3]) <= g * sabs[1:3])
        u = TJ._used(n, use)
        assert s[3] == out["tra_sq"][u].max() and s[4] == out["rot_sq"][u].max()
        again = hip.traj_errors(F["That"], F["T"], d, use, Aa)
        for off in (0, 8):
            dev = _errors_dev(hip, d, F["That"], F["T"], use, Aa, off)
            for k in ("tra_sq", "rot_sq", "sums"):
                assert np.array_equal(out[k], again[k], equal_nan=True), k
                assert np.array_equal(out[k], dev[k], equal_nan=True), (k, off)
    # ranks: the sums of two halves merge to the whole within the same bound, the count and maxima exactly
    if n > 1:
        h = n // 2
        Rh, th = TJ.split(F["That"], d)
        Rt, tt = TJ.split(F["T"], d)
        parts = [hip.traj_errors(TJ.join(Rh[sl], th[sl]), TJ.join(Rt[sl], tt[sl]), d, None, Aa)["sums"]
                 for sl in (slice(0, h), slice(h, n))]
        whole = hip.traj_errors(F["That"], F["T"], d, None, Aa)["sums"]
        merged = hip.merge_traj_sums(parts)
        assert merged[0] == whole[0] and np.array_equal(merged[3:], whole[3:])
        assert np.all(np.abs(merged[1:3] - whole[1:3]) <= 2 * float(g) * whole[1:3])


# ---------------------------------------------------------------------------------------- relative poses
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("m", TJ.EDGE_SIZES)
def test_relative_poses(hip, d, m):
    """Entry by entry within gamma_{d+1} sum|terms|; bitwise under a permutation of the edges; fed to hip.edge_errors
    at r = d with kappa = tau = 1 they reproduce the restated RPE within tests/_edges.py's own bound."""
    n = N_EDGE_POSES
    F = TJ.fixture(d, n)
    p1, p2 = TJ.edges(n, m)
    R, t = hip.relative_poses(F["T"], d, p1, p2)
    assert R.shape == (m, d, d) and t.shape == (m, d)
    Rr, tr, Rabs, tabs = TJ.relative_poses(F["T"], d, p1, p2)
    g = _L(TJ.gamma(d + 1))
    assert np.all(np.abs(R.astype(_L) - Rr) <= g * Rabs)
    assert np.all(np.abs(t.astype(_L) - tr) <= g * tabs)
    perm = np.random.default_rng(m).permutation(m)
    Rp, tp = hip.relative_poses(F["T"], d, p1[perm], p2[perm])
    assert np.array_equal(Rp, R[perm]) and np.array_equal(tp, t[perm])
    one = np.ones(m)
    out = hip.edge_errors(F["That"], d, p1, p2, R, t, one, one)
    ref = EE.edge_errors(F["That"], d, p1, p2, R, t, one, one)
    assert np.all(np.abs(out["rot_sq"].astype(_L) - ref["rot"]) <= ref["rot_bound"])
    assert np.all(np.abs(out["tra_sq"].astype(_L) - ref["tra"]) <= ref["tra_bound"])
    # the estimate is the truth moved rigidly plus noise of 0.05 rad and 0.1: the RPE sees the noise alone (the
    # rotation noise through the lever arm |t_p2 - t_p1| of order 20, so tra_sq is of order 1), not the offset of 10^3
    assert 1e-4 < float(np.mean(out["tra_sq"])) < 100.0 and float(np.max(hip.rot_angle(out["rot_sq"]))) < 1.0
    clean = TJ.fixture(d, n, noise=False)
    out0 = hip.edge_errors(clean["That"], d, p1, p2, R, t, one, one)
    assert float(np.max(out0["tra_sq"])) <= (1e-14 * 3000) ** 2 and float(np.max(out0["rot_sq"])) <= (1e-14) ** 2


# ---------------------------------------------------------------------------------------- the driver and the graph entry
@pytest.mark.parametrize("d,n", [c for c in CASES if c[1] > 1])
def test_traj_align_meets_the_host_bars(hip, d, n):
    F = TJ.fixture(d, n)
    for use in (None, F["use"]):
        Aa, info = hip.traj_align(F["That"], F["T"], d, use)
        ref, rinfo = TJ.align(F["That"], F["T"], d, use)
        dA = float(np.max(np.abs(Aa[:, :d].astype(_L) - ref[:, :d])))
        da = float(np.max(np.abs(Aa[:, d].astype(_L) - ref[:, d])))
        scale = 1.0 + float(np.linalg.norm(rinfo["mu_hat"].astype(np.float64))
                            + np.linalg.norm(rinfo["mu"].astype(np.float64)))
        print(f"traj_align d={d} n={n} masked={use is not None}: |A - ref| = {dA:.2e}, |a - ref| = {da:.2e}")
        assert dA <= 1e-12 and da <= 1e-12 * scale
        A = Aa[:, :d]
        assert np.max(np.abs(A @ A.T - np.eye(d))) <= 1e-14 and np.linalg.det(A) > 0
        assert info["count"] == rinfo["count"] and info["rank"] == rinfo["rank"] == d
    # the noise-free fixture gives back the known map
    G = TJ.fixture(d, n, noise=False)
    Aa, _ = hip.traj_align(G["That"], G["T"], d)
    assert np.max(np.abs(Aa[:, :d] - G["A0"])) <= 1e-12 and np.max(np.abs(Aa[:, d] - G["a0"])) <= 1e-12 * 3000
    assert hip.traj_errors(G["That"], G["T"], d, None, Aa)["sums"][3] <= (1e-12 * 3000) ** 2


@functools.lru_cache(maxsize=None)
def _graph_case(d, n=200, m=600):
    """(arrays of a graph whose measurements are the fixture truth's relative poses, fixture).  Read-only."""
    F = TJ.fixture(d, n)
    p1, p2 = TJ.edges(n, m)
    R, t, _, _ = TJ.relative_poses(F["T"], d, p1, p2)
    one = np.ones(m)
    return dict(p1=p1, p2=p2, R=R.astype(np.float64), t=t.astype(np.float64), kappa=one, tau=one), F


@pytest.mark.parametrize("d", [2, 3])
def test_graph_evaluate_composes_the_entries(hip, d):
    """Graph.evaluate at r = d: per pose bitwise hip.traj_errors under its own Aa, per edge bitwise hip.edge_errors of
    hip.relative_poses of the truth; the means from the sums and the edge cost; the ATE after the least-squares
    alignment is no larger than without alignment or aligned at one pose."""
    A, F = _graph_case(d)
    n, m = 200, len(A["p1"])
    g = hip.Graph.from_arrays(d, n, **A)
    ev = {k: g.evaluate(F["That"], d, F["T"], align=k, pose=3) for k in ("none", "pose", "lsq")}
    assert ev["lsq"]["ate_rmse"] <= ev["pose"]["ate_rmse"] and ev["lsq"]["ate_rmse"] <= ev["none"]["ate_rmse"]
    assert ev["lsq"]["ate_rmse"] < 0.2 < ev["none"]["ate_rmse"]  # translation noise 0.1 per axis; the offset is 10^3
    assert np.array_equal(ev["none"]["Aa"], np.eye(d, d + 1)) and ev["none"]["rank"] == -1
    Aa, info = hip.traj_align(F["That"], F["T"], d)
    assert np.array_equal(ev["lsq"]["Aa"], Aa) and ev["lsq"]["rank"] == info["rank"]
    assert np.array_equal(ev["lsq"]["sigma"], info["sigma"])
    Rh, th = TJ.split(F["That"], d)
    Rt, tt = TJ.split(F["T"], d)
    Ap = Rt[3] @ Rh[3].T
    assert np.max(np.abs(ev["pose"]["Aa"][:, :d] - Ap)) <= 1e-15
    assert np.max(np.abs(ev["pose"]["Aa"][:, d] - (tt[3] - Ap @ th[3]))) <= 1e-12
    # at that pose only rounding is left: |t| of order 10^3 at 2^-53, squared
    assert ev["pose"]["tra_sq"][3] <= (1e-11) ** 2 and ev["pose"]["rot_sq"][3] <= (1e-14) ** 2
    R, t = hip.relative_poses(F["T"], d, A["p1"], A["p2"])
    one = np.ones(m)
    for k, e in ev.items():
        out = hip.traj_errors(F["That"], F["T"], d, None, e["Aa"])
        assert np.array_equal(e["tra_sq"], out["tra_sq"]) and np.array_equal(e["rot_sq"], out["rot_sq"])
        s = out["sums"]
        assert e["count"] == n and e["ate_rmse"] == np.sqrt(s[1] / s[0]) and e["ate_max"] == np.sqrt(s[3])
        assert e["rot_rmse"] == np.sqrt(s[2] / s[0]) and e["rot_max"] == np.sqrt(s[4])
        rpe = hip.edge_errors(F["That"], d, A["p1"], A["p2"], R, t, one, one)
        assert np.array_equal(e["rpe_rot_sq"], rpe["rot_sq"]) and np.array_equal(e["rpe_tra_sq"], rpe["tra_sq"])
        assert e["edges_used"] == m
        assert abs(e["rpe_tra_rmse"] - np.sqrt(np.mean(rpe["tra_sq"]))) <= 1e-13 * e["rpe_tra_rmse"]
        assert abs(e["rpe_rot_rmse"] - np.sqrt(np.mean(rpe["rot_sq"]))) <= 1e-13 * e["rpe_rot_rmse"]
    # the RPE does not see the alignment
    assert ev["none"]["rpe_tra_rmse"] == ev["lsq"]["rpe_tra_rmse"] == ev["pose"]["rpe_tra_rmse"]
    # a mask, with the truth missing (NaN) where it is unused: finite figures over the used poses and edges
    use = F["use"]
    Tm = np.array(F["T"]).reshape(d, n, d + 1)
    Tm[:, use == 0, :] = np.nan
    Tm = Tm.reshape(d, -1)
    e = g.evaluate(F["That"], d, Tm, use=use)
    both = (use[A["p1"]] != 0) & (use[A["p2"]] != 0)
    assert e["count"] == np.count_nonzero(use) and e["edges_used"] == np.count_nonzero(both)
    assert np.isfinite([e["ate_rmse"], e["rot_rmse"], e["rpe_tra_rmse"], e["rpe_rot_rmse"]]).all()
    assert np.array_equal(np.isnan(e["tra_sq"]), use == 0) and np.array_equal(np.isnan(e["rpe_tra_sq"]), ~both)
    assert np.array_equal(e["rpe_tra_sq"][both], ev["lsq"]["rpe_tra_sq"][both])
    Aa_m, _ = hip.traj_align(F["That"], F["T"], d, use)
    assert np.array_equal(e["Aa"], Aa_m)


def test_graph_evaluate_rounds_a_lifted_solution(hip):
    """r > d: the solution is rounded in the frame of its pose `pose` first -- the same figures as evaluating
    hip.round_se's trajectory at r = d."""
    from oracle import dpgo_oracle as O
    d, r = 3, 5
    A, F = _graph_case(d)
    g = hip.Graph.from_arrays(d, 200, **A)
    X = O.lifting_matrix(d, r) @ F["That"]
    anchor = X[:, 7 * (d + 1):8 * (d + 1)]
    a = g.evaluate(X, r, F["T"], pose=7)
    b = g.evaluate(hip.round_se(X, d, anchor), d, F["T"])
    for k in ("tra_sq", "rot_sq", "rpe_rot_sq", "rpe_tra_sq", "Aa"):
        assert np.array_equal(a[k], b[k]), k
    assert a["ate_rmse"] == b["ate_rmse"] and a["rpe_rot_rmse"] == b["rpe_rot_rmse"]


# ---------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(hip):
    L = hip.lib()
    d, n = 3, 129
    F = TJ.fixture(d, n)
    a, b = _flat(F["That"]), _flat(F["T"])
    dp, ip = hip._dp, hip._ip
    pa, pb = a.ctypes.data_as(dp), b.ctypes.data_as(dp)
    mom = np.full(hip.traj_moments_len(d), 7.0)
    tra, rot, sums = np.full(n, 7.0), np.full(n, 7.0), np.full(5, 7.0)
    Aa = np.full(12, 7.0)
    info = hip.AlignInfo()
    info.rank = -7
    pm, pt, pr, ps, pA = (x.ctypes.data_as(dp) for x in (mom, tra, rot, sums, Aa))
    bad = [
        L.dpgo_hip_traj_moments(4, n, pa, pb, None, None, pm),
        L.dpgo_hip_traj_moments(d, 0, pa, pb, None, None, pm),
        L.dpgo_hip_traj_moments(d, n, None, pb, None, None, pm),
        L.dpgo_hip_traj_moments(d, n, pa, None, None, None, pm),
        L.dpgo_hip_traj_moments(d, n, pa, pb, None, None, None),
        L.dpgo_hip_traj_moments(d, n, pa, pb, None, None, a[5:].ctypes.data_as(dp)),  # mom inside That
        L.dpgo_hip_traj_errors(1, n, pa, pb, None, None, pt, pr, ps),
        L.dpgo_hip_traj_errors(d, -1, pa, pb, None, None, pt, pr, ps),
        L.dpgo_hip_traj_errors(d, n, None, pb, None, None, pt, pr, ps),
        L.dpgo_hip_traj_errors(d, n, pa, pb, None, None, None, None, None),
        L.dpgo_hip_traj_errors(d, n, pa, pb, None, None, pt, pt, ps),  # tra_sq and rot_sq the same array
        L.dpgo_hip_traj_errors(d, n, pa, pb, None, None, pt, tra[64:].ctypes.data_as(dp), ps),
        L.dpgo_hip_traj_align(5, n, pa, pb, None, pA, C.byref(info)),
        L.dpgo_hip_traj_align(d, n, pa, pb, None, None, C.byref(info)),
        L.dpgo_hip_traj_align(d, n, pa, pb, np.zeros(n, np.int32).ctypes.data_as(ip), pA, C.byref(info)),  # count = 0
    ]
    assert all(rc != 0 for rc in bad), bad
    p1 = np.array([0, 1, 2], np.int32)
    p2 = np.array([1, 2, 3], np.int32)
    Ro, to = np.full(27, 7.0), np.full(9, 7.0)
    pR, pT = Ro.ctypes.data_as(dp), to.ctypes.data_as(dp)

    def rel(dd, nn, T, m, q1, q2, R=pR, t=pT):
        return L.dpgo_hip_relative_poses(dd, nn, T, m, q1.ctypes.data_as(ip), q2.ctypes.data_as(ip), R, t)
    assert rel(4, n, pb, 3, p1, p2) != 0 and rel(d, 0, pb, 3, p1, p2) != 0 and rel(d, n, pb, 0, p1, p2) != 0
    assert rel(d, n, None, 3, p1, p2) != 0 and rel(d, n, pb, 3, p1, p2, R=None) != 0
    assert rel(d, n, pb, 3, p1, p1) != 0                                   # p1 == p2
    assert rel(d, n, pb, 3, p1, np.array([1, 2, n], np.int32)) != 0        # an index outside [0, n)
    assert rel(d, n, pb, 3, np.array([0, -1, 2], np.int32), p2) != 0
    assert rel(d, n, pb, 3, p1, p2, R=pT) != 0                             # R_out and t_out the same array
    for x in (mom, tra, rot, sums, Aa, Ro, to):
        assert np.all(x == 7.0)
    assert info.rank == -7 and np.array_equal(a, _flat(F["That"]))
    # the _dev entries refuse a missing work buffer
    import torch
    z = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    with pytest.raises(hip.DPGOHipError):
        hip.traj_moments_dev(d, 1, z.data_ptr(), z.data_ptr() + 96, None, None, z.data_ptr() + 192, 0)
    with pytest.raises(hip.DPGOHipError):
        hip.traj_errors_dev(d, 1, z.data_ptr(), z.data_ptr() + 96, None, None, None, None, z.data_ptr() + 192, None)
    # and the good calls go through
    assert rel(d, n, pb, 3, p1, p2) == 0 and not np.any(Ro == 7.0)
    A, _ = _graph_case(d)
    g = hip.Graph.from_arrays(d, 200, **A)
    G = TJ.fixture(d, 200)
    for kw in (dict(align="lsq", pose=200), dict(align="lsq", pose=-1),
               dict(align="pose", pose=1, use=np.where(np.arange(200) == 1, 0, 1))):
        with pytest.raises(hip.DPGOHipError):
            g.evaluate(G["That"], d, G["T"], **kw)
    with pytest.raises(hip.DPGOHipError):
        g.evaluate(G["That"], d, G["T"], align="umeyama")
