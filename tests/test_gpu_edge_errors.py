"""GPU tests of the edge-error kernel (dpgo_hip_edge_errors and its _dev form, Graph.edge_errors) against the
np.longdouble restatement and the bounds of tests/_edges.py (tests/test_edge_errors_reference.py checks that ground
on the CPU), and of the cost against f of an edge-stream problem handle.  Build-defined batch form of
computeMeasurementError (src/DPGO_utils.cpp:509-515)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _edges as EE
from tests import _ragged as RG
from tests._common import random_point

pytestmark = pytest.mark.gpu
_L = np.longdouble
NAMES = ("err", "rot_sq", "tra_sq", "cost")


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


@functools.lru_cache(maxsize=None)
def _ragged(d):
    meas, T = RG.ragged_graph(d)
    A = EE.meas_arrays(meas)
    for a in A.values():
        a.setflags(write=False)
    return meas, A, T


@functools.lru_cache(maxsize=None)
def _point(d, r, n=RG.N_POSES):
    X = random_point(r, d, n, 7000 + 100 * d + 10 * r + n)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _weights(m):
    """Random weights in [0, 1] with exact zeros and ones among them.  Read-only."""
    w = np.random.default_rng(m).uniform(0.0, 1.0, m)
    w[::7] = 0.0
    w[3::11] = 1.0
    w.setflags(write=False)
    return w


def _within(got, ref, bound):
    return np.all(np.abs(np.asarray(got).astype(_L) - ref) <= bound)


# ---------------------------------------------------------------------------------------- ragged graph
@pytest.mark.parametrize("d,r", EE.SUPPORTED)
def test_ragged_graph_errors_within_bound(hip, d, r):
    """err, rot_sq and tra_sq of every edge of the ragged graph at a random point within tests/_edges.py's bounds
    (k = r d + 2 for err); err is bitwise kappa rot_sq + tau tra_sq of the kernel's own outputs (two rounded products,
    one addition: the kernel forms it from the same registers); the parallel edges agree bitwise in rot_sq and tra_sq
    (same poses, measurements equal up to their own noise: compared through a copy of the measurement)."""
    meas, A, _ = _ragged(d)
    X = _point(d, r)
    ref = EE.edge_errors(X, d, **A)
    out = hip.edge_errors(X, d, **A)
    m = len(A["p1"])
    assert all(out[k].shape == (m,) for k in NAMES[:3])
    worst = float(np.max(np.abs(out["err"].astype(_L) - ref["err"]) / ref["err_bound"]))
    print(f"edge errors d={d} r={r}: worst |err - ref| / bound = {worst:.3f}")
    assert _within(out["err"], ref["err"], ref["err_bound"])
    assert _within(out["rot_sq"], ref["rot"], ref["rot_bound"])
    assert _within(out["tra_sq"], ref["tra"], ref["tra_bound"])
    assert np.array_equal(out["err"], A["kappa"] * out["rot_sq"] + A["tau"] * out["tra_sq"])
    # parallel edges: the second copy of PARALLEL given the first one's measurement must reproduce it bitwise
    par = np.nonzero((A["p1"] == RG.PARALLEL[0]) & (A["p2"] == RG.PARALLEL[1]))[0]
    assert len(par) == 2
    B = {k: np.array(v) for k, v in A.items()}
    for k in ("R", "t", "kappa", "tau"):
        B[k][par[1]] = B[k][par[0]]
    twin = hip.edge_errors(X, d, **B)
    for k in NAMES[:3]:
        assert twin[k][par[1]] == twin[k][par[0]] == out[k][par[0]]


@pytest.mark.parametrize("d,r", [(2, 2), (2, 3), (3, 3), (3, 5), (3, 8)])
def test_cost_against_restatement_and_problem_f(hip, d, r):
    """The cost within gamma_k sum|1/2 w err|, k = cost_depth(m), of the restatement's sum 1/2 sum w err in
    np.longdouble over the kernel's own err (which the ragged test ties to the restatement edge by edge), with unit
    weights and with random ones (exact 0 and 1 among them); and within 1e-12 relative of dpgo_hip_f on a
    single-agent edge-stream handle whose set_Q_edges took the same edges and weights."""
    meas, A, _ = _ragged(d)
    X = _point(d, r)
    m = len(A["p1"])
    for w in (None, _weights(m)):
        out = hip.edge_errors(X, d, w=w, **A)
        got = out["cost"]
        want, _ = EE.cost(out["err"], w)
        print(f"cost d={d} r={r} w={'ones' if w is None else 'random'}: |cost - sum| / bound = "
              f"{float(abs(_L(got) - want) / EE.cost_bound(out['err'], w)):.3f}")
        assert EE.cost_within_bound(got, out["err"], w), (got, float(EE.cost(out["err"], w)[0]))
        P = hip.Problem(meas.num_poses, d, r)
        P.set_Q_edges(0, A["p1"], A["p2"], A["R"], A["t"], A["kappa"], A["tau"], w)
        f = float(P.f(X)[0])
        assert abs(got - f) <= 1e-12 * abs(f), (got, f)
    assert hip.edge_errors(X, d, w=np.ones(m), **A)["cost"] == hip.edge_errors(X, d, **A)["cost"]


def test_graph_edge_errors_is_the_array_form(hip):
    d, r = 3, 5
    meas, A, _ = _ragged(d)
    X = _point(d, r)
    g = hip.Graph.from_arrays(d, meas.num_poses, A["p1"], A["p2"], A["R"], A["t"], A["kappa"], A["tau"])
    w = _weights(g.m)
    a, b = hip.edge_errors(X, d, w=w, **A), g.edge_errors(X, r, w=w)
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(g.edge_errors(hip.to_dev_layout(X), r, outputs=("err",))["err"], a["err"])
    with pytest.raises(hip.DPGOHipError):
        g.edge_errors(X, 9)


# ---------------------------------------------------------------------------------------- rounded
@pytest.mark.parametrize("d", [2, 3])
def test_rounded_trajectory_on_the_noise_free_graph(hip, d):
    """T = hip.round_se of a lifted ground truth, evaluated at r = d: the differences cancel to rounding and the
    errors stay finite and within the bound (whose first-order term does not vanish with them)."""
    A, Ttrue = EE.noise_free(d)
    X = O.lifting_matrix(d, d + 2) @ Ttrue
    T = hip.round_se(X, d)
    assert T.shape == Ttrue.shape
    ref = EE.edge_errors(T, d, **A)
    out = hip.edge_errors(T, d, **A)
    assert all(np.isfinite(out[k]).all() for k in NAMES[:3]) and np.isfinite(out["cost"])
    assert np.all(out["err"] >= 0) and out["err"].max() < 1e-20
    assert _within(out["err"], ref["err"], ref["err_bound"])
    assert _within(out["rot_sq"], ref["rot"], ref["rot_bound"])
    assert _within(out["tra_sq"], ref["tra"], ref["tra_bound"])


# ---------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n", [2, 200])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 1000])
def test_shapes_around_the_block_size(hip, m, n):
    """A partial block, one edge short of a block, a full block, one edge into the second, several blocks; on two
    poses (every edge the same pair, both directions) and on 200."""
    for d, r in ((2, 3), (3, 5)):
        A = EE.random_edges(d, n, m)
        X = _point(d, r, n)
        w = _weights(m)
        ref = EE.edge_errors(X, d, **A)
        out = hip.edge_errors(X, d, w=w, **A)
        assert out["err"].shape == (m,)
        assert _within(out["err"], ref["err"], ref["err_bound"])
        assert _within(out["rot_sq"], ref["rot"], ref["rot_bound"])
        assert _within(out["tra_sq"], ref["tra"], ref["tra_bound"])
        assert EE.cost_within_bound(out["cost"], out["err"], w)


# ---------------------------------------------------------------------------------------- pointer forms
def _dev_call(H, X, d, A, w, off, want=NAMES):
    """dpgo_hip_edge_errors_dev on torch buffers, every pointer `off` * 8 bytes past its allocation's start."""
    import torch
    r = X.shape[0]
    n = X.shape[1] // (d + 1)
    m = len(A["p1"])
    keep = []

    def up(a, dtype):
        a = np.array(a).ravel()  # a writable copy: torch.from_numpy refuses read-only arrays
        per = 8 // a.itemsize
        t = torch.empty(off * per + a.size, dtype=dtype, device="cuda")
        t[off * per:].copy_(torch.from_numpy(a))
        keep.append(t)
        return t.data_ptr() + 8 * off

    def room(count):
        t = torch.full((off + count,), float("nan"), dtype=torch.float64, device="cuda")
        keep.append(t)
        return t

    ptr = {k: up(A[k], torch.int32) for k in ("p1", "p2")}
    ptr.update({k: up(A[k], torch.float64) for k in ("R", "t", "kappa", "tau")})
    wp = up(w, torch.float64) if w is not None else None
    xp = up(H.to_dev_layout(X), torch.float64)
    outs = {k: room(1 if k == "cost" else m) for k in want}
    work = room(H.edge_errors_work_doubles(m))
    s = torch.cuda.current_stream()
    H.edge_errors_dev(r, d, n, m, ptr["p1"], ptr["p2"], ptr["R"], ptr["t"], ptr["kappa"], ptr["tau"], wp, xp,
                      **{f"{k}_dev": outs[k].data_ptr() + 8 * off for k in want},
                      work_dev=work.data_ptr() + 8 * off, stream_ptr=s.cuda_stream)
    s.synchronize()
    return {k: outs[k][off:].cpu().numpy() for k in want}


@pytest.mark.parametrize("d,r", [(2, 2), (3, 5), (3, 8)])
def test_pointer_forms_are_bitwise(hip, d, r):
    """Two calls, the _dev form, the _dev form with every pointer 8 bytes off, every subset of the optional outputs,
    and the same edges in another order: the per-edge outputs are bitwise the same (permuted with the edges); the cost
    is bitwise repeatable for one order and within its bound for another."""
    meas, A, _ = _ragged(d)
    X = _point(d, r)
    m = len(A["p1"])
    w = _weights(m)
    first = hip.edge_errors(X, d, w=w, **A)
    again = hip.edge_errors(X, d, w=w, **A)
    for off in (0, 1):
        dev = _dev_call(hip, X, d, A, w, off)
        for k in NAMES[:3]:
            assert np.array_equal(dev[k], first[k]), (k, off)
        assert dev["cost"][0] == first["cost"]
    for k in NAMES:
        assert np.array_equal(again[k], first[k])
    for count in range(1, 4):
        for subset in itertools.combinations(NAMES, count):
            part = hip.edge_errors(X, d, w=w, outputs=subset, **A)
            assert set(part) == set(subset)
            for k in subset:
                assert np.array_equal(part[k], first[k]), subset
    assert _dev_call(hip, X, d, A, w, 0, want=("tra_sq",))["tra_sq"].tobytes() == first["tra_sq"].tobytes()
    perm = np.random.default_rng(d * 10 + r).permutation(m)
    B = {k: np.ascontiguousarray(v[perm]) for k, v in A.items()}
    shuf = hip.edge_errors(X, d, w=w[perm], **B)
    for k in NAMES[:3]:
        assert np.array_equal(shuf[k], first[k][perm]), k
    assert EE.cost_within_bound(shuf["cost"], first["err"], w)
    assert EE.cost_within_bound(first["cost"], first["err"], w)


# ---------------------------------------------------------------------------------------- refusals
def _raw(H, r, d, n, A, X, w=None, null=(), outs=NAMES):
    """dpgo_hip_edge_errors called directly: (rc, outputs) with the outputs NaN-initialised; `null` names the edge
    list's arrays (or 'X', 'E') passed as NULL."""
    m = len(A["p1"])
    hold = {k: np.ascontiguousarray(A[k], dtype=np.int32 if k in ("p1", "p2") else np.float64)
            for k in ("p1", "p2", "R", "t", "kappa", "tau")}
    if w is not None:
        hold["w"] = np.ascontiguousarray(w, dtype=np.float64)
    E = H.Edges(m, *[None if k in null or k not in hold or hold[k].size == 0 else hold[k].ctypes.data
                     for k in ("p1", "p2", "R", "t", "kappa", "tau", "w")])
    x = H.to_dev_layout(X)
    res = {k: np.full(1 if k == "cost" else max(m, 1), np.nan) for k in outs}
    dp = C.POINTER(C.c_double)
    rc = H.lib().dpgo_hip_edge_errors(r, d, n, None if "E" in null else C.byref(E),
                                      None if "X" in null or x.size == 0 else x.ctypes.data_as(dp),
                                      *[res[k].ctypes.data_as(dp) if k in res else None for k in NAMES])
    return rc, res


def test_refusals_leave_the_outputs_untouched(hip):
    d, r, n, m = 3, 5, 50, 40
    A = {k: np.array(v) for k, v in EE.random_edges(d, n, m).items()}
    X = _point(d, r, n)
    EINVAL = 1
    rc, res = _raw(hip, r, d, n, A, X)
    assert rc == 0 and all(np.isfinite(v).all() for v in res.values())

    def refused(rc_res, what):
        rc, res = rc_res
        assert rc != 0, what
        assert all(np.isnan(v).all() for v in res.values()), what
        return rc

    EINVAL = refused(_raw(hip, 9, d, n, A, _point(d, 8, n)), "r = 9")
    for rr, dd in ((2, 3), (1, 2), (5, 4), (5, 1), (0, 3)):
        assert refused(_raw(hip, rr, dd, n, A, X), f"(r, d) = ({rr}, {dd})") == EINVAL
    empty = {k: v[:0] for k, v in A.items()}
    assert refused(_raw(hip, r, d, n, empty, X), "m = 0") == EINVAL
    assert refused(_raw(hip, r, d, 0, A, X), "n = 0") == EINVAL
    assert refused(_raw(hip, r, d, -3, A, X), "n < 0") == EINVAL
    for name in ("E", "X", "p1", "p2", "R", "t", "kappa", "tau"):
        assert refused(_raw(hip, r, d, n, A, X, null=(name,)), f"null {name}") == EINVAL
    assert refused(_raw(hip, r, d, n, A, X, outs=()), "no output") == EINVAL
    for k, (i, j) in enumerate(((7, 7), (-1, 3), (3, -1), (n, 3), (3, n))):
        B = {q: np.array(v) for q, v in A.items()}
        B["p1"][5 * k + 1], B["p2"][5 * k + 1] = i, j
        assert refused(_raw(hip, r, d, n, B, X), f"edge ({i}, {j})") == EINVAL
    assert hip.edge_errors_work_doubles(0) == 0 and hip.edge_errors_work_doubles(-5) == 0
    assert hip.edge_errors_work_doubles(257) == 2
    with pytest.raises(hip.DPGOHipError):  # the _dev form needs the work buffer with the cost
        hip.edge_errors_dev(r, d, n, m, 8, 8, 8, 8, 8, 8, None, 8, cost_dev=8, work_dev=None)
