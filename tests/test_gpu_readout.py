"""Solution readout on the GPU: the SE(d) rounding kernel (dpgo_hip_round_se / _dev) against the oracle's
projectToRotationGroup, and the engine's trajectory / loop-closure weight getters (dpgo_rbcd_get_anchor,
_get_trajectory, _get_weights) against the oracle's PGOAgent colour schedule."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests._common import load_meas

pytestmark = pytest.mark.gpu

# the project's bar for evaluations; the rounding error expected here is a few eps / gap (see _gaps)
KERNEL_BAR = 1e-12
MIN_GAP = 0.2


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


# ------------------------------------------------------------------------------------------ inputs and references
def lifted_iterate(d, r, n, sigma):
    """n poses [R_j | t_j] lifted by YLift and perturbed off the rank-d set: R_j = projectToRotationGroup of a
    Gaussian matrix, t_j = 5 Gaussian (default_rng(11), pose by pose), noise sigma default_rng(5)."""
    rng = np.random.default_rng(11)
    b = d + 1
    T = np.zeros((d, b * n))
    for j in range(n):
        T[:, j * b:j * b + d] = O.project_to_rotation(rng.normal(size=(d, d)))
        T[:, j * b + d] = 5.0 * rng.normal(size=d)
    X0 = O.lifting_matrix(d, r) @ T
    return O.lifted_project(X0 + sigma * np.random.default_rng(5).normal(size=X0.shape), d)


def round_reference(X, d, anchor):
    """O.round_to_se in the frame of the lifted pose `anchor` (r x (d+1)); anchor None is O.round_to_se itself."""
    if anchor is None:
        return O.round_to_se(X, d)
    b = d + 1
    Ya = anchor[:, :d]
    T = Ya.T @ X
    t0 = Ya.T @ anchor[:, d]
    for i in range(X.shape[1] // b):
        T[:, i * b:i * b + d] = O.project_to_rotation(T[:, i * b:i * b + d])
        T[:, i * b + d] -= t0
    return T


def gaps(X, d, anchor):
    """Per pose: gap_j = sigma_{d-1}(M_j) + sign(det M_j) sigma_d(M_j) of M_j = Y_a^T Y_j (the projection's condition
    number is about 1 / gap; it is not unique at gap 0), and det M_j."""
    b = d + 1
    Ya = X[:, :d] if anchor is None else anchor[:, :d]
    n = X.shape[1] // b
    M = np.stack([Ya.T @ X[:, j * b:j * b + d] for j in range(n)])
    s = np.linalg.svd(M, compute_uv=False)
    det = np.linalg.det(M)
    return s[:, d - 2] + np.sign(det) * s[:, d - 1], det


def check_rounded(T, Tref, d, label):
    b = d + 1
    n = T.shape[1] // b
    err = float(np.max(np.abs(T - Tref)))
    scale = max(1.0, float(np.max(np.abs(Tref))))
    Rs = np.stack([T[:, j * b:j * b + d] for j in range(n)])
    orth = float(np.max(np.linalg.norm(np.swapaxes(Rs, 1, 2) @ Rs - np.eye(d), axis=(1, 2))))
    dets = np.linalg.det(Rs)
    print(f"{label}: max|T_dev - T_oracle| = {err:.3e} (bar {KERNEL_BAR * scale:.3e}), max|R^T R - I| = {orth:.3e}, "
          f"min det R = {dets.min():.6f}")
    assert err <= KERNEL_BAR * scale
    assert orth <= 1e-13
    assert np.all(dets > 0)


def round_dev(H, X, d, anchor, misalign=False):
    """dpgo_hip_round_se_dev on torch device buffers (misalign: X and T start 8 bytes off a 16-byte boundary, the
    kernel's scalar path)."""
    import torch
    r, b = X.shape[0], d + 1
    n = X.shape[1] // b
    off = 1 if misalign else 0
    xt = torch.empty(off + X.size, dtype=torch.float64, device="cuda")
    xt[off:].copy_(torch.from_numpy(H.to_dev_layout(X)))
    tt = torch.full((off + n * d * b,), float("nan"), dtype=torch.float64, device="cuda")
    at = None
    if anchor is not None:
        at = torch.from_numpy(H.to_dev_layout(anchor)).cuda()
    s = torch.cuda.current_stream()
    H.round_se_dev(r, d, n, xt.data_ptr() + 8 * off, at.data_ptr() if at is not None else None,
                   tt.data_ptr() + 8 * off, s.cuda_stream)
    s.synchronize()
    return H.from_dev_layout(tt[off:].cpu().numpy(), d)


# ------------------------------------------------------------------------------------------ 1. kernel vs oracle
CASES = [(3, 5, 216, 0.3), (3, 8, 216, 0.3), (2, 4, 300, 0.3), (3, 3, 216, 0.2), (2, 2, 300, 0.2),
         (3, 5, 1, 0.3), (3, 5, 65, 0.3)]


@pytest.mark.parametrize("anchor_pose", [None, 7])
@pytest.mark.parametrize("d,r,n,sigma", CASES)
def test_round_se_matches_oracle(hip, d, r, n, sigma, anchor_pose):
    X = lifted_iterate(d, r, n, sigma)
    b = d + 1
    anchor = None
    if anchor_pose is not None:
        # one pose has no pose 7: its anchor is pose 7 of the 65-pose iterate of the same shape
        src = X if n > anchor_pose else lifted_iterate(d, r, 65, sigma)
        anchor = src[:, anchor_pose * b:(anchor_pose + 1) * b].copy()
    gap, det = gaps(X, d, anchor)
    print(f"(d {d}, r {r}, n {n}, sigma {sigma}, anchor {anchor_pose}): min gap {gap.min():.3f}, "
          f"{int((det < 0).sum())} poses with det < 0")
    assert gap.min() >= MIN_GAP
    if r > d and n > 65 and anchor_pose is None:
        assert (det < 0).any()  # the flip branch runs
    Tref = round_reference(X, d, anchor)
    T = hip.round_se(X, d, anchor)
    assert T.shape == Tref.shape
    check_rounded(T, Tref, d, "round_se")
    Td = round_dev(hip, X, d, anchor)
    assert np.array_equal(T, Td)  # the host entry point is the same kernel on staged copies
    assert np.array_equal(T, round_dev(hip, X, d, anchor, misalign=True))  # the 8-byte path moves the same values


# ------------------------------------------------------------------------------------------ 2. crafted flips
@pytest.mark.parametrize("d,r,diag", [(3, 5, (1.0, 0.8, -0.5)), (2, 4, (1.0, -0.5))])
def test_round_se_crafted_flips(hip, d, r, diag):
    """Y_j = Y_0 diag R_j: distinct singular values and det < 0 at every pose, so every pose takes the flip."""
    rng = np.random.default_rng(23)
    n, b = 130, d + 1
    Y0 = O.lifting_matrix(d, r)
    anchor = np.concatenate([Y0, rng.normal(size=(r, 1))], axis=1)
    X = np.zeros((r, b * n))
    Rs = []
    for j in range(n):
        Rj = O.project_to_rotation(rng.normal(size=(d, d)))
        Rs.append(Rj)
        X[:, j * b:j * b + d] = Y0 @ np.diag(diag) @ Rj
        X[:, j * b + d] = 3.0 * rng.normal(size=r)
    gap, det = gaps(X, d, anchor)
    assert np.all(det < 0) and gap.min() >= MIN_GAP
    T = hip.round_se(X, d, anchor)
    check_rounded(T, round_reference(X, d, anchor), d, f"crafted flips d = {d}")
    # U = diag(1, .., -1), V^T = R_j: after the flip the projection is R_j itself
    assert max(np.max(np.abs(T[:, j * b:j * b + d] - Rs[j])) for j in range(n)) <= KERNEL_BAR
    assert np.array_equal(T, round_dev(hip, X, d, anchor))


# ------------------------------------------------------------------------------------------ 3. engine, 3D, robust
def _grid_with_outliers(hip, k, seed, frac, rng_seed):
    """grid3d edges with a fraction of the loop closures (non-consecutive poses) corrupted (the recipe of
    tests/test_gpu_rbcd.py)."""
    g0 = hip.Graph.grid3d(k, seed=seed)
    a = g0.arrays()
    p1, p2 = a["p1"].astype(np.int64), a["p2"].astype(np.int64)
    R, t = a["R"].copy(), a["t"].copy()
    rng = np.random.default_rng(rng_seed)
    lc = np.nonzero(np.abs(p2 - p1) != 1)[0]
    bad = rng.choice(lc, size=max(1, int(frac * len(lc))), replace=False)
    t[bad] += rng.normal(0.0, 5.0, size=(len(bad), 3))
    g = hip.Graph.from_arrays(3, g0.n, p1, p2, R, t, a["kappa"], a["tau"])
    meas = O.Measurements(3, np.zeros(len(p1), np.int64), np.zeros(len(p1), np.int64), p1, p2, R, t,
                          a["kappa"], a["tau"], np.ones(len(p1)), g0.n)
    return g, g0, meas


def _run_engine(H, g, aop, num_agents, X0, iters, r, **kw):
    e = H.Rbcd(g, aop, np.zeros(num_agents, np.int32), 0, 1, H.rbcd_params(r=r, **kw))
    e.set_X(X0)
    for it in range(iters):
        c = it % e.num_colors
        e.pre_exchange(c)
        e.update(c, None)
    return e


def _check_trajectory(H, e, g, d, r, Xo, label):
    """trajectory_into against the oracle's rounding of the engine's own X (the kernel bar) and of the oracle's X
    (the engine's X parity bar, 1e-9)."""
    Xflat = np.zeros(g.n * (d + 1) * r)
    e.get_X_into(Xflat)
    Xe = H.from_dev_layout(Xflat, r)
    Tflat = np.full(g.n * (d + 1) * d, np.nan)
    e.trajectory_into(Tflat)
    T = H.from_dev_layout(Tflat, d)
    assert not np.isnan(T).any()
    gap, _ = gaps(Xe, d, None)
    print(f"{label}: min gap {gap.min():.3f}")
    check_rounded(T, O.round_to_se(Xe, d), d, label + " vs oracle rounding of the engine's X")
    To = O.round_to_se(Xo, d)
    err = float(np.max(np.abs(T - To)))
    print(f"{label}: max|T - round(X_oracle)| = {err:.3e} (bar {1e-9 * np.max(np.abs(To)):.3e})")
    assert err <= 1e-9 * np.max(np.abs(To))
    # an explicit anchor equal to pose 0 is the same frame
    T2 = np.full_like(Tflat, np.nan)
    e.trajectory_into(T2, anchor=e.anchor(0))
    assert np.array_equal(T2, Tflat)
    return T


@pytest.fixture(scope="module")
def outlier_grid(hip):
    k, A, r = 6, 2, 5
    g, g0, meas = _grid_with_outliers(hip, k, 3, 0.1, 7)
    aop = g0.grid_partition(A)
    X0 = g0.chain_init(r, O.lifting_matrix(3, r))  # odometry edges are uncorrupted
    return g, meas, aop, X0, A ** 3, r


@pytest.mark.parametrize("accel", [False, True])
@pytest.mark.parametrize("robust", ["GNC_TLS", "Huber"])
def test_engine_trajectory_and_weights_robust(hip, outlier_grid, robust, accel):
    """Two reweightings (robust_opt_inner_iters = 3, 6 iterations) on a grid with 10 % corrupted loop closures: the
    rounded trajectory and every reported weight against the oracle's PGOAgents.  (TLS is left out: its weight is
    discontinuous in the residual.)"""
    g, meas, aop, X0, K, r = outlier_grid
    iters = 6
    e = _run_engine(hip, g, aop, K, X0, iters, r, acceleration=int(accel), robust_cost=hip.ROBUST[robust],
                    robust_opt_inner_iters=3)
    ags = []
    Xo, _ = O.colour_rbcd(meas, aop, K, X0, iters, r, acceleration=accel, robust=robust, robust_opt_inner_iters=3,
                          agents_out=ags)
    _check_trajectory(hip, e, g, 3, r, Xo, f"{robust} accel={accel}")
    # ---- weights: (global p1, global p2) -> the oracle's weight of the responsible copy
    assert g.duplicates == 0
    glob = [np.nonzero(np.asarray(aop) == a)[0] for a in range(K)]
    ref = {}
    copies = inside = 0
    for ag in ags:
        pl, sh = ag.private_lc, ag.shared_lc
        for x in range(pl.m):
            ref[(int(glob[ag.id][pl.p1[x]]), int(glob[ag.id][pl.p2[x]]))] = float(pl.weight[x])
        for x in range(sh.m):
            r1, r2 = int(sh.r1[x]), int(sh.r2[x])
            if ag.id == min(r1, r2):  # only the lower-ID agent's copy is ever updated
                ref[(int(glob[r1][sh.p1[x]]), int(glob[r2][sh.p2[x]]))] = float(sh.weight[x])
            else:
                assert sh.weight[x] == 1.0
        for w_ in (pl.weight, sh.weight):
            copies += len(w_)
            inside += int(np.sum((w_ > 0.0) & (w_ < 1.0)))
    print(f"{robust} accel={accel}: {inside}/{copies} loop-closure copies strictly inside (0, 1)")
    assert 2 * inside >= copies  # the oracle's weights are not trivial
    w = np.full(g.m, np.nan)
    e.weights_into(w)
    assert not np.isnan(w).any()  # one rank is responsible for every edge
    owner = hip.weight_owner(g, aop, K)
    a = g.arrays()
    p1, p2 = a["p1"].astype(np.int64), a["p2"].astype(np.int64)
    assert np.all(w[owner < 0] == 1.0)  # odometry
    lc = np.nonzero(owner >= 0)[0]
    assert len(lc) == len(ref)
    wref = np.array([ref[(int(p1[k]), int(p2[k]))] for k in lc])
    err = float(np.max(np.abs(w[lc] - wref)))
    print(f"{robust} accel={accel}: max|w - w_oracle| = {err:.3e} over {len(lc)} loop closures (bar 1e-9)")
    assert err <= 1e-9
    assert np.all((w >= 0.0) & (w <= 1.0))


def test_engine_weights_l2_are_one(hip, outlier_grid):
    g, meas, aop, X0, K, r = outlier_grid
    e = _run_engine(hip, g, aop, K, X0, 3, r, acceleration=1)
    w = np.full(g.m, np.nan)
    e.weights_into(w)
    assert np.all(w == 1.0)


# ------------------------------------------------------------------------------------------ 4. engine, 2D
def test_engine_trajectory_2d(hip):
    meas = load_meas("CSAIL")
    d, r, K, iters = 2, 4, 4, 4
    n = meas.num_poses
    aop = np.minimum(np.arange(n) // (n // K), K - 1).astype(np.int32)
    X0 = O.lifting_matrix(d, r) @ O.chordal_initialization(d, n, meas)
    g = hip.Graph.from_arrays(d, n, meas.p1, meas.p2, meas.R, meas.t, meas.kappa, meas.tau)
    e = _run_engine(hip, g, aop, K, X0, iters, r, acceleration=1)
    Xo, _ = O.colour_rbcd(meas, aop, K, X0, iters, r, acceleration=True)
    _check_trajectory(hip, e, g, d, r, Xo, "CSAIL")
    w = np.full(g.m, np.nan)
    e.weights_into(w)
    assert np.all(w == 1.0)


# ------------------------------------------------------------------------------------------ 5. errors
def test_round_se_errors(hip):
    with pytest.raises(hip.DPGOHipError, match="unsupported"):
        hip.round_se(np.zeros((2, 4 * 3)), 3)  # r < d
    with pytest.raises(hip.DPGOHipError, match="unsupported"):
        hip.round_se(np.zeros((9, 4 * 3)), 3)  # no kernel for r = 9
    with pytest.raises(hip.DPGOHipError, match="unsupported"):
        hip.round_se(np.zeros((5, 5 * 3)), 4)  # d = 4
    L = hip.lib()
    x = np.zeros(20)
    xp = x.ctypes.data_as(hip._dp)
    assert L.dpgo_hip_round_se(5, 3, 0, xp, None, xp) == -1  # n <= 0: DPGO_HIP_EINVAL
    assert b"n >= 1" in L.dpgo_hip_last_error()
    assert L.dpgo_hip_round_se(5, 3, 1, None, None, xp) == -1
    assert L.dpgo_hip_round_se(5, 3, 1, xp, None, None) == -1
    assert b"null" in L.dpgo_hip_last_error()
    assert L.dpgo_hip_round_se_dev(5, 3, 1, None, None, None, None) == -1


def test_anchor_round_trip_one_rank(hip):
    g = hip.Graph.grid3d(4, seed=1)
    r, d = 5, 3
    aop = g.grid_partition(2)
    e = hip.Rbcd(g, aop, np.zeros(8, np.int32), 0, 1, hip.rbcd_params(r=r, acceleration=1))
    e.set_X(g.chain_init(r, O.lifting_matrix(d, r)))
    for it in range(2):
        e.pre_exchange(it % e.num_colors)
        e.update(it % e.num_colors, None)
    T = np.full(g.n * (d + 1) * d, np.nan)
    e.trajectory_into(T, anchor=None)  # one rank owns pose 0
    assert not np.isnan(T).any()
    Xflat = np.zeros(g.n * (d + 1) * r)
    e.get_X_into(Xflat)
    X = hip.from_dev_layout(Xflat, r)
    ident = np.concatenate([np.eye(d), np.zeros((d, 1))], axis=1)
    for pose in (0, 17, g.n - 1):
        A = e.anchor(pose)
        assert np.array_equal(A, X[:, pose * (d + 1):(pose + 1) * (d + 1)])
        assert np.max(np.abs(hip.round_se(A, d, A) - ident)) <= 1e-13
    with pytest.raises(hip.DPGOHipError, match="out of range"):
        e.anchor(g.n)
    with pytest.raises(ValueError):
        e.trajectory_into(np.zeros(3))
    with pytest.raises(ValueError):
        e.weights_into(np.zeros(3))
