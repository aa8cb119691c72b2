"""Host entry points of the pairwise consistency check (no GPU): dpgo_pair_consistency_host and dpgo_max_clique
against the model of tests/_pcm.py, dpgo_graph_pcm and dpgo_graph_distributed_init_ex(DPGO_ALIGN_PCM, use_gpu = 0)
on the fixtures whose ground tests/test_pcm_reference.py asserts (60 % of every agent pair's shared closures
corrupted: rotation alone, translation alone, both).

Distance of every non-root agent's frame from the L2 alignment of the planted inliers alone (chordal for the rotation,
Euclidean for the translation), align="pcm" / align="robust" on the same corrupted input:
  3D (odometry local trajectories, c_t = 1.5)
    agent 1  6.0e-16, 9.9e-16 / 0.0418, 0.674;  agent 2  7.4e-16, 1.9e-15 / 0.0355, 1.08;
    agent 3  5.8e-16, 1.6e-15 / 0.0324, 2.40
  2D (chordal local trajectories, c_t = 4.5)
    agent 1  1.6e-16, 2.0e-15 / 0.000425, 2.04;  agent 2  0, 2.0e-15 / 0.00111, 1.78;
    agent 3  1.1e-16, 3.6e-15 / 0.00173, 0.532
The robust alignment decides on rotations alone: its rotations are close, and every closure with the right rotation
and a wrong translation enters its translation mean (at 60 % outliers its rotation inliers are no longer sure
either)."""
import numpy as np
import pytest

from tests import _frames as F
from tests import _pcm as P


@pytest.fixture(scope="module")
def H():
    from dpgo_amd import hip
    return hip


def check_against_model(H, case, out, dense=True):
    """bits, degrees, symmetry, diagonal, padding and (dense) e of a pair_consistency result against the model"""
    go, wo = case["group_off"], out["word_off"]
    assert np.array_equal(wo, H.pair_consistency_words(go))
    dense_off = np.concatenate([[0], np.cumsum(np.diff(go).astype(np.int64) ** 2)])
    for g, (Fk, xk, _) in enumerate(P.groups_of(case)):
        mg = len(xk)
        W = (mg + 63) // 64
        assert wo[g + 1] - wo[g] == mg * W
        A = H.adjacency_matrix(out["adj"], wo, go, g)
        Am = P.adjacency(Fk, xk, case["c_R"], case["c_t"])
        assert np.array_equal(A, Am), g
        assert np.array_equal(A, A.T) and not A.diagonal().any()
        assert np.array_equal(out["degree"][go[g]:go[g + 1]], A.sum(axis=1))
        rows = out["adj"][wo[g]:wo[g + 1]].reshape(mg, W) if mg else np.zeros((0, 0), np.uint64)
        if mg % 64:
            assert not (rows[:, -1] >> np.uint64(mg % 64)).any()  # padding bits
        if dense and mg:
            er, et = P.pair_errors(Fk, xk)
            for name, ref in (("e_rot", er), ("e_tra", et)):
                got = out[name][dense_off[g]:dense_off[g + 1]].reshape(mg, mg)
                assert np.array_equal(got, got.T), (g, name)  # bitwise symmetric
                assert (got[ref == 0] == 0.0).all(), (g, name)  # the diagonal, exactly
                rel = np.abs(got - ref)[ref > 0] / ref[ref > 0]  # every entry on its own, relative
                assert rel.size == 0 or float(rel.max()) <= 1e-12, (g, name)


@pytest.mark.parametrize("d", [2, 3])
def test_pair_consistency_host_matches_model(H, d):
    case = P.multi_group(d)
    out = H.pair_consistency_host(P.flat_frames(case["F"]), case["x"], d, case["group_off"], case["c_R"], case["c_t"],
                                  dense=True)
    check_against_model(H, case, out)
    plain = H.pair_consistency_host(P.flat_frames(case["F"]), case["x"], d, case["group_off"], case["c_R"],
                                    case["c_t"])
    assert np.array_equal(plain["adj"], out["adj"]) and np.array_equal(plain["degree"], out["degree"])


def duplicate_case(d):
    """every candidate twice: at c_R = c_t = 0 exactly the two copies are consistent (e is exactly 0)"""
    Fk, xk, _ = P.make_group(d, 35, 35, 9)
    return np.concatenate([Fk, Fk]), np.concatenate([xk, xk])


def nan_case(d):
    Fk, xk, _ = P.make_group(d, 70, 70, 10)
    Fk, xk = Fk.copy(), xk.copy()
    Fk[3, 0, 0] = np.nan  # a rotation entry
    Fk[40, 1, d] = np.nan  # a translation entry
    xk[66, 0] = np.nan  # a lever point
    return Fk, xk, (3, 40, 66)


def check_duplicates(H, fn, d):
    Fk, xk = duplicate_case(d)
    out = fn(P.flat_frames(Fk), xk, d, [0, 70], 0.0, 0.0, dense=True)
    A = H.adjacency_matrix(out["adj"], out["word_off"], out["group_off"], 0)
    want = np.zeros((70, 70), bool)
    want[np.arange(35), np.arange(35) + 35] = want[np.arange(35) + 35, np.arange(35)] = True
    assert np.array_equal(A, want)
    assert list(out["degree"]) == [1] * 70
    assert (out["e_rot"].reshape(70, 70)[want] == 0.0).all() and (out["e_tra"].reshape(70, 70)[want] == 0.0).all()


def check_nan(H, fn, d):
    Fk, xk, bad = nan_case(d)
    out = fn(P.flat_frames(Fk), xk, d, [0, 70], 10.0, 10.0)
    A = H.adjacency_matrix(out["adj"], out["word_off"], out["group_off"], 0)
    for k in bad:
        assert not A[k].any() and not A[:, k].any() and out["degree"][k] == 0
    good = np.setdiff1d(np.arange(70), bad)
    assert A[np.ix_(good, good)].sum() == len(good) * (len(good) - 1)  # the inliers of make_group, all consistent
    nanc = fn(P.flat_frames(Fk), xk, d, [0, 70], np.nan, 10.0)
    assert not nanc["adj"].any() and not nanc["degree"].any()


@pytest.mark.parametrize("d", [2, 3])
def test_duplicates_and_nan_host(H, d):
    check_duplicates(H, H.pair_consistency_host, d)
    check_nan(H, H.pair_consistency_host, d)


def test_max_clique_matches_bron_kerbosch(H):
    for i, A in enumerate(P.clique_cases()):
        members, proven = H.max_clique(H.pack_adjacency(A))
        assert proven, i
        assert len(members) == len(P.bron_kerbosch(A)[0]), i
        assert P.is_clique(A, members) and list(members) == sorted(set(members)), i
        greedy, gp = H.max_clique(H.pack_adjacency(A), node_budget=0)
        assert not gp and list(greedy) == P.greedy_clique(A), i


def test_max_clique_planted_budget_and_degenerate(H):
    A, planted = P.planted_clique_graph()
    members, proven = H.max_clique(H.pack_adjacency(A))
    assert proven and np.array_equal(members, planted)
    greedy, gp = H.max_clique(H.pack_adjacency(A), node_budget=0)
    assert not gp and list(greedy) == P.greedy_clique(A) and P.is_clique(A, greedy)
    # a budget that ends the search early: a graph on which the greedy clique is not maximum, so the root node alone
    # cannot prove anything
    B = next(c for c in P.clique_cases() if len(P.greedy_clique(c)) < len(P.bron_kerbosch(c)[0]))
    few, fp = H.max_clique(H.pack_adjacency(B), node_budget=1)
    assert not fp and P.is_clique(B, few) and len(P.greedy_clique(B)) <= len(few) <= len(P.bron_kerbosch(B)[0])
    again, _ = H.max_clique(H.pack_adjacency(B), node_budget=1)
    assert np.array_equal(few, again)  # deterministic
    none, p0 = H.max_clique(np.zeros((0, 1), np.uint64), m=0)
    assert len(none) == 0 and p0
    one, p1 = H.max_clique(np.zeros((1, 1), np.uint64))
    assert list(one) == [0] and p1
    iso, p3 = H.max_clique(H.pack_adjacency(np.zeros((3, 3), bool)))
    assert list(iso) == [0] and p3  # no edge: the greedy incumbent, the lowest index, stands
    full = ~np.eye(130, dtype=bool)
    alln, pa = H.max_clique(H.pack_adjacency(full))
    assert list(alln) == list(range(130)) and pa


@pytest.mark.parametrize("fixture", [P.fixture3d, P.fixture2d])
def test_graph_pcm_recovers_the_planted_labels(H, fixture):
    fx = fixture()
    g = P.graph_of(H, fx)
    ei, info = g.pcm(fx["aop"], fx["T_local"], max_translation_error=fx["c_t"])
    assert np.array_equal(ei, fx["labels"])
    G = P.graph_candidates(fx["d"], fx["p1"], fx["p2"], fx["R"], fx["t"], fx["aop"], fx["T_local"])
    sizes = np.array([len(v[0]) for v in G.values()])
    assert info["groups"] == len(G) and info["candidates"] == sizes.sum() == fx["shared"].sum()
    assert info["pair_tests"] == (sizes.astype(np.int64) ** 2).sum()
    assert info["inliers"] == (fx["labels"] == 1).sum() and info["unproven"] == 0
    ratio = min((~fx["bad"][es]).sum() / len(es) for es, _, _ in G.values())
    assert info["min_clique_ratio"] == ratio
    # a budget of 0 still answers (the greedy cliques) and says that nothing was proven
    ei0, info0 = g.pcm(fx["aop"], fx["T_local"], max_translation_error=fx["c_t"], clique_node_budget=0)
    assert info0["unproven"] == info0["groups"] and set(np.unique(ei0)) <= {0, 1, 255}


@pytest.mark.parametrize("fixture", [P.fixture3d, P.fixture2d])
def test_init_pcm_is_the_l2_alignment_of_the_planted_inliers(H, fixture):
    fx = fixture()
    d, K, aop = fx["d"], fx["K"], fx["aop"]
    g = P.graph_of(H, fx)
    T, frames, info = g.distributed_init_ex(aop, local=fx["local"], align="pcm", max_translation_error=fx["c_t"])
    if fx["local"] == "odometry":
        assert np.abs(T - fx["T_local"]).max() <= 1e-12
    want = P.subset_alignment(d, fx["p1"], fx["p2"], fx["R"], fx["t"], aop, K, T, ~fx["bad"])
    used = info["edge_inlier"] != 255
    assert np.array_equal(info["edge_inlier"][used], fx["labels"][used])
    assert np.array_equal(info["parent"], want["parent"])
    assert np.array_equal(info["candidates"], want["candidates"])
    assert np.array_equal(info["inliers"], want["inliers"])
    assert used.sum() == info["candidates"].sum()
    assert np.abs(frames - want["frames"]).max() <= 1e-12
    root = int(aop[0])
    assert np.array_equal(frames[root], np.hstack([np.eye(d), np.zeros((d, 1))]))
    _, fr_rob, _ = g.distributed_init_ex(aop, local=fx["local"], align="robust")
    for a in range(K):
        if a == root:
            continue
        pr, pt = F.frame_distance(frames[a], want["frames"][a])
        rr, rt = F.frame_distance(fr_rob[a], want["frames"][a])
        print(f"agent {a}: pcm {pr:.3g} {pt:.3g}  robust {rr:.3g} {rt:.3g}")
        assert pr <= 1e-12 and pt <= 1e-12
        assert rt > 1e-3 and rt > pt, (a, rt, pt)  # farther than that


def test_agent_with_only_outlier_closures_is_aligned_on_one(H):
    """The all-outlier agent of test_host_robust_init.test_agent_with_only_outlier_closures_is_refused: the last agent
    keeps two shared closures, both outliers.  The two candidates are mutually inconsistent, the group's graph has no
    edge, the maximum clique has size 1 and is the greedy incumbent, candidate 0 (equal degrees, the lower index).
    PCM therefore aligns the agent on that one closure, where the GNC refuses: a single closure cannot be told from
    an inlier, and candidates = 2 with inliers = 1 is the caller's sign of it."""
    fx = F.fixture3d()
    aop, p1, p2 = fx["aop"], fx["p1"], fx["p2"]
    A = fx["K"] - 1
    mine = np.nonzero((aop[p1] == A) != (aop[p2] == A))[0]
    keep = np.ones(len(p1), bool)
    keep[mine[2:]] = False
    R, t = fx["R_clean"].copy(), fx["t_clean"].copy()
    rng = np.random.default_rng(3)
    for e in mine[:2]:
        R[e] = F._random_rotation(rng, 3)
        t[e] += rng.normal(0.0, 5.0, size=3)
    p1, p2, R, t = p1[keep], p2[keep], R[keep], t[keep]
    g = H.Graph.from_arrays(3, fx["n"], p1, p2, R, t, fx["kappa"][keep], fx["tau"][keep])
    T, frames, info = g.distributed_init_ex(aop, local="odometry", align="pcm", max_translation_error=1.5)
    assert info["candidates"][A] == 2 and info["inliers"][A] == 1
    last = np.nonzero(info["edge_inlier"] != 255)[0][-2:]
    assert list(info["edge_inlier"][last]) == [1, 0]
    use = np.zeros(len(p1), bool)
    use[info["edge_inlier"] == 1] = True
    want = P.subset_alignment(3, p1, p2, R, t, aop, fx["K"], T, use)
    assert np.abs(frames - want["frames"]).max() <= 1e-12


def test_errors(H):
    fx = P.fixture3d()
    g = P.graph_of(H, fx)
    with pytest.raises(H.DPGOHipError, match="max_translation_error") as ei:
        g.distributed_init_ex(fx["aop"], local="odometry", align="pcm")
    assert ei.value.code == -1
    with pytest.raises(H.DPGOHipError, match="max_translation_error"):
        g.pcm(fx["aop"], fx["T_local"])
    case = P.multi_group(3)
    Ff, x, go = P.flat_frames(case["F"]), np.asarray(case["x"]), case["group_off"]
    with pytest.raises(H.DPGOHipError, match="d must be 2 or 3") as e4:
        H.pair_consistency_host(np.zeros((2, 20)), np.zeros((2, 4)), 4, [0, 2], 1.0, 1.0)
    assert e4.value.code == -1
    with pytest.raises(H.DPGOHipError, match="descends"):
        H.pair_consistency_host(Ff, x, 3, [0, 200, 100, len(x)], 1.0, 1.0, capacity=10 ** 6)
    with pytest.raises(H.DPGOHipError, match="end at m"):
        H.pair_consistency_host(Ff, x, 3, go[:-1], 1.0, 1.0)
    need = int(H.pair_consistency_words(go)[-1])
    with pytest.raises(H.DPGOHipError, match=f"needs {need} words, the capacity is {need - 1}"):
        H.pair_consistency_host(Ff, x, 3, go, 1.0, 1.0, capacity=need - 1)
    with pytest.raises(H.DPGOHipError, match="capacity"):
        H.pair_consistency_words(go, capacity=need - 1)
    with pytest.raises(H.DPGOHipError, match="descends"):
        H.pair_consistency_words([0, 5, 3])
    import ctypes as C
    L = H.lib()
    gp = go.ctypes.data_as(C.POINTER(C.c_int))
    adj = np.zeros(need, np.uint64)
    deg = np.zeros(len(x), np.int32)
    args = lambda **kw: [kw.get("d", 3), len(x), kw.get("F", Ff.ctypes.data_as(H._dp)), kw.get("x", x.ctypes.data_as(H._dp)),
                         len(go) - 1, kw.get("go", gp), 1.0, 1.0, kw.get("adj", adj.ctypes.data_as(H._ullp)), need,
                         kw.get("deg", deg.ctypes.data_as(H._ip)), None, None]
    for null in ("F", "x", "go", "adj", "deg"):
        assert L.dpgo_pair_consistency_host(*args(**{null: None})) == -1, null
        assert b"null" in L.dpgo_hip_last_error()
    assert L.dpgo_pair_consistency_host(*args()) == 0
    size, proven = C.c_int(), C.c_int()
    rows = H.pack_adjacency(np.zeros((70, 70), bool))
    cl = np.zeros(70, np.int32)
    assert L.dpgo_max_clique(70, 1, rows.ctypes.data_as(H._ullp), -1, cl.ctypes.data_as(H._ip), C.byref(size),
                             C.byref(proven)) == -1  # 70 vertices need two words per row
    assert L.dpgo_max_clique(70, 2, None, -1, cl.ctypes.data_as(H._ip), C.byref(size), C.byref(proven)) == -1
    assert L.dpgo_max_clique(70, 2, rows.ctypes.data_as(H._ullp), -1, cl.ctypes.data_as(H._ip), None,
                             C.byref(proven)) == -1
    # the dense outputs' cap is 2^26 entries over all groups: 8200^2 passes it
    with pytest.raises(H.DPGOHipError, match="DPGO_PCM_DENSE_MAX"):
        H.pair_consistency_host(np.zeros((8200, 12)), np.zeros((8200, 3)), 3, [0, 8200], 1.0, 1.0, dense=True)
