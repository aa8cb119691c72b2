"""The pair-test kernel (k_pair_consistency) against its host twin and the model of tests/_pcm.py: identical bits,
degrees and padding on multi-group inputs, the dense e within 1e-12, duplicates and NaN, a group past one tile in both
directions, the device-pointer entry on a non-default stream over poisoned outputs, dpgo_graph_distributed_init_ex
(DPGO_ALIGN_PCM) with use_gpu = 1 against use_gpu = 0, and PCM's mask as the weights of an L2 solve.

The RBCD engine takes no per-edge weights from outside (its weights are its own GNC's), so the end-to-end test runs
the weighted solve on the problem handle that does (set_Q_edges(weight=)), started from the X that
Rbcd.set_trajectory(T, YLift, frames) writes, which is frame_lift(T, YLift, frames, agent_of_pose)."""
import numpy as np
import pytest

from tests import _pcm as P
from tests.test_host_pcm import check_against_model, check_duplicates, check_nan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _same(a, b, dense):
    assert np.array_equal(a["word_off"], b["word_off"])
    assert np.array_equal(a["adj"], b["adj"])  # every word, padding bits included
    assert np.array_equal(a["degree"], b["degree"])
    if dense:
        assert np.array_equal(a["e_rot"], b["e_rot"]) and np.array_equal(a["e_tra"], b["e_tra"])


def _dev_call(H, case, dense, poison=True):
    """pair_consistency_dev on a stream of its own; outputs filled with 0xFF bytes beforehand"""
    import torch
    d = case["d"]
    Ff, x, go = P.flat_frames(case["F"]), np.array(case["x"], dtype=np.float64), case["group_off"]  # writable copies
    m = len(x)
    wo = H.pair_consistency_words(go)
    nd = int((np.diff(go).astype(np.int64) ** 2).sum())
    dev = "cuda:0"
    tF, tx = torch.from_numpy(Ff).to(dev), torch.from_numpy(x).to(dev)
    fill = -1 if poison else 0
    adj = torch.full((max(int(wo[-1]), 1),), fill, dtype=torch.int64, device=dev)
    deg = torch.full((max(m, 1),), fill, dtype=torch.int32, device=dev)
    er = torch.full((max(nd, 1),), float("nan"), dtype=torch.float64, device=dev) if dense else None
    et = torch.full((max(nd, 1),), float("nan"), dtype=torch.float64, device=dev) if dense else None
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    H.pair_consistency_dev(d, m, tF.data_ptr(), tx.data_ptr(), go, case["c_R"], case["c_t"], adj.data_ptr(),
                           int(wo[-1]), deg.data_ptr(), er.data_ptr() if dense else None,
                           et.data_ptr() if dense else None, s.cuda_stream)
    s.synchronize()
    out = dict(adj=adj.cpu().numpy().view(np.uint64)[:int(wo[-1])], word_off=wo, degree=deg.cpu().numpy()[:m],
               group_off=go)
    if dense:
        out["e_rot"], out["e_tra"] = er.cpu().numpy()[:nd], et.cpu().numpy()[:nd]
    return out


@pytest.mark.parametrize("d", [2, 3])
def test_kernel_bits_equal_the_host_twin(hip, d):
    case = P.multi_group(d)
    args = (P.flat_frames(case["F"]), case["x"], d, case["group_off"], case["c_R"], case["c_t"])
    host = hip.pair_consistency_host(*args, dense=True)
    gpu = hip.pair_consistency(*args, dense=True)
    _same(gpu, host, True)
    check_against_model(hip, case, gpu)  # bits equal the model's, dense e within 1e-12 relative
    _same(hip.pair_consistency(*args), host, False)  # without the dense outputs
    dev = _dev_call(hip, case, True)  # device pointers, a stream of its own, poisoned outputs
    _same(dev, host, True)
    _same(_dev_call(hip, case, False), host, False)


@pytest.mark.parametrize("d", [2, 3])
def test_duplicates_and_nan(hip, d):
    check_duplicates(hip, hip.pair_consistency, d)
    check_nan(hip, hip.pair_consistency, d)


def test_one_group_of_a_thousand(hip):
    """16 x 16 tiles, the last row and column tile 40 wide: the tile table past one tile in both directions"""
    case = P.big_group()
    args = (P.flat_frames(case["F"]), case["x"], 3, case["group_off"], case["c_R"], case["c_t"])
    host = hip.pair_consistency_host(*args, dense=True)
    gpu = hip.pair_consistency(*args, dense=True)
    _same(gpu, host, True)
    A = hip.adjacency_matrix(gpu["adj"], gpu["word_off"], gpu["group_off"], 0)
    assert np.array_equal(A, P.adjacency(case["F"], case["x"], case["c_R"], case["c_t"]))
    rows = gpu["adj"].reshape(1000, 16)
    assert not (rows[:, -1] >> np.uint64(1000 % 64)).any()
    members, proven = hip.max_clique(rows)
    assert proven and np.array_equal(members, np.nonzero(case["inlier"])[0])
    _same(_dev_call(hip, case, False), host, False)


def test_empty_inputs(hip):
    z = hip.pair_consistency(np.zeros((0, 12)), np.zeros((0, 3)), 3, [0], 1.0, 1.0)
    assert z["adj"].size == 0 and z["degree"].size == 0
    z = hip.pair_consistency(np.zeros((0, 12)), np.zeros((0, 3)), 3, [0, 0, 0], 1.0, 1.0)
    assert z["adj"].size == 0 and list(z["word_off"]) == [0, 0, 0]
    one = hip.pair_consistency(np.zeros((1, 6)), np.zeros((1, 2)), 2, [0, 0, 1], 1.0, 1.0)
    assert list(one["adj"]) == [0] and list(one["degree"]) == [0]
    with pytest.raises(hip.DPGOHipError, match="d must be 2 or 3"):
        hip.pair_consistency(np.zeros((2, 20)), np.zeros((2, 4)), 4, [0, 2], 1.0, 1.0)
    with pytest.raises(hip.DPGOHipError, match="capacity"):
        hip.pair_consistency(np.zeros((70, 12)), np.zeros((70, 3)), 3, [0, 70], 1.0, 1.0, capacity=139)


@pytest.mark.parametrize("fixture", [P.fixture3d, P.fixture2d])
def test_init_pcm_on_the_device_equals_the_host(hip, fixture):
    fx = fixture()
    g = P.graph_of(hip, fx)
    kw = dict(local="odometry", align="pcm", max_translation_error=fx["c_t"] if fx["local"] == "odometry" else 6.0)
    Th, fh, ih = g.distributed_init_ex(fx["aop"], gpu=False, **kw)
    Tg, fg, ig = g.distributed_init_ex(fx["aop"], gpu=True, **kw)
    assert np.array_equal(Th, Tg) and np.array_equal(fh, fg)
    assert np.array_equal(ih["edge_inlier"], ig["edge_inlier"])
    assert np.array_equal(ih["inliers"], ig["inliers"]) and np.array_equal(ih["candidates"], ig["candidates"])
    assert (ig["inliers"][np.arange(fx["K"]) != fx["aop"][0]] >= 1).all()
    eh, nh = g.pcm(fx["aop"], Th, max_translation_error=kw["max_translation_error"], gpu=False)
    eg, ng = g.pcm(fx["aop"], Th, max_translation_error=kw["max_translation_error"], gpu=True)
    assert np.array_equal(eh, eg) and nh == ng
    if fx["local"] == "odometry":
        assert np.array_equal(eg, fx["labels"])


def test_mask_as_weights_equals_the_graph_without_the_rejected_edges(hip):
    """k = 8 grid in 8 sub-cubes, 60 % of every agent pair's shared closures corrupted.  PCM's mask as 0/1 weights of
    an L2 solve against the same solve on the graph without the rejected edges, both from the lifted PCM
    initialisation: a zero-weight edge contributes exact zeros to Q and to the cost, so the two runs see the same
    numbers, and the costs agree to 1e-12 relative (the sums differ in where the zeros stand, no more)."""
    H = hip
    r, d = 5, 3
    grid = H.Graph.grid3d(8, seed=4, rot_sigma=0.01, trans_sigma=0.01)
    aop = grid.grid_partition(2)
    a = grid.arrays()
    p1, p2 = a["p1"].astype(np.int64), a["p2"].astype(np.int64)
    c_t = 1.5
    R, t, bad = P.corrupt_shared(d, p1, p2, a["R"], a["t"], aop, 31, c_t)
    shared = aop[p1] != aop[p2]
    assert 0.5 <= bad.sum() / shared.sum() <= 0.6
    g = H.Graph.from_arrays(d, grid.n, p1, p2, R, t, a["kappa"], a["tau"])
    T, frames, info = g.distributed_init_ex(aop, local="chordal", align="pcm", max_translation_error=c_t, gpu=True)
    ei, pinfo = g.pcm(aop, T, max_translation_error=c_t, gpu=True)
    assert pinfo["unproven"] == 0 and pinfo["groups"] >= 7
    assert np.array_equal(ei == 255, ~shared)
    mask = (ei != 0).astype(np.float64)
    assert np.array_equal(ei == 0, bad)  # the rejected closures are the corrupted ones
    Y = H.lifting_matrix(d, r)
    X0 = H.frame_lift(T, Y, frames, aop)  # what Rbcd.set_trajectory(T, Y, frames) writes
    params = H.default_params(tr_iterations=3, tr_tolerance=1e-6, tr_initial_radius=100.0, tr_max_inner=20)

    def solve(graph, pp1, pp2, RR, tt, kk, ta, w):
        h = H.Problem(graph.n, d, r)
        h.set_Q_edges(0, pp1, pp2, RR, tt, kk, ta, weight=w)
        X, res = h.optimize(X0, params)
        return X, res

    Xw, rw = solve(g, p1, p2, R, t, a["kappa"], a["tau"], mask)
    keep = mask == 1.0
    g2 = H.Graph.from_arrays(d, grid.n, p1[keep], p2[keep], R[keep], t[keep], a["kappa"][keep], a["tau"][keep])
    Xr, rr = solve(g2, p1[keep], p2[keep], R[keep], t[keep], a["kappa"][keep], a["tau"][keep], None)
    cw = g.edge_errors(Xw, r, w=mask)["cost"]
    cr = g2.edge_errors(Xr, r)["cost"]
    c0 = g.edge_errors(X0, r, w=mask)["cost"]
    print(f"cost: start {c0:.6g}, weighted {cw:.17g}, removed {cr:.17g}, unweighted at the weighted X "
          f"{g.edge_errors(Xw, r)['cost']:.6g}")
    assert cw < c0  # the run descended
    assert cw <= cr * (1 + 1e-12)
    assert abs(cw - cr) <= 1e-12 * cr
