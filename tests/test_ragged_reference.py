"""The ragged graph (tests/_ragged.py) keeps the kernels' fallback paths in reach, and its edge-by-edge
extended-precision reference agrees with the float64 oracle: checked on the CPU, before any GPU test relies on either."""
import numpy as np
import pytest

from oracle import dpgo_oracle as O
from tests import _ragged as RG
from tests._common import random_point, random_tangent, seeded_G


@pytest.mark.parametrize("d", [2, 3])
def test_profile(d):
    """Per d: a tile unstaged by its incidences alone, one by its records alone, one by both, the others staged with
    margin; hubs of degree 8..11 with first and second visits, outgoing and incoming; a hub in an unstaged tile; one
    pose without measurements; one parallel and one antiparallel pair; a last tile of fewer than 8 poses."""
    meas, T = RG.ragged_graph(d)
    prof = RG.assert_profile(meas)
    assert T.shape == (d, (d + 1) * meas.num_poses)
    assert np.all((meas.kappa >= 0.5) & (meas.kappa <= 50) & (meas.tau >= 0.5) & (meas.tau <= 50))
    print(f"d={d}: n {meas.num_poses}, m {meas.m}, ni {prof['ni'].tolist()}, ne {prof['ne'].tolist()}, "
          f"max degree {int(prof['degree'].max())}")
    # deterministic: the same graph on every machine
    again, _ = RG.ragged_graph(d)
    assert np.array_equal(again.p1, meas.p1) and np.array_equal(again.R, meas.R) and np.array_equal(again.tau, meas.tau)
    # the ground truth nearly satisfies the measurements (noise 0.05)
    b = d + 1
    for e in range(0, meas.m, 97):
        i, j = int(meas.p1[e]), int(meas.p2[e])
        Ri, Rj = T[:, i * b:i * b + d], T[:, j * b:j * b + d]
        assert np.linalg.norm(Ri @ meas.R[e] - Rj) < 0.5
        assert np.linalg.norm(T[:, j * b + d] - T[:, i * b + d] - Ri @ meas.t[e]) < 0.5


def test_profile_ragged_agents():
    """RAGGED_AGENTS: the one-pose agent and both poses of the two-pose agent have shared edges only."""
    meas, _ = RG.ragged_graph(3)
    prof = RG.tile_profile(meas.p1, meas.p2, RG.RAGGED_AGENTS)
    assert sum(RG.RAGGED_AGENTS) == meas.num_poses
    assert prof["count"].tolist()[:6] == [1, 63, 64, 64, 1, 2]
    only_shared = np.nonzero((prof["degree"] == 0) & (prof["shared"] > 0))[0].tolist()
    assert only_shared == [0, RG.CUT[0], RG.CUT[1]]


def _rel(a, ref):
    ref = np.asarray(ref, np.longdouble)
    return float(np.linalg.norm((np.asarray(a) - ref).astype(float)) / max(float(np.linalg.norm(ref.astype(float))), 1e-300))


@pytest.mark.parametrize("d,r", [(3, 5), (3, 8), (2, 2), (2, 7)])
def test_edge_reference_matches_oracle(d, r):
    meas, _ = RG.ragged_graph(d)
    n = meas.num_poses
    P = O.QuadraticProblem(n, d, r)
    P.set_Q(O.connection_laplacian(meas, n))
    X = random_point(r, d, n, 11)
    V = random_tangent(X, d, 12)
    G = seeded_G(X, d, r, n, 13)
    P.set_G(G)
    ref = RG.edge_reference(meas, X, G, V)
    errs = dict(f=abs(P.f(X) - float(ref["f"])) / abs(float(ref["f"])), egrad=_rel(P.egrad(X), ref["egrad"]),
                ehvp=_rel(P.ehvp(V), ref["ehvp"]), riegrad=_rel(P.riegrad(X), ref["riegrad"]),
                rhvp=_rel(P.rhvp(X, V), ref["rhvp"]))
    print(d, r, {k: f"{v:.1e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= 1e-13, (k, v)


def test_edge_reference_agent_blocks():
    """With the endpoints of other agents set to -1 the reference is the principal submatrix of the global Laplacian
    on the agent's poses (private edges in full, shared edges on the diagonal only)."""
    d, r = 3, 4
    meas, _ = RG.ragged_graph(d)
    n, b = meas.num_poses, d + 1
    Q = O.connection_laplacian(meas, n)
    off = np.concatenate([[0], np.cumsum(RG.RAGGED_AGENTS)])
    X = random_point(r, d, n, 5)
    for k in (0, 4, 5):
        lo, hi = int(off[k]), int(off[k + 1])
        sel = np.nonzero(((meas.p1 >= lo) & (meas.p1 < hi)) | ((meas.p2 >= lo) & (meas.p2 < hi)))[0]
        sub = meas.subset(sel)
        p1 = np.where((sub.p1 >= lo) & (sub.p1 < hi), sub.p1 - lo, -1)
        p2 = np.where((sub.p2 >= lo) & (sub.p2 < hi), sub.p2 - lo, -1)
        Xk = X[:, lo * b:hi * b]
        got = RG.edge_apply(sub, Xk, p1, p2)
        want = (Q[lo * b:hi * b, lo * b:hi * b] @ Xk.T).T
        assert _rel(want, got) <= 1e-13
