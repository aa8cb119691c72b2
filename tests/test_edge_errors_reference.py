"""CPU checks of the ground the edge-error GPU tests stand on (tests/_edges.py): the np.longdouble restatement
against the oracle's computeMeasurementError edge by edge, the identity 1/2 sum err = 1/2 <Q, X^T X> against the
assembled connection Laplacian, and the bound on the noise-free graph where the cancellation is total."""
import numpy as np

from oracle import dpgo_oracle as O
from tests import _edges as EE
from tests._common import load_meas, random_point, unit_laplacian

_L = np.longdouble
R_LIFT = 5


def _small():
    meas = load_meas("smallGrid3D")
    return meas, EE.meas_arrays(meas), random_point(R_LIFT, meas.d, meas.num_poses, 41)


def test_restatement_equals_oracle_measurement_error():
    meas, A, X = _small()
    d = meas.d
    ref = EE.edge_errors(X, d, **A)
    P = O.to_poses(X, R_LIFT, d)
    assert len(ref["err"]) == len(A["p1"]) > 100
    for e in range(len(A["p1"])):
        i, j = int(A["p1"][e]), int(A["p2"][e])
        want = O.measurement_error(A["R"][e], A["t"][e], P[i][:, :d], P[i][:, d], P[j][:, :d], P[j][:, d],
                                   A["kappa"][e], A["tau"][e])
        assert abs(float(ref["err"][e]) - want) <= 1e-13 * want, e
    assert np.all(ref["err"] == _L(1) * A["kappa"] * ref["rot"] + _L(1) * A["tau"] * ref["tra"])


def test_half_sum_of_errors_is_the_quadratic_cost():
    meas, A, X = _small()
    ref = EE.edge_errors(X, meas.d, **A)
    c, _ = EE.cost(ref["err"])
    Q = unit_laplacian(A, meas.num_poses)
    f = 0.5 * float(np.sum(np.asarray((Q @ X.T).T) * X))
    assert abs(float(c) - f) <= 1e-12 * abs(f)
    w = np.random.default_rng(5).uniform(0.0, 1.0, len(A["p1"]))
    cw, Aw = EE.cost(ref["err"], w)
    assert float(cw) < float(c) and float(Aw) == float(cw)


def test_depths_and_bounds_are_the_stated_ones():
    assert EE.sq_depth(3, 5) == 17 and EE.sq_depth(2, 2) == 6
    # one block: product, wave butterfly, four wave sums; the finishing block's butterfly and wave sums
    assert EE.cost_depth(1) == EE.cost_depth(256) == 1 + 6 + 3 + 6 + 15
    assert EE.cost_depth(256 * 1024) == EE.cost_depth(1)
    assert EE.cost_depth(256 * 1024 + 1) == EE.cost_depth(1) + 1
    assert EE.cost_depth(3 * 10 ** 6) == EE.cost_depth(1) + 11


def test_noise_free_graph_stays_inside_its_own_bound():
    """Measurements made of the ground truth's relative poses: every difference cancels to rounding, err_ref is the
    rounding of the fixture itself, and it sits below the bound's first-order term (which does not vanish with v)."""
    for d in (2, 3):
        A, T = EE.noise_free(d)
        ref = EE.edge_errors(T, d, **A)
        assert np.all(ref["err"] >= 0) and float(ref["err"].max()) < 1e-24
        assert np.all(ref["err"] <= ref["err_bound"])
        assert np.all(ref["rot"] <= ref["rot_bound"]) and np.all(ref["tra"] <= ref["tra_bound"])
        lifted = O.lifting_matrix(d, d + 2) @ T
        ref = EE.edge_errors(lifted, d, **A)
        assert np.all(ref["err"] <= ref["err_bound"])
