"""The ground the robust-initialisation tests stand on (no GPU, no native library): the numpy restatement in
tests/_frames.py recovers exactly the corrupted closures on both fixtures, under conditions on the fixtures that a
seeded sweep of the restatement alone meets (200 seeds, 5-50 candidates, 30-80 % outliers, inlier noise 0-0.02 rad:
the exact inlier set every time, within 38 GNC iterations), and it gives the reference's known answers
(tests/testUtils.cpp:72-118)."""
import numpy as np
import pytest

from tests import _frames as F


def _quat_rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("fixture", [F.fixture3d, F.fixture2d])
def test_fixture_conditions_and_exact_inlier_recovery(fixture):
    fx = fixture()
    rb = fx["robust"]
    aop, p1, p2 = fx["aop"], fx["p1"], fx["p2"]
    assert rb["aligned"].all() and sorted(rb["order"]) == list(range(fx["K"]))
    assert fx["shared_bad"].sum() == int(0.3 * (aop[p1] != aop[p2]).sum())
    used_total = 0
    for A in range(fx["K"]):
        P = int(rb["parent"][A])
        if P < 0:
            assert A == aop[0] and rb["candidates"][A] == 0
            continue
        pair = ((aop[p1] == A) & (aop[p2] == P)) | ((aop[p1] == P) & (aop[p2] == A))
        assert np.all(rb["edge_inlier"][pair] != 255)
        good = int((~fx["shared_bad"][pair]).sum())
        assert pair.sum() == rb["candidates"][A]
        assert good >= 5, (A, P, good)
        assert (pair.sum() - good) <= 0.45 * pair.sum(), (A, P, good, int(pair.sum()))
        assert rb["inliers"][A] == good
        used_total += int(pair.sum())
    used = rb["edge_inlier"] != 255
    assert used.sum() == used_total
    # exact: the restatement's flags are the ground-truth corruption flags on every used edge
    assert np.array_equal(rb["edge_inlier"][used] == 0, fx["shared_bad"][used])
    # the odometry is never corrupted, and some private closure is
    local = F.local_index(aop, fx["K"])
    odo = (aop[p1] == aop[p2]) & (local[p2] == local[p1] + 1)
    assert not (fx["shared_bad"] | fx["private_bad"])[odo].any() and fx["private_bad"].any()


def test_single_rotation_is_returned():
    rng = np.random.default_rng(1)
    for _ in range(50):
        Rt = _quat_rotation(rng)
        Ropt, w, iters = F.rotation_average(Rt[None], None, F.angular2chordal(0.5))
        assert np.linalg.norm((Ropt - Rt).astype(np.float64)) <= 1e-8
        assert list(np.nonzero(w > 1 - F.W_TOL)[0]) == [0]


def test_ten_inliers_among_fifty():
    rng = np.random.default_rng(2)
    tol, cbar = F.angular2chordal(0.02), F.angular2chordal(0.3)
    for _ in range(50):
        Rt = _quat_rotation(rng)
        Rs = [Rt] * 10
        while len(Rs) < 50:
            Rr = _quat_rotation(rng)
            if np.linalg.norm(Rr - Rt) > 1.2 * cbar:
                Rs.append(Rr)
        Ropt, w, iters = F.rotation_average(np.array(Rs), None, cbar)
        Ro = Ropt.astype(np.float64)
        assert abs(np.linalg.det(Ro) - 1) < 1e-8 and np.linalg.norm(Ro.T @ Ro - np.eye(3)) < 1e-8
        assert np.linalg.norm(Ro - Rt) <= tol
        assert list(np.nonzero(w > 1 - F.W_TOL)[0]) == list(range(10))


def test_two_dimensional_and_weighted_sets():
    """d = 2 and non-unit kappa: inliers within 0.02 rad of the truth are recovered exactly."""
    rng = np.random.default_rng(3)
    for trial in range(20):
        th = rng.uniform(-np.pi, np.pi)
        n, nin = 20, 12
        ang = np.concatenate([th + rng.uniform(-0.02, 0.02, nin), th + rng.uniform(1.0, 5.0, n - nin)])
        Rs = np.array([[[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]] for a in ang])
        kappa = rng.uniform(0.5, 2.0, n) if trial % 2 else None
        _, w, _ = F.rotation_average(Rs, kappa, F.THRESHOLD)
        assert list(np.nonzero(w > 1 - F.W_TOL)[0]) == list(range(nin))
