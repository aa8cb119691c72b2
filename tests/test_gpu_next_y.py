"""Next selection's Y written by the non-selected pass (tuning key TUNE_NEXT_Y = 15).  Under the cyclic colour schedule
the colour that runs iterate(false) now is selected next: its pass (k_polar_vnext, or k_polar_comb when no updateV is
pending) also writes that colour's next updateY, Y = project((1 - alpha') X + alpha' V) with the next iteration's
alpha', and the status reference XPrev = X, from its registers, and the next dpgo_rbcd_pre_exchange skips the selected
colour's own pass when the prediction held.  The same expressions on the same values: iterates, counters, traces and
the agent status are bitwise those of value 0, whether the prediction holds (cyclic schedule), is not made (restart,
GNC reweighting / initializeAcceleration), fails (the caller selects another colour) or is invalidated (set_X,
set_selected).  One rank only: with more ranks the selected colour's pass runs on the side stream as before."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEXT_Y = 15


@pytest.fixture(scope="module")
def hip():
    from dpgo_amd import hip as H
    assert H.device_count() >= 1
    return H


def _coords(k):
    """Grid coordinates of grid3d(k)'s poses: plane by plane, rows and planes traversed boustrophedon."""
    i = np.arange(k ** 3)
    z, idx = i // (k * k), i % (k * k)
    idx = np.where(z & 1, k * k - 1 - idx, idx)
    y, x = idx // k, idx % k
    x = np.where(y & 1, k - 1 - x, x)
    return x, y, z


@functools.lru_cache(maxsize=None)
def _data(k, layout):
    """layout "cubes": two agents per axis (uneven for odd k), two colours.  "tri": three agents that all touch each
    other (the left part, and the right part cut in two), three colours.  Built once per shape, never modified."""
    from dpgo_amd import hip as H
    g = H.Graph.grid3d(k, seed=5)
    x, y, z = _coords(k)
    s = (k + 1) // 2
    if layout == "cubes":
        aop = (x // s + 2 * (y // s + 2 * (z // s))).astype(np.int32)
    else:
        aop = np.where(x < s, 0, np.where(y < s, 1, 2)).astype(np.int32)
    X0, _, _ = g.distributed_init(aop, 5, H.lifting_matrix(3, 5), gpu=True, rtol=1e-12, dev_layout=True)
    X0.setflags(write=False)
    return g, aop, int(aop.max()) + 1, X0


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _run(hip, k, layout, schedule, events=None, **params):
    """events: {iteration: callable(engine, X0)} run before that iteration; the counters are read before and after the
    iteration that follows an event.  Returns the outputs and (final counters, counters around the events)."""
    g, aop, nag, X0 = _data(k, layout)
    e = hip.Rbcd(g, aop, np.zeros(nag, np.int32), 0, 1, hip.rbcd_params(r=5, **params))
    e.set_trace(1024)
    e.set_X(X0)
    status, around = [], []
    for it, c in enumerate(schedule(e.num_colors)):
        ev = (events or {}).get(it)
        if ev is not None:
            ev(e, X0)
            before = e.next_y_counters()
        e.pre_exchange(c)
        e.update(c, None)
        if ev is not None:
            around.append((before, e.next_y_counters()))
        if it % 4 == 3:
            rc, rd = e.status()
            status.append((rc.copy(), rd.copy()))
    rc, rd = e.status()
    status.append((rc.copy(), rd.copy()))
    X = np.zeros(X0.size)
    e.get_X_into(X)
    tr = [np.array([[rec[f] for f in hip.TRACE_FIELDS] for rec in e.get_trace(a)]) for a in range(nag)]
    return (X, e.stats().copy(), tr, status), (e.next_y_counters(), around), e.num_colors


def _ab(hip, k, layout, schedule, events=None, **params):
    saved = hip.get_tuning(NEXT_Y)
    out = []
    try:
        for v in (0, 1):
            hip.set_tuning(NEXT_Y, v)
            out.append(_run(hip, k, layout, schedule, events, **params))
    finally:
        hip.set_tuning(NEXT_Y, saved)
    (X, stats, tr, status), (cnt0, _), ncol = out[0]
    (X1, stats1, tr1, status1), (cnt1, around1), _ = out[1]
    assert sum(len(t) for t in tr) > 0
    assert np.array_equal(_bits(X), _bits(X1))
    assert np.array_equal(stats, stats1)
    for a, (t0, t1) in enumerate(zip(tr, tr1)):
        assert t0.shape == t1.shape and np.array_equal(_bits(t0), _bits(t1)), a
    assert len(status) == len(status1)
    for (rc, rd), (rc1, rd1) in zip(status, status1):
        assert np.array_equal(_bits(rc), _bits(rc1))  # the precomputed XPrev is the status reference
        assert np.array_equal(rd, rd1)
    assert cnt0 == (0, 0)  # value 0 never writes ahead
    print("colours", ncol, "skipped, mispredicted:", cnt1, "around events:", around1)
    return cnt1, around1, ncol


def _cyclic(iters):
    return lambda ncol: [it % ncol for it in range(iters)]


def _expected_cyclic_skips(iters, restart_interval):
    """Iterations (1-based I = 2 .. iters) whose selected pass is skipped under the cyclic schedule with the L2 cost:
    a record exists unless iteration I - 1 restarted or I restarts (an iteration restarts when (I + 1) % interval
    == 0, shouldRestart)."""
    rs = {i for i in range(1, iters + 1) if (i + 1) % restart_interval == 0}
    return sum(1 for i in range(2, iters + 1) if i not in rs and (i - 1) not in rs)


# k = 7: launches of fewer than 8 tiles, agents smaller than two tiles; 11: uneven agents, partial last tiles
@pytest.mark.parametrize("k", [7, 11])
def test_next_y_cyclic_l2_with_restarts(hip, k):
    cnt, _, ncol = _ab(hip, k, "cubes", _cyclic(40), acceleration=1, restart_interval=7)
    assert ncol == 2
    assert cnt == (_expected_cyclic_skips(40, 7), 0)  # every prediction made was used: none failed


def test_next_y_default_restart_interval(hip):
    cnt, _, _ = _ab(hip, 11, "cubes", _cyclic(40), acceleration=1)
    assert cnt == (_expected_cyclic_skips(40, 30), 0)


@pytest.mark.parametrize("k", [7, 11])
def test_next_y_gnc_tls_reweightings(hip, k):
    """Reweightings with initializeAcceleration (every 5 iterations) and restarts (every 7) fall between predictions
    and their use: no prediction is made across either."""
    cnt, _, _ = _ab(hip, k, "cubes", _cyclic(40), acceleration=1, restart_interval=7,
                    robust_cost=hip.ROBUST["GNC_TLS"], robust_opt_inner_iters=5)
    assert cnt[0] > 0 and cnt[1] == 0


def test_next_y_status_off(hip):
    cnt, _, _ = _ab(hip, 11, "cubes", _cyclic(24), acceleration=1, restart_interval=7, status=0)
    assert cnt[0] > 0


def test_next_y_no_acceleration(hip):
    cnt, _, _ = _ab(hip, 11, "cubes", _cyclic(24), acceleration=0)
    assert cnt == (0, 0)  # no Y without acceleration


def test_next_y_three_colours_mispredictions(hip):
    """Three colours.  The cyclic order first (predictions hold), then the caller breaks it: the same colour twice,
    colours out of order -- those records are dropped and the selected colour's own pass runs."""
    order = [0, 1, 2, 0, 1, 2, 2, 2, 0, 0, 1, 0, 2, 1, 1, 2, 0, 1, 2, 0, 1, 2, 1, 0, 2, 2, 0, 1]

    def schedule(ncol):
        assert ncol >= 3
        return order

    cnt, _, _ = _ab(hip, 7, "tri", schedule, acceleration=1, restart_interval=9)
    assert cnt[0] > 0 and cnt[1] > 0


def test_next_y_invalidated_by_set_x_and_set_selected(hip):
    """set_X and set_selected between a prediction and its use clear the record: the iteration that follows runs
    the selected colour's own pass and counts neither a skip nor a misprediction."""
    def set_x(e, X0):
        X = np.zeros(X0.size)
        e.get_X_into(X)
        e.set_X(X)

    def select_some(e, X0):
        mask = np.ones(e.num_agents, np.int32)
        mask[0] = 0
        e.set_selected(mask)

    def select_all(e, X0):
        e.set_selected(None)

    events = {9: set_x, 15: select_some, 21: select_all}
    for layout, k in (("cubes", 11), ("tri", 7)):
        cnt, around, _ = _ab(hip, k, layout, _cyclic(30), events, acceleration=1, restart_interval=50)
        assert cnt[0] > 0
        assert len(around) == 3
        for before, after in around:
            assert before == after
