"""CPU checks of the steady-state criterion's numpy model (tests/steady_model.py) and of the cases the GPU tests use:
on the oracle's series every relative change up to the stop is a factor >= 3 away from tol."""
import math

import numpy as np
import pytest

import steady_model as sm


def lanes_mean(av):
    """segment_mean spelled out lane by lane (independent of the vectorised form)."""
    acc = [0.0] * 64
    for i, v in enumerate(np.asarray(av, dtype=np.float32)):
        acc[i % 64] += float(v)
    off = 32
    while off:
        for i in range(off):
            acc[i] += acc[i + off]
        off //= 2
    return acc[0] / float(len(av))


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 512, 1000, 1024])
def test_segment_mean_follows_the_lane_order(n):
    rng = np.random.default_rng(n)
    av = (rng.random(n) * rng.choice([1e-3, 1.0, 1e3], n)).astype(np.float32)
    assert sm.segment_mean(av) == lanes_mean(av)
    assert abs(sm.segment_mean(av) - float(np.mean(av.astype(np.float64)))) <= 1e-12 * float(np.abs(av).max())


def test_segment_mean_order_matters():
    """The order is part of the specification: series that span many binades give another double when summed front to
    back (floats of one magnitude sum exactly in double, whatever the order)."""
    rng = np.random.default_rng(7)
    differs = 0
    for _ in range(50):
        av = (rng.random(512) * 10.0 ** rng.integers(-12, 12, 512)).astype(np.float32)
        plain = 0.0
        for v in av:
            plain += float(v)
        differs += (plain / 512.0) != sm.segment_mean(av)
    assert differs > 0


def series_from_means(means, E):
    return np.repeat(np.asarray(means, dtype=np.float32), E)


def test_patience_and_streak():
    E = 64
    av = series_from_means([1.0, 2.0, 2.0, 3.0, 3.0, 3.0, 3.0], E)
    r = sm.run_until(av, 7 * E, E, 1e-6, 2)
    assert r["steady"] and r["steady_step"] == 6 * E and r["steps_run"] == 6 * E and r["checks"] == 5
    assert r["rels"][:4] == [0.5, 0.0, 1.0 / 3.0, 0.0] and r["last_rel"] == 0.0 and r["last_mean"] == 3.0
    r = sm.run_until(av, 7 * E, E, 1e-6, 1)
    assert r["steady_step"] == 3 * E and r["checks"] == 2
    r = sm.run_until(av, 7 * E, E, 1e-6, 4)            # never four in a row
    assert not r["steady"] and r["steady_step"] == -1 and r["steps_run"] == 7 * E and r["checks"] == 6


def test_first_segment_is_not_checked_and_the_rest_of_the_cap_is_run():
    E = 32
    av = series_from_means([5.0] * 10, E)
    r = sm.run_until(av, E, E, 1.0, 1)
    assert not r["steady"] and r["checks"] == 0 and math.isinf(r["last_rel"]) and r["steps_run"] == E
    r = sm.run_until(av, 2 * E, E, 0.0, 1)             # tol = 0: met by an exactly equal mean
    assert r["steady"] and r["steady_step"] == 2 * E
    r = sm.run_until(av, 2 * E + 7, E, 0.0, 2)
    assert not r["steady"] and r["steps_run"] == 2 * E + 7 and r["checks"] == 1
    r = sm.run_until(av, 0, E, 0.0, 1)
    assert r["steps_run"] == 0 and r["checks"] == 0


def test_zero_means():
    assert sm.rel_change(0.0, 0.0) == 0.0
    assert math.isinf(sm.rel_change(0.0, 1.0))
    assert sm.rel_change(-2.0, -1.0) == 0.5
    E = 16
    r = sm.run_until(series_from_means([0.0, 0.0, 0.0], E), 3 * E, E, 0.0, 2)
    assert r["steady"] and r["steady_step"] == 3 * E
    r = sm.run_until(series_from_means([1.0, 0.0, 0.0], E), 3 * E, E, 1e9, 2)
    assert not r["steady"] and math.isinf(r["rels"][0])


def test_batch_stops_with_its_last_member():
    E = 16
    a = series_from_means([1.0, 1.0, 1.0, 1.0, 1.0, 1.0], E)
    b = series_from_means([1.0, 2.0, 3.0, 3.0, 3.0, 3.0], E)
    steps, members = sm.batch_run_until([a, b], 6 * E, E, 1e-6, 2)
    assert steps == 5 * E and [m["steady_step"] for m in members] == [3 * E, 5 * E]
    assert members[0]["checks"] == 2 and all(m["steps_run"] == steps for m in members)
    steps, members = sm.batch_run_until([a, b], 4 * E, E, 1e-6, 2)
    assert steps == 4 * E and [m["steady"] for m in members] == [True, False]


def test_margin():
    assert sm.margin([1e-1, 1e-5], 1e-3) == pytest.approx(100.0)
    assert sm.margin([4e-3], 1e-3) == pytest.approx(4.0)
    assert sm.margin([], 1e-3) == math.inf and sm.margin([1e-3], 1e-3) == 1.0


def oracle_series(lbm, oracle, shape, n, omega=sm.OMEGA, accel=sm.ACCEL):
    p, ob = sm.case_params(lbm, shape, omega, accel)
    return oracle.run(p, oracle.init_cells(p), ob, n)


@pytest.mark.parametrize("shape", sorted(sm.SHAPES))
def test_gpu_cases_decide_with_a_margin(lbm, oracle, shape):
    """The condition on every (shape, E, tol) a GPU test uses."""
    av = oracle_series(lbm, oracle, shape, sm.CAPACITY)
    r = sm.run_until(av, **sm.STEADY)
    assert r["steady"] and r["steps_run"] == r["steady_step"] == 2048, r
    assert sm.margin(r["rels"], sm.STEADY["tol"]) >= sm.MARGIN, r["rels"]
    n = sm.run_until(av, **sm.NOT_STEADY)
    assert not n["steady"] and n["steps_run"] == 1300 and n["checks"] == 1
    assert sm.margin(n["rels"], sm.NOT_STEADY["tol"]) >= sm.MARGIN, n["rels"]
    second = sm.run_until(av[r["steps_run"] + sm.GO_ON:], **sm.SECOND)
    assert second["steady"] and second["steady_step"] == 1536, second
    assert sm.margin(second["rels"], sm.SECOND["tol"]) >= sm.MARGIN, second["rels"]


def test_gpu_batch_members_decide_with_a_margin(lbm, oracle):
    series = [oracle_series(lbm, oracle, "resident", sm.BATCH_STEADY["max_steps"], omega, accel) for omega, accel in sm.BATCH]
    steps, members = sm.batch_run_until(series, **sm.BATCH_STEADY)
    assert steps == 2560
    assert sorted(set(m["steady_step"] for m in members)) == [2048, 2560]      # they converge at different checks
    for m in members:
        assert sm.margin(m["rels"], sm.BATCH_STEADY["tol"]) >= sm.MARGIN, m["rels"]
