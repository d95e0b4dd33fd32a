"""The two kinds of checked run on one handle: run_until and run_until_residual share the stop word, its pinned copy,
the events and the segment driver (on a batch: the finished-count, the stop word and the event), so calls of both kinds
are made in turn on one engine and on one batch.  Every call stops at its first possible check (tol 1e30, patience 1):
after 2 E steps on the average velocity, whose first segment is no check, and after E steps on the residual; on the
resident shape each such stop leaves an enqueued look-ahead segment to drop.  After every call the lattice is the
oracle's after the steps run so far, and the result is that of a fresh engine that reached the same step by run() and
then made only that call.  "resident": 64x16; "per_pass": 100x16 (tests/steady_model.py)."""

import numpy as np
import pytest

import steady_model as sm
from test_gpu_parity import AV_RTOL
from test_gpu_residual_until import dbits
from test_gpu_steady import assert_state_is_oracle, check_path, oracle_after

pytestmark = pytest.mark.gpu

E, TOL, PATIENCE, MAX_STEPS = 512, 1e30, 1, 4 * 512
CALLS = ("average", "residual", "average", "residual")
STEPS = {"average": 2 * E, "residual": E}
assert sum(STEPS[kind] for kind in CALLS) - E + MAX_STEPS <= sm.CAPACITY

_ORACLE = {}


def oracle_at(lbm, oracle, p, ob, key, steps):
    """the oracle's state after `steps` steps, computed once per case"""
    if (key, steps) not in _ORACLE:
        _ORACLE[key, steps] = oracle_after(lbm, oracle, p, ob, steps)
    return _ORACLE[key, steps]


def checked(target, kind):
    """one checked run of an Engine or a Batch"""
    if kind == "average":
        return target.run_until(MAX_STEPS, E, TOL, PATIENCE)
    return target.run_until_residual(MAX_STEPS, E, TOL, PATIENCE, history=1)


def assert_same_result(kind, got, want, float_bits):
    """residual: every field bit for bit, and the history; average velocity: the decision, and last_rel / last_mean bit
    for bit where the sums do not depend on where a call's passes begin (float_bits)"""
    if kind == "average":
        for k in ("steps_run", "steady", "steady_step", "checks"):
            print(k, got[k], want[k])
            assert got[k] == want[k], k
        for k in ("last_rel", "last_mean"):
            print(k, got[k], want[k])
            if float_bits:
                assert dbits(got[k]) == dbits(want[k]), k
        return
    for k in ("steps_run", "steady", "steady_step", "checks", "diverged"):
        print(k, got[k], want[k])
        assert got[k] == want[k], k
    print("last_rel", got["last_rel"], want["last_rel"], got["last"], want["last"])
    assert dbits(got["last_rel"]) == dbits(want["last_rel"])
    assert got["last"].tobytes() == want["last"].tobytes()


def assert_same_history(got, want, shape):
    assert got[0].dtype == want[0].dtype and got[0].tolist() == want[0].tolist() == [E]
    assert got[1].shape == want[1].shape == shape and got[1].tobytes() == want[1].tobytes()


def assert_stopped_at_the_first_check(kind, result):
    assert (result["steady"], result["steps_run"], result["steady_step"], result["checks"]) == (True, STEPS[kind], STEPS[kind], 1)


@pytest.mark.parametrize("shape", ["resident", "per_pass"])
def test_calls_of_both_kinds_in_turn_on_one_engine(lbm, oracle, shape):
    p, ob = sm.case_params(lbm, shape)
    with lbm.Engine(p, ob) as eng:
        check_path(eng, shape)
        steps = 0
        for kind in CALLS:
            got = checked(eng, kind)
            with lbm.Engine(p, ob) as fresh:
                fresh.run(steps)
                want = checked(fresh, kind)
            assert_stopped_at_the_first_check(kind, got)
            assert_same_result(kind, got, want, float_bits=shape == "resident")
            if kind == "residual":
                assert_same_history(got["history"], want["history"], (1,))
            steps += got["steps_run"]
            assert_state_is_oracle(eng, oracle_at(lbm, oracle, p, ob, shape, steps), steps)
        assert steps == sum(STEPS[kind] for kind in CALLS)


@pytest.mark.parametrize("shape,members", [("resident", sm.BATCH[:3]), ("per_pass", [(1.0, 0.005), (0.8, 0.005)])])
def test_calls_of_both_kinds_in_turn_on_one_batch(lbm, oracle, shape, members):
    made = [sm.case_params(lbm, shape, omega, accel) for omega, accel in members]
    params, obstacles = [m[0] for m in made], [m[1] for m in made]
    singles = [lbm.Engine(p, ob) for p, ob in made]
    try:
        with lbm.Batch(params, obstacles) as batch:
            assert (batch.info()["resident_steps"] > 0) == (shape == "resident")
            steps = 0
            for kind in CALLS:
                got = checked(batch, kind)
                with lbm.Batch(params, obstacles) as fresh:
                    fresh.run(steps)
                    want = checked(fresh, kind)
                for g, w in zip(got, want):
                    assert_stopped_at_the_first_check(kind, g)
                    assert_same_result(kind, g, w, float_bits=shape == "resident")
                if kind == "residual":
                    assert_same_history(got.history, want.history, (1, len(members)))
                steps += got[0]["steps_run"]
                assert batch.info()["steps_done"] == steps
                for i, single in enumerate(singles):
                    single.run(got[0]["steps_run"])
                    m = batch.member(i)
                    assert m.info()["steps_done"] == steps
                    assert np.array_equal(m.cells().view(np.uint32), single.cells().view(np.uint32)), i
                    av, single_av = m.av_vels(), single.av_vels()
                    assert av.size == single_av.size == steps
                    if shape == "resident":     # per-band sums: the same whatever the calls
                        assert np.array_equal(av.view(np.uint32), single_av.view(np.uint32)), i
                    else:
                        np.testing.assert_allclose(av, single_av, rtol=AV_RTOL)
            # the single engines are themselves the oracle's
            for (p, ob), (omega, accel), single in zip(made, members, singles):
                assert_state_is_oracle(single, oracle_at(lbm, oracle, p, ob, (shape, omega, accel), steps), steps)
    finally:
        for single in singles:
            single.close()


@pytest.mark.parametrize("shape", ["resident", "per_pass"])
def test_a_refusal_between_calls_leaves_nothing_behind(lbm, oracle, shape):
    p, ob = sm.case_params(lbm, shape)
    with lbm.Engine(p, ob) as eng, lbm.Engine(p, ob) as untouched:
        eng.set_stats(64, 8)
        with pytest.raises(lbm.LbmError, match="run_until_residual: .* are armed"):
            checked(eng, "residual")
        eng.set_stats(0, 0)
        assert eng.info()["steps_done"] == 0
        got, want = checked(eng, "average"), checked(untouched, "average")
        assert_stopped_at_the_first_check("average", got)
        assert_same_result("average", got, want, float_bits=True)   # the same calls on both: the same sums
        assert np.array_equal(eng.cells().view(np.uint32), untouched.cells().view(np.uint32))
        assert np.array_equal(eng.av_vels().view(np.uint32), untouched.av_vels().view(np.uint32))
        assert_state_is_oracle(eng, oracle_at(lbm, oracle, p, ob, shape, 2 * E), 2 * E)
