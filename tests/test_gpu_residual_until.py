"""Residual-steady runs (lbm_run_until_residual / lbm_batch_run_until_residual): after every check_every steps one row of
the velocity residuals is taken and judged on the device.  Every result, every row of the history and every stop is the
one tests/residual_until_model.py gives on the CPU oracle's lattices, bit for bit (the sums are exact), and the call
leaves exactly the lattice of lbm_run(steps_run).  "resident": 64x16, resident kernel, one segment of look-ahead (dropped
after the stop); "per_pass": 100x16; ODD: 102x16, nx % 4 != 0, the one-cell gather."""
import ctypes
import math

import numpy as np
import pytest

import residual_model
import residual_until_model as rum
import steady_model as sm
from test_gpu_steady import VARIANTS, assert_state_is_oracle, check_path, oracle_after, setenv
from test_residual_abi import smallest

pytestmark = pytest.mark.gpu

_ROWS = {}


def model_rows(lbm, oracle, shape, omega=sm.OMEGA, accel=sm.ACCEL):
    """the model's rows of the first 8 checks of 512 steps from rest, computed once per case"""
    key = (shape, omega, accel)
    if key not in _ROWS:
        p, ob = rum.case(lbm, shape, omega, accel)
        _ROWS[key] = rum.oracle_rows(oracle, p, ob, oracle.init_cells(p), 8, 512)[1]
    return _ROWS[key]


def dbits(v):
    return np.float64(v).view(np.uint64)


def assert_result_is_model(got, want):
    for k in ("steps_run", "steady", "steady_step", "checks", "diverged"):
        print(k, got[k], want[k])
        assert got[k] == want[k], k
    print("last_rel", got["last_rel"], want["last_rel"])
    assert dbits(got["last_rel"]) == dbits(want["last_rel"])
    if want["last"] is None:
        assert got["last"].tolist() == (0.0, 0.0, 0, 0.0, -1, -1, 0)
    else:
        assert residual_model.same_bits(got["last"], want["last"]) == []


def assert_history_is_model(history, rows, n, every):
    steps, got = history
    assert steps.dtype == np.int32 and steps.tolist() == [(i + 1) * every for i in range(n)] and got.shape == (n,)
    for i in range(n):
        assert residual_model.same_bits(got[i], rows[i]) == [], i


@pytest.mark.parametrize("shape,env", VARIANTS + [(rum.ODD, {})])
def test_stops_where_the_model_says_and_goes_on(lbm, oracle, monkeypatch, shape, env):
    """the steady case: the result, every row, the state after it, run(k) after it, a second call with its own baseline"""
    setenv(monkeypatch, env)
    p, ob = rum.case(lbm, shape)
    rows = model_rows(lbm, oracle, shape)
    want = rum.run_until(rows, **rum.STEADY)
    with lbm.Engine(p, ob) as plain, lbm.Engine(p, ob) as eng:
        if isinstance(shape, str):
            check_path(eng, shape)
        got = eng.run_until_residual(**rum.STEADY)
        assert_result_is_model(got, want)
        assert (got["steps_run"], got["steady_step"], got["checks"], got["steady"], got["diverged"]) == (2048, 2048, 4, True, False)
        assert_history_is_model(got["history"], rows, 4, 512)
        steps = got["steps_run"]
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, steps), steps)
        plain.run(steps)
        assert np.array_equal(eng.av_vels().view(np.uint32), plain.av_vels().view(np.uint32))
        # going on: the dropped look-ahead segment left nothing behind
        eng.run(sm.GO_ON)
        steps += sm.GO_ON
        state = oracle_after(lbm, oracle, p, ob, steps)
        assert_state_is_oracle(eng, state, steps)
        # a second call takes a new baseline, the lattice after 2085 steps, and counts its own segments
        _, rows2 = rum.oracle_rows(oracle, p, ob, state[0], 4, 512)
        want2 = rum.run_until(rows2, 2048, 512, 1e-4, 2)
        assert want2["steady_step"] == 1024 and sm.margin(want2["rels"], 1e-4) >= rum.MARGIN
        got2 = eng.run_until_residual(2048, 512, 1e-4, 2)
        assert_result_is_model(got2, want2)
        assert_history_is_model(got2["history"], rows2, 2, 512)
        steps += 1024
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, steps), steps)
        eng.run(20)
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, steps + 20), steps + 20)


@pytest.mark.parametrize("capacity", [0, 1, 2])
def test_look_ahead_with_a_small_history(lbm, oracle, capacity):
    """the resident shape: the segment enqueued behind the stop clobbers no reported row, whatever the capacity"""
    p, ob = rum.case(lbm, "resident")
    rows = model_rows(lbm, oracle, "resident")
    with lbm.Engine(p, ob) as eng:
        check_path(eng, "resident")
        got = eng.run_until_residual(history=capacity, **rum.STEADY)
        assert_result_is_model(got, rum.run_until(rows, **rum.STEADY))
        assert_history_is_model(got["history"], rows, capacity, 512)
        # patience 1 and a tol everything meets: the stop at the first check, the second segment already enqueued
        got = eng.run_until_residual(4096, 512, 1e30, 1, history=capacity)
        assert (got["steady"], got["steps_run"], got["checks"]) == (True, 512, 1)
        assert got["history"][1].shape == (min(capacity, 1),)
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, 2560), 2560)


@pytest.mark.parametrize("shape,env", VARIANTS)
def test_not_steady_runs_to_the_cap(lbm, oracle, monkeypatch, shape, env):
    """a tol below the fp32 floor, max_steps not a multiple of check_every: two checks, the rest unchecked"""
    setenv(monkeypatch, env)
    p, ob = rum.case(lbm, shape)
    rows = model_rows(lbm, oracle, shape)
    with lbm.Engine(p, ob) as eng:
        got = eng.run_until_residual(**rum.NOT_STEADY)
        assert_result_is_model(got, rum.run_until(rows, **rum.NOT_STEADY))
        assert (got["steady"], got["diverged"], got["steps_run"], got["steady_step"], got["checks"]) == (False, False, 1300, -1, 2)
        assert_history_is_model(got["history"], rows, 2, 512)
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, 1300), 1300)


@pytest.mark.parametrize("shape,every,first", [("resident", 1, 0), ("resident", 512, 1), ("per_pass", 512, 1), (rum.ODD, 64, 1)])
def test_rows_are_the_recorders(lbm, shape, every, first):
    """the history against lbm_set_residual's rows on a second engine advanced by split run(every) calls.  The recorder
    samples after timestep tt (0-based) with tt % every == 0, the lattice after tt + 1 steps; its samples fall on the
    checks of a call that starts after `first` steps with first % every == 1 % every (every == 1: anywhere)."""
    p, ob = rum.case(lbm, shape)
    assert first % every == 1 % every
    with lbm.Engine(p, ob) as eng, lbm.Engine(p, ob) as rec:
        if first:
            eng.run(first)
            rec.run(first)
        got = eng.run_until_residual(3 * every, every, 0.0, 2)
        assert got["checks"] == 3 and not got["steady"]
        rec.set_residual(every, 8)
        for _ in range(3):
            rec.run(every)
        steps, rows = rec.residuals()
        assert steps.tolist() == [first + (i + 1) * every - 1 for i in range(3)]
        assert rows.tobytes() == got["history"][1].tobytes()
        assert np.array_equal(eng.cells().view(np.uint32), rec.cells().view(np.uint32))


def test_divergence_ends_the_call_at_the_first_check(lbm, oracle):
    p, ob, cells = smallest(lbm)
    bad = residual_model.poisoned(cells)
    _, rows = rum.oracle_rows(oracle, p, ob, bad, 1, 1)
    with lbm.Engine(p, ob, bad) as eng:
        got = eng.run_until_residual(3, 1, 1e-4, 2)
        assert_result_is_model(got, rum.run_until(rows, 3, 1, 1e-4, 2))
        assert got["diverged"] and not got["steady"] and got["steps_run"] == 1 and got["checks"] == 1 and got["steady_step"] == -1
        assert got["last"]["nonfinite"] == residual_model.POISON_COUNTS[0]
        assert_history_is_model(got["history"], rows, 1, 1)
        assert eng.info()["steps_done"] == 1


@pytest.mark.parametrize("shape", ["resident", "per_pass"])
def test_every_segment_length_keeps_the_lattice(lbm, oracle, shape):
    """short segments (also below resident_min_steps), one resident launch, and one beyond the resident chunk of 4096 steps;
    a stop at the very first check although a second segment was enqueued, and a run no check stops"""
    p, ob = rum.case(lbm, shape)
    for E in (1, 3, 64, 512, 4100):
        with lbm.Engine(p, ob) as eng:
            got = eng.run_until_residual(8192, E, 1e30, 1)
            assert (got["steady"], got["steps_run"], got["steady_step"], got["checks"]) == (True, E, E, 1), E
            assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, E), E)
            steps = E
            if E <= 64:
                N = 9 * E + E // 2                                      # nine checks, then a rest shorter than a segment
                got = eng.run_until_residual(N, E, 0.0, 2, history=3)
                assert (got["steady"], got["steps_run"], got["checks"], got["history"][1].size) == (False, N, 9, 3), E
                steps += N
                assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, steps), steps)
            go_on = E + 1 if E <= 512 else 37
            eng.run(go_on)
            steps += go_on
            assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, steps), steps)
            assert eng.av_vels().size == steps


@pytest.mark.parametrize("nx,ny", [(16, 8), (64, 16)])
def test_at_rest_is_steady_after_patience_checks(lbm, nx, ny):
    """accel 0 from the uniform equilibrium: r = 0, steady after P checks for any tol"""
    p = lbm.Params(nx, ny, 400, 10, 0.1, 0.0, 1.85)
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0, :3] = ob[3:5, 6:8] = 1
    with lbm.Engine(p, ob) as eng:
        for patience, tol in ((1, 0.0), (3, 0.0), (2, 1e-300)):
            got = eng.run_until_residual(60, 8, tol, patience)
            assert (got["steady"], got["steady_step"], got["steps_run"], got["checks"]) == (True, 8 * patience, 8 * patience, patience)
            assert got["last_rel"] == 0.0 and not math.copysign(1.0, got["last_rel"]) < 0
            assert got["last"]["sum_du_sq"] == 0.0 and got["last"]["sum_u_sq"] == 0.0 and got["last"]["span"] == 8
            assert (got["last"]["max_x"], got["last"]["max_y"]) == (3, 0)


def assert_batch_is_model(batch, got, member_rows, steps, want, every):
    assert batch.info()["steps_done"] == steps
    for g, w in zip(got, want):
        assert_result_is_model(g, w)
    h_steps, h_rows = got.history
    n = steps // every
    assert h_steps.tolist() == [(i + 1) * every for i in range(n)] and h_rows.shape == (n, len(got))
    for j in range(n):
        for i in range(len(got)):
            assert residual_model.same_bits(h_rows[j, i], member_rows[i][j]) == [], (j, i)


def test_batch_members_stop_at_their_own_checks(lbm, oracle):
    """eight 64x16 members with different omega / accel: the batch stops with its last member"""
    made = [rum.case(lbm, "resident", omega, accel) for omega, accel in sm.BATCH]
    params, obstacles = [m[0] for m in made], [m[1] for m in made]
    member_rows = [model_rows(lbm, oracle, "resident", omega, accel) for omega, accel in sm.BATCH]
    steps, want = rum.batch_run_until(member_rows, **rum.STEADY)
    with lbm.Batch(params, obstacles) as batch:
        assert batch.info()["resident_steps"] > 0
        got = batch.run_until_residual(**rum.STEADY)
        assert steps == 2560 and tuple(g["steady_step"] for g in got) == rum.BATCH_STEADY_STEPS
        assert_batch_is_model(batch, got, member_rows, steps, want, 512)       # (a frozen member's later rows are real rows)
        for i in range(len(params)):
            with lbm.Engine(params[i], obstacles[i]) as single:
                single.run(steps)
                m = batch.member(i)
                assert np.array_equal(m.cells().view(np.uint32), single.cells().view(np.uint32))
                assert np.array_equal(m.av_vels().view(np.uint32), single.av_vels().view(np.uint32))
        for i in (0, 5):
            assert_state_is_oracle(batch.member(i), oracle_after(lbm, oracle, params[i], obstacles[i], steps), steps)
        # not steady within the cap: all members run to it; a history of one row
        got = batch.run_until_residual(1300, 512, 1e-9, 2, history=1)
        assert all(not g["steady"] and not g["diverged"] and g["steps_run"] == 1300 and g["checks"] == 2 for g in got)
        assert got.history[0].tolist() == [512] and got.history[1].shape == (1, 8)
        assert batch.info()["steps_done"] == steps + 1300


def test_batch_on_the_per_pass_kernels(lbm, oracle):
    made = [rum.case(lbm, "per_pass", omega, 0.005) for omega in (1.0, 0.8)]
    params, obstacles = [m[0] for m in made], [m[1] for m in made]
    member_rows = [rum.oracle_rows(oracle, p, ob, oracle.init_cells(p), 3, 100)[1] for p, ob in made]
    steps, want = rum.batch_run_until(member_rows, 1000, 100, 1e30, 2)
    with lbm.Batch(params, obstacles) as batch:
        assert batch.info()["resident_steps"] == 0
        got = batch.run_until_residual(1000, 100, 1e30, 2)
        assert steps == 200 and all(g["steady"] and g["steady_step"] == 200 for g in got)
        assert_batch_is_model(batch, got, member_rows, steps, want, 100)
        for i in range(2):
            assert_state_is_oracle(batch.member(i), oracle_after(lbm, oracle, params[i], obstacles[i], 200), 200)


def test_batch_with_a_poisoned_member_still_ends(lbm, oracle):
    """member 1 diverges at the first check, the others are steady at the second: the batch ends there, and member 1's
    second row is a real row"""
    p, ob, cells = smallest(lbm)
    starts = [cells, residual_model.poisoned(cells), cells * np.float32(1.0)]
    member_rows = [rum.oracle_rows(oracle, p, ob, c, 2, 1)[1] for c in starts]
    steps, want = rum.batch_run_until(member_rows, 6, 1, 1e30, 2)
    assert steps == 2 and [w["diverged"] for w in want] == [False, True, False] and [w["checks"] for w in want] == [2, 1, 2]
    with lbm.Batch([p] * 3, [ob] * 3, starts) as batch:
        got = batch.run_until_residual(6, 1, 1e30, 2)
        assert [(g["steady"], g["diverged"], g["steady_step"]) for g in got] == [(True, False, 2), (False, True, -1), (True, False, 2)]
        assert_batch_is_model(batch, got, member_rows, steps, want, 1)
        assert got[1]["last"]["nonfinite"] == residual_model.POISON_COUNTS[0]
        assert got.history[1][1, 1]["nonfinite"] == residual_model.POISON_COUNTS[1]


# ---- refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["resident", "per_pass"])
def test_refusals_leave_the_context_usable(lbm, oracle, shape):
    p, ob = rum.case(lbm, shape)
    lib = lbm.load_library()
    res = lbm._CResidualSteadyResult()
    rows = np.zeros(4, dtype=lbm.RESIDUAL_DTYPE)

    def c_call(eng, max_steps, check_every, tol, patience, capacity=4):
        rc = lib.lbm_run_until_residual(eng.handle, max_steps, check_every, ctypes.c_double(tol), patience, ctypes.byref(res),
                                        rows.ctypes.data, capacity)
        return rc, lib.lbm_last_error().decode()

    with lbm.Engine(p, ob) as eng:
        eng.run(10)
        for args, match in (((p.max_iters, 16, 1e-3, 2), "the av_vels record holds"), ((100, 0, 1e-3, 2), "check_every"),
                            ((100, 16, 1e-3, 0), "patience"), ((100, 16, -1.0, 2), "tol"), ((100, 16, float("nan"), 2), "tol"),
                            ((-1, 16, 1e-3, 2), "negative step count"), ((100, 16, 1e-3, 2, -1), "negative history capacity -1")):
            rc, err = c_call(eng, *args)
            assert rc != 0 and "lbm_run_until_residual: " in err and match in err, (args, err)
            assert eng.info()["steps_done"] == 10
        with pytest.raises(lbm.LbmError, match="the av_vels record holds"):
            eng.run_until_residual(p.max_iters, 16)
        # every recorder kind, the residual recorder included
        for arm, disarm, name in ((lambda: eng.set_frames(10, 2), lambda: eng.set_frames(0), "animation frames"),
                                  (lambda: eng.set_probes([(1, 1)], 1, 4), lambda: eng.set_probes([], 0), "point probes"),
                                  (lambda: eng.set_mean(10), lambda: eng.set_mean(0), "mean fields"),
                                  (lambda: eng.set_field_frames(10, 2), lambda: eng.set_field_frames(0), "field frames"),
                                  (lambda: eng.set_forces(10, 4), lambda: eng.set_forces(0), "obstacle forces"),
                                  (lambda: eng.set_stats(10, 4), lambda: eng.set_stats(0), "lattice statistics"),
                                  (lambda: eng.set_residual(10, 4), lambda: eng.set_residual(0), "velocity residuals")):
            arm()
            with pytest.raises(lbm.LbmError, match="lbm_run_until_residual: %s are armed" % name):
                eng.run_until_residual(100, 16)
            disarm()
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_run_until_residual: only LBM_HALO_SYNC"):
                eng.run_until_residual(100, 16)
        eng.set_halo_mode("sync")
        assert eng.info()["steps_done"] == 10
        got = eng.run_until_residual(64, 16, 1e30, 1)
        assert got["steps_run"] == 16 and got["steady"]
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, 26), 26)


def test_refusals_of_slabs_ranks_and_members(lbm):
    p, ob = rum.case(lbm, "resident")
    with lbm.Engine(p, ob, n_gpus=2) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_run_until_residual: the context has 2 slabs"):
            eng.run_until_residual(100, 16)
        assert eng.info()["steps_done"] == 0
        eng.run(5)
    comm = (lambda plan, views: None, lambda values: None)
    with lbm.Engine(p, ob, rank=0, world_size=1, host_comm=comm) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_run_until_residual: not available in a multi-process"):
            eng.run_until_residual(100, 16)
        assert eng.info()["steps_done"] == 0
    with lbm.Batch([p, p], [ob, ob]) as batch:
        lib = lbm.load_library()
        res = lbm._CResidualSteadyResult()
        assert lib.lbm_run_until_residual(batch.member(1).handle, 100, 16, ctypes.c_double(1e-3), 2, ctypes.byref(res), None, 0) != 0
        assert "lbm_run_until_residual: this context is a member of a batch" in lib.lbm_last_error().decode()
        with pytest.raises(lbm.LbmError, match="member of a batch"):
            batch.member(1).run_until_residual(100, 16)
        batch.member(0).set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run_until_residual: animation frames are armed"):
            batch.run_until_residual(100, 16)
        batch.member(0).set_frames(0, 0)
        batch.set_stats(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_run_until_residual: lattice statistics are armed \(lbm_batch_set_stats\)"):
            batch.run_until_residual(100, 16)
        batch.set_stats(0)
        with pytest.raises(lbm.LbmError, match="the av_vels record holds"):
            batch.run_until_residual(p.max_iters + 1, 16)
        res8 = (lbm._CResidualSteadyResult * 2)()
        steps = ctypes.c_int()
        rows = np.zeros((4, 2), dtype=lbm.RESIDUAL_DTYPE)
        assert lib.lbm_batch_run_until_residual(batch._live(), 100, 16, ctypes.c_double(1e-3), 2, res8, ctypes.byref(steps),
                                                rows.ctypes.data, -3) != 0
        assert "lbm_batch_run_until_residual: negative history capacity -3" in lib.lbm_last_error().decode()
        assert batch.info()["steps_done"] == 0
        got = batch.run_until_residual(64, 16, 1e30, 1)
        assert got[1]["steps_run"] == 16 and all(g["steady"] for g in got) and got.history[1].shape == (1, 2)
