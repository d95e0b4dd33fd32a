"""A resident give-up fails its owner for good (the rule at lbm_sync in include/lbm_hip.h).  A launch of lbm::resident_band
whose workgroups are not all running gives up after its bound and leaves a status word; the call that first sees the word
reports it, and from then on every call of tests/give_up_calls.py's ledger on that context -- or, for a batch, on the
batch and on every member -- is refused in the ledger's words, issues nothing and changes nothing, until the owner is
destroyed.  Before this suite only the first sync() was looked at, and the second call of any reader handed back the broken
lattice as a success.

The give-up is an ordinary kernel return, produced by the knob the resident suites use (LBM_RESIDENT_ABSENT_BAND: one
band's workgroup returns at once, its neighbours wait out LBM_RESIDENT_TIMEOUT_MS = 200 ms); every owner is made to give up
exactly once, the knob is set only around that one call and is read at each launch.  Lattice: 128 x 16 with random
obstacles, eight bands of two rows; a healthy prefix and a healthy successor on the same inputs equal the oracle bit for
bit, so the flag is not set by mistake."""
import ctypes
import os
import time

import numpy as np
import pytest

import give_up_calls as ledger
from cli_case import obstacles_text, params_text, run_cli
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu

NX, NY = 128, 16
ABSENT_BAND = 5                                               # of eight
SENTINEL = -7.0


@pytest.fixture(autouse=True)
def bound(monkeypatch):
    """read when an owner is created"""
    monkeypatch.setenv("LBM_RESIDENT_TIMEOUT_MS", "200")
    monkeypatch.delenv("LBM_RESIDENT_ABSENT_BAND", raising=False)


@pytest.fixture(scope="module")
def case(lbm, oracle):
    """(p, ob, [the lattices of nine members], {steps: the oracle's lattice of member 0 after so many})"""
    p, ob, _ = random_case(lbm, NX, NY, 2024, walls=False)
    cells = [random_case(lbm, NX, NY, 2024 + i, walls=False)[2] for i in range(9)]
    ref, want = cells[0].copy(), {}
    oracle.run(p, ref, ob, 10)
    want[10] = ref.copy()
    oracle.run(p, ref, ob, 20)
    want[30] = ref.copy()
    for w in want.values():
        w.setflags(write=False)
    return p, ob, cells, want


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def resident_serves(info, n_steps, bands=NY // 2, absent=ABSENT_BAND):
    """the resident kernel will run a call of n_steps, and the absent band is one of its bands"""
    assert info["resident_steps"] > 0 and 0 < info["resident_min_steps"] <= n_steps, info
    assert info["row_count"] // info["resident_rows"] == bands > absent, info


def one_give_up(monkeypatch, call, band=ABSENT_BAND):
    """`call` with one band absent from every launch it issues: the one give-up of its owner"""
    monkeypatch.setenv("LBM_RESIDENT_ABSENT_BAND", str(band))
    try:
        return call()
    finally:
        monkeypatch.delenv("LBM_RESIDENT_ABSENT_BAND")


def fail_engine(lbm, monkeypatch, eng, n_steps=20):
    """run(n_steps) gives up; the sync that sees it reports it in the words of old"""
    resident_serves(eng.info(), n_steps)
    one_give_up(monkeypatch, lambda: eng.run(n_steps))
    with pytest.raises(lbm.LbmError, match=ledger.FIRST_REPORT):
        eng.sync()


def refused(lbm, name, call, o, times=2):
    """the second call is the regression: a reader's first sync used to clear what the next one needed"""
    for _ in range(times):
        with pytest.raises(lbm.LbmError) as e:
            call(o)
        assert str(e.value) == ledger.refusal(name), name


def all_refused(lbm, calls, o):
    for name, call in ledger.refused(calls):
        refused(lbm, name, call, o)
    for name in ledger.ring_readers(calls):
        assert ledger.ring_read(o, name) == (1, 0, SENTINEL, int(SENTINEL)), name
        assert o.lib.lbm_last_error().decode() == ledger.refusal(name)


# ---- 1: a healthy prefix, the failure, then every entry point -----------------------------------------------------------
def test_a_failed_context_refuses_every_call(lbm, oracle, monkeypatch, case):
    p, ob, cells, want = case
    eng = lbm.Engine(p, ob, cells[0])
    eng.run(10)
    assert same_bits(eng.cells(), want[10])
    fail_engine(lbm, monkeypatch, eng)
    info = eng.info()
    assert info["steps_done"] == 30                           # the call that gave up was issued as a call of 20 steps
    all_refused(lbm, ledger.CTX_CALLS, eng)
    with pytest.raises(lbm.LbmError) as e:                    # (the ledger's lbm_run is of per-pass length: 3 steps)
        eng.run(20)
    assert str(e.value) == ledger.refusal("lbm_run")
    # the caller's arrays stay as they were, the count outputs are 0
    lib, h = eng.lib, eng.handle
    out = [np.full((NY, NX, 9), SENTINEL, dtype=np.float32), np.full(30, SENTINEL, dtype=np.float32)]
    out += [np.full((NY, NX), SENTINEL, dtype=np.float32) for _ in range(4)]
    assert lib.lbm_read_cells(h, out[0].ctypes.data) == 1 and lib.lbm_last_error().decode() == ledger.refusal("lbm_read_cells")
    assert lib.lbm_read_av_vels(h, out[1].ctypes.data, 30) == 1 and lib.lbm_last_error().decode() == ledger.refusal("lbm_read_av_vels")
    assert lib.lbm_read_final_state(h, *(a.ctypes.data for a in out[2:])) == 1
    assert lib.lbm_last_error().decode() == ledger.refusal("lbm_read_final_state")
    assert all((a == np.float32(SENTINEL)).all() for a in out)
    ms, n = ctypes.c_float(SENTINEL), ctypes.c_longlong(-7)
    assert lib.lbm_run_timed(h, 20, ctypes.byref(ms)) == 1 and ms.value == 0.0
    assert lib.lbm_read_mean(h, None, None, None, None, ctypes.byref(n)) == 1 and n.value == 0
    assert lib.lbm_last_error().decode() == ledger.refusal("lbm_read_mean")        # not "the mean fields are not armed"
    # what still works, and nothing of all that moved the context
    assert eng.info() == info and eng.rccl_info()["n_comms"] == 0
    eng.close()
    # nothing outlives the owner: the same inputs, the knob gone
    with lbm.Engine(p, ob, cells[0]) as eng:
        eng.run(10)
        eng.run(20)
        assert same_bits(eng.cells(), want[30])
        assert eng.info()["steps_done"] == 30


# ---- 2: whoever notices first reports it, and the next call is refused -----------------------------------------------------
@pytest.mark.parametrize("first", ["cells", "av_vels", "final_state", "total_density", "run"])
def test_who_notices_first(lbm, monkeypatch, case, first):
    p, ob, cells, _ = case
    with lbm.Engine(p, ob, cells[0]) as eng:
        resident_serves(eng.info(), 20)
        one_give_up(monkeypatch, lambda: eng.run(20))
        with pytest.raises(lbm.LbmError, match=ledger.FIRST_REPORT):
            if first == "run":
                # lbm_run waits for nothing, so a second resident call cannot see the word: its launches end at once (they
                # poll it), and the sync behind them reports
                eng.run(20)
                eng.sync()
            else:
                getattr(eng, first)()
        refused(lbm, "lbm_read_cells", lambda o: o.cells(), eng)
        refused(lbm, "lbm_" + {"cells": "read_cells", "av_vels": "read_av_vels", "final_state": "read_final_state",
                               "total_density": "total_density", "run": "run"}[first],
                (lambda o: o.run(20)) if first == "run" else (lambda o: getattr(o, first)()), eng)


# ---- 3: the timed path looks at the status ------------------------------------------------------------------------------
def test_run_timed_fails_on_the_call_that_gave_up(lbm, monkeypatch, case):
    p, ob, cells, want = case
    with lbm.Engine(p, ob, cells[0]) as eng:
        resident_serves(eng.info(), 20)
        assert eng.run_timed(10) > 0.0 and same_bits(eng.cells(), want[10])       # a healthy timed call has its time
        with pytest.raises(lbm.LbmError, match=ledger.FIRST_REPORT):
            one_give_up(monkeypatch, lambda: eng.run_timed(20))
        refused(lbm, "lbm_read_cells", lambda o: o.cells(), eng)
        refused(lbm, "lbm_run_timed", lambda o: o.run_timed(20), eng)


# ---- 4: armed owners ------------------------------------------------------------------------------------------------------
DISARM = {"lbm_set_frames": lambda o: o.set_frames(0), "lbm_set_probes": lambda o: o.set_probes([], 0), "lbm_set_mean": lambda o: o.set_mean(0),
          "lbm_set_mean_order": lambda o: o.set_mean_order(0, 2), "lbm_set_field_frames": lambda o: o.set_field_frames(0),
          "lbm_set_forces": lambda o: o.set_forces(0), "lbm_set_stats": lambda o: o.set_stats(0), "lbm_set_residual": lambda o: o.set_residual(0),
          "lbm_set_profiles": lambda o: o.set_profiles(0), "lbm_set_coarse_frames": lambda o: o.set_coarse_frames(0),
          "lbm_set_enstrophy": lambda o: o.set_enstrophy(0), "lbm_set_stress": lambda o: o.set_stress(0), "lbm_set_psi": lambda o: o.set_psi(0),
          "lbm_set_tracers": lambda o: o.set_tracers(np.zeros((0, 2)), 0)}


@pytest.mark.parametrize("armed", ["field_frames", "stats"])
def test_an_armed_owner_hands_out_no_records(lbm, monkeypatch, case, armed):
    """field frames are recorded by the resident kernel itself (every step); statistics by a gather behind sub-calls of two
    steps, each a resident launch of its own here"""
    p, ob, cells, _ = case
    if armed == "stats":
        monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "1")
    with lbm.Engine(p, ob, cells[0]) as eng:
        if armed == "field_frames":
            eng.set_field_frames(1, 64)
            reader, name, sub_call = eng.field_frames, "lbm_read_field_frames", 20
        else:
            eng.set_stats(2, 64)
            reader, name, sub_call = eng.stats, "lbm_read_stats", 2
        eng.run(10)
        assert len(reader()[0]) == (10 if armed == "field_frames" else 5)         # healthy: the records of the prefix
        resident_serves(eng.info(), sub_call)
        one_give_up(monkeypatch, lambda: eng.run(20))
        with pytest.raises(lbm.LbmError, match=ledger.FIRST_REPORT):
            reader()                                          # the reader is the first to synchronise
        refused(lbm, name, lambda o: reader(), eng)
        assert ledger.ring_read(eng, name) == (1, 0, SENTINEL, int(SENTINEL))      # 20 (10) records were due: none is handed out
        setters = [(n, c) for n, c in ledger.refused(ledger.CTX_CALLS) if n.startswith("lbm_set_") and n != "lbm_set_halo_mode"]
        assert sorted(n for n, _ in setters) == sorted(DISARM)
        for n, arm in setters:                                # arming any kind, and disarming it
            refused(lbm, n, arm, eng, times=1)
            refused(lbm, n, DISARM[n], eng, times=1)
        assert eng.info()["steps_done"] == 30


# ---- 5: one call of three launches ----------------------------------------------------------------------------------------
def test_a_call_of_three_launches_gives_up_once(lbm, monkeypatch):
    """9 000 steps are launches of 4096, 4096 and 808: the first gives up after the bound, the two behind it see the status
    word at their first wait and end at once"""
    p, ob, cells = random_case(lbm, 64, 8, 77, blocked_frac=0.05, walls=False)
    p.max_iters = 9000
    with lbm.Engine(p, ob, cells) as eng:
        info = eng.info()
        resident_serves(info, 9000, bands=8 // info["resident_rows"], absent=1)
        assert 2 * info["resident_steps"] < 9000 <= 3 * info["resident_steps"]
        t0 = time.time()
        one_give_up(monkeypatch, lambda: eng.run(9000), band=1)
        with pytest.raises(lbm.LbmError, match=ledger.FIRST_REPORT):
            eng.sync()
        assert time.time() - t0 < 20                          # (the bound test_resident_gives_up_instead_of_hanging allows)
        refused(lbm, "lbm_read_cells", lambda o: o.cells(), eng)


# ---- 6: a give-up in a segment of a checked run --------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["run_until", "run_until_residual"])
def test_a_checked_run_fails_and_stays_failed(lbm, monkeypatch, case, entry):
    """segments of 16 steps are one resident launch each, so a segment of look-ahead is in flight when the first verdict
    arrives; it is dropped, the rest of the cap is not run, and the call reports the give-up itself"""
    p, ob, cells, want = case
    with lbm.Engine(p, ob, cells[0]) as eng:
        info = eng.info()
        resident_serves(info, 16)
        assert 16 <= info["resident_steps"]
        eng.run(10)
        assert same_bits(eng.cells(), want[10])
        with pytest.raises(lbm.LbmError, match=ledger.FIRST_REPORT):
            one_give_up(monkeypatch, lambda: getattr(eng, entry)(72, 16, 0.0, 2))
        steps = eng.info()["steps_done"]
        assert 10 <= steps <= 10 + 32                         # at most the segment that gave up and its look-ahead
        all_refused(lbm, ledger.CTX_CALLS, eng)
        assert eng.info()["steps_done"] == steps


# ---- 7, 8: batches --------------------------------------------------------------------------------------------------------
def test_a_batch_fails_as_a_whole(lbm, oracle, monkeypatch, case):
    p, ob, cells, want = case
    batch = lbm.Batch([p] * 3, [ob] * 3, cells[:3])
    resident_serves(batch.member(0).info(), 20)
    assert batch.info()["resident_steps"] > 0 and 0 < batch.info()["resident_min_steps"] <= 20
    batch.run(10)
    assert same_bits(batch.member(0).cells(), want[10])
    one_give_up(monkeypatch, lambda: batch.run(20))
    with pytest.raises(lbm.LbmError, match=ledger.FIRST_REPORT):
        batch.sync()
    refused(lbm, "lbm_batch_sync", lambda o: o.sync(), batch)
    info = batch.info()
    assert info["steps_done"] == 30
    for i in range(3):                                        # every member, every entry point that takes one, twice
        all_refused(lbm, ledger.CTX_CALLS, batch.member(i))
    all_refused(lbm, ledger.BATCH_CALLS, batch)
    with pytest.raises(lbm.LbmError) as e:
        batch.run(20)
    assert str(e.value) == ledger.refusal("lbm_batch_run")
    res, steps = (lbm._CSteadyResult * 3)(), ctypes.c_int(-7)
    assert batch.lib.lbm_batch_run_until(batch.handle, 8, 4, 0.0, 1, res, ctypes.byref(steps)) == 1 and steps.value == 0
    # what still works
    assert batch.info() == info and ledger.batch_member_handle(batch) == batch.member(2).handle.value
    assert [batch.member(i).info()["steps_done"] for i in range(3)] == [30] * 3
    batch.close()
    with lbm.Batch([p] * 3, [ob] * 3, cells[:3]) as batch:    # a healthy successor
        batch.run(10)
        batch.run(20)
        assert same_bits(batch.member(0).cells(), want[30])


@pytest.mark.parametrize("entry", ["run_until", "run_until_residual"])
def test_a_checked_batch_run_stops_at_the_give_up(lbm, monkeypatch, case, entry):
    """the host waits for every segment's verdict, and the status word travels in front of it: the segment that gave up
    is the last one issued, and the call reports it"""
    p, ob, cells, _ = case
    with lbm.Batch([p] * 3, [ob] * 3, cells[:3]) as batch:
        resident_serves(batch.member(0).info(), 16)
        with pytest.raises(lbm.LbmError, match=ledger.FIRST_REPORT):
            one_give_up(monkeypatch, lambda: getattr(batch, entry)(72, 16, 0.0, 2))
        assert batch.info()["steps_done"] == 16
        refused(lbm, "lbm_batch_" + entry, lambda o: getattr(o, entry)(72, 16, 0.0, 2), batch)
        refused(lbm, "lbm_read_cells", lambda o: o.cells(), batch.member(1))
        assert batch.info()["steps_done"] == 16


def test_a_batch_of_two_launches_has_one_flag(lbm, monkeypatch, case):
    """nine members are launches of eight and of one per chunk: a member of the second launch is asked first, and one of the
    first launch is failed with it"""
    p, ob, cells, _ = case
    with lbm.Batch([p] * 9, [ob] * 9, cells) as batch:
        info = batch.info()
        assert info["launches_per_chunk"] == 2 and info["members_per_launch"] == 8, info
        resident_serves(batch.member(0).info(), 20)
        one_give_up(monkeypatch, lambda: batch.run(20))
        with pytest.raises(lbm.LbmError, match=ledger.FIRST_REPORT):
            batch.member(8).cells()
        refused(lbm, "lbm_read_cells", lambda o: o.cells(), batch.member(0))
        refused(lbm, "lbm_read_cells", lambda o: o.cells(), batch.member(8))
        refused(lbm, "lbm_batch_run", lambda o: o.run(20), batch)


# ---- 9: the command line (a pin of what it does today: the library ends the program at the first report) ------------------
@pytest.mark.parametrize("mode", [{}, {"LBM_STEADY": "1e-9:16"}])
def test_the_command_line_writes_no_results(lbm, monkeypatch, case, tmp_path, mode):
    p, ob, _, _ = case
    p40 = lbm.Params(p.nx, p.ny, 40, p.reynolds_dim, p.density, p.accel, p.omega)
    with lbm.Engine(p40, ob, None) as eng:
        resident_serves(eng.info(), 16)
    out = run_cli(lbm, tmp_path, params_text(p40), obstacles_text(ob), LBM_RESIDENT_ABSENT_BAND=str(ABSENT_BAND),
                  LBM_RESIDENT_TIMEOUT_MS="200", **mode)
    assert out.returncode != 0
    assert ledger.FIRST_REPORT in out.stderr, out.stderr
    assert not os.path.exists(tmp_path / "av_vels.dat") and not os.path.exists(tmp_path / "final_state.dat")
