"""Lattice statistics of a batch (lbm_batch_set_stats / Batch.set_stats): every member's rows, lattice and av_vels (all
as bit patterns) are those of a single Engine armed with Engine.set_stats on the same inputs and advanced by the same
calls, and the rows are the numpy model's (tests/stats_model.py) over the oracle's lattices, bit for bit.  One member
seeded with a population that is not finite leaves the others untouched."""
import ctypes

import numpy as np
import pytest

import stats_model
from test_gpu_batch import random_members
from test_gpu_forces import bits
from test_gpu_stats import assert_rows, run_engine

pytestmark = pytest.mark.gpu


def run_batch(lbm, params, obstacles, cells, calls, every, capacity=0, unarmed_first=0):
    """`unarmed_first` steps, then statistics armed, then `calls`, drained after each:
    ([(lattice, av_vels) per member], steps, rows [n, members], info)"""
    steps, rows = [], []
    with lbm.Batch(params, obstacles, cells) as batch:
        if unarmed_first:
            batch.run(unarmed_first)
        batch.set_stats(every, capacity or 1 + sum(calls) // every)
        for n in calls:
            batch.run(n)
            s, r = batch.stats()
            steps.append(s)
            rows.append(r)
        info = batch.info()
        total = unarmed_first + sum(calls)
        assert info["steps_done"] == total
        members = [(batch.member(i).cells(), batch.member(i).av_vels(total)) for i in range(len(params))]
    return members, np.concatenate(steps), np.concatenate(rows), info


def same(a, b):
    """two lattices or series, bit for bit, NaN cells by position (a NaN's payload is not the arithmetic's to keep)"""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def assert_members_equal_engines(lbm, params, obstacles, cells, calls, every, got, unarmed_first=0):
    members, steps, rows, _ = got
    assert rows.shape == (len(steps), len(params)) and rows.dtype == lbm.STATS_DTYPE
    for i, p in enumerate(params):
        lattice, av, e_steps, e_rows, _, _ = run_engine(lbm, p, obstacles[i], cells[i], calls, every, unarmed_first=unarmed_first)
        assert steps.tolist() == e_steps.tolist(), i
        assert np.ascontiguousarray(rows[:, i]).tobytes() == e_rows.tobytes(), f"member {i}: rows differ from Engine.set_stats'"
        assert same(members[i][0], lattice), f"member {i}: lattice"
        assert same(members[i][1], av), f"member {i}: av_vels"


def assert_member_equals_model(oracle, p, ob, cells, first, total, every, got, i):
    start = cells.copy()
    oracle.run(p, start, ob, first)
    ref, want = stats_model.oracle_rows(oracle, p, ob, start, first, total, every)
    members, steps, rows, _ = got
    assert_rows(steps, rows[:, i], want)
    assert same(members[i][0], ref), f"member {i}: recording changed the lattice"


def varied(lbm, nx, ny, n, seed):
    """members that differ in omega, accel and obstacle map (random_members); the last has no blocked cell at all"""
    params, obstacles, cells = random_members(lbm, nx, ny, n, seed)
    obstacles = [ob.copy() for ob in obstacles]
    obstacles[-1][:] = 0
    assert len({(p.omega, p.accel) for p in params}) == n
    return params, obstacles, [c.copy() for c in cells]


@pytest.mark.parametrize("n_members,nx,ny,per_launch", [(3, 128, 128, 8), (2, 256, 256, 2)])
def test_members_equal_engines_and_model(lbm, oracle, monkeypatch, n_members, nx, ny, per_launch):
    """3 members of 128 x 128 (one XCD each) and 2 of 256 x 256; the calls straddle resident_min_steps = 8: the sub-calls of
    10 steps run batched, those of 1, 3 and 7 advance the members one after another on the per-pass kernels.  Member 1
    starts with +Inf in one population of a fluid cell: its rows count the cells that spreads to, the others' stay clean."""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "8")
    params, obstacles, cells = varied(lbm, nx, ny, n_members, seed=nx + n_members)
    y, x = [int(v[0]) for v in np.nonzero(obstacles[1] == 0)]
    cells[1][y, x, 1] = np.inf
    calls, every = [1, 23, 7], 10
    got = run_batch(lbm, params, obstacles, cells, calls, every)
    _, steps, rows, info = got
    assert info["resident_steps"] > 0 and info["resident_min_steps"] == 8 and info["members_per_launch"] == per_launch, info
    assert steps.tolist() == [0, 10, 20, 30]
    assert_members_equal_engines(lbm, params, obstacles, cells, calls, every, got)
    for i in (0, 1):
        assert_member_equals_model(oracle, params[i], obstacles[i], cells[i], 0, sum(calls), every, got, i)
    assert np.all(rows["nonfinite"][:, 1] > 0) and rows["nonfinite"][-1, 1] > rows["nonfinite"][0, 1]
    others = [i for i in range(n_members) if i != 1]
    assert np.all(rows["nonfinite"][:, others] == 0) and np.all(rows["max_u"][:, others] > 0)
    assert all(np.isfinite(got[0][i][0]).all() for i in others)


def test_non_resident_shape_and_scalar_path(lbm, oracle):
    """100 x 40 is no resident shape (the member table is made at arming); 102 x 12 takes one cell per lane"""
    for nx, ny in ((100, 40), (102, 12)):
        params, obstacles, cells = varied(lbm, nx, ny, 3, seed=140 + nx)
        got = run_batch(lbm, params, obstacles, cells, [12, 9], 4)
        assert got[3]["resident_steps"] == 0 and got[1].tolist() == [0, 4, 8, 12, 16, 20]
        assert_members_equal_engines(lbm, params, obstacles, cells, [12, 9], 4, got)
        assert_member_equals_model(oracle, params[1], obstacles[1], cells[1], 0, 21, 4, got, 1)


def test_armed_after_unarmed_steps_and_ragged_split(lbm):
    params, obstacles, cells = varied(lbm, 128, 16, 2, seed=16)
    whole = run_batch(lbm, params, obstacles, cells, [63], 4, unarmed_first=5)
    ragged = run_batch(lbm, params, obstacles, cells, [1, 2, 13, 4, 30, 1, 12], 4, unarmed_first=5)
    assert whole[1].tolist() == ragged[1].tolist() == [tt for tt in range(5, 68) if tt % 4 == 0]     # the first: 8
    assert whole[2].tobytes() == ragged[2].tobytes()
    for i in range(2):
        assert np.array_equal(bits(whole[0][i][0]), bits(ragged[0][i][0]))
    assert_members_equal_engines(lbm, params, obstacles, cells, [63], 4, whole, unarmed_first=5)


def test_ring_overflow_drain_order_query_rearm_disarm(lbm):
    params, obstacles, cells = varied(lbm, 128, 16, 3, seed=23)
    with lbm.Batch(params, obstacles, cells) as batch:
        n = batch.lib.lbm_batch_read_stats
        done = lambda: [batch.member(i).info()["steps_done"] for i in range(3)] + [batch.info()["steps_done"]]  # noqa: E731
        batch.set_stats(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run: 25 steps would record 3 rows.*holds 2.*lbm_batch_read_stats"):
            batch.run(25)                    # rows at 0, 10, 20
        assert done() == [0, 0, 0, 0]        # a run without room moves no member
        batch.run(15)                        # 0, 10
        with pytest.raises(lbm.LbmError, match="2 rows are waiting"):
            batch.run(10)
        assert done() == [15, 15, 15, 15]
        waiting = ctypes.c_int(-1)
        assert n(batch.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # the query form
        assert n(batch.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # ... drains nothing
        steps, first = batch.stats(1)
        assert steps.tolist() == [0] and first.shape == (1, 3)                                      # oldest first
        batch.run(10)                        # 20 goes into the slot that 0 left
        steps, rows = batch.stats()
        assert steps.tolist() == [10, 20] and rows.shape == (2, 3) and np.all(rows["mom_x"][0] != rows["mom_x"][1])
        batch.run(6)                         # 30
        batch.set_stats(10, 2)               # re-arming discards the unread row
        assert batch.stats()[0].size == 0
        batch.run(10)                        # 40
        assert batch.stats()[0].tolist() == [40]
        batch.set_stats(0)                   # disarms and frees
        batch.run(30)
        assert n(batch.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 0
        assert batch.stats()[0].size == 0
        assert done() == [71, 71, 71, 71]


def test_refusals(lbm):
    params, obstacles, cells = varied(lbm, 128, 16, 3, seed=31)
    with lbm.Batch(params, obstacles, cells) as batch:
        lib, h = batch.lib, batch.handle
        for every, cap, msg in ((-1, 4, "negative interval -1"), (1, 0, "capacity 0, at least one row"), (1, -2, "capacity -2"),
                                (1, 2236963, "a ring of 2236963 rows of 3 members is 2.00 GiB, 2 GiB or more")):
            assert lib.lbm_batch_set_stats(h, every, cap) != 0
            assert lib.lbm_last_error().decode().startswith("lbm_batch_set_stats: ") and msg in lib.lbm_last_error().decode()
        batch.run(3)                                                    # a refused arming leaves the batch runnable
        assert batch.stats()[0].size == 0
        batch.set_stats(10, 4)
        # the member-level setters, and the batch's forces, while the batch's statistics are armed
        m = batch.member(2)
        for arm in (lambda: m.set_frames(10, 2), lambda: m.set_probes([(1, 1)], 1, 4), lambda: m.set_mean(10),
                    lambda: m.set_field_frames(10, 2)):
            with pytest.raises(lbm.LbmError, match=r"this batch has lattice statistics armed \(lbm_batch_set_stats\)"):
                arm()
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_forces: this batch has lattice statistics armed \(lbm_batch_set_stats\)"):
            batch.set_forces(10, 4)
        batch.set_forces(0)                                             # disarming the forces leaves the statistics alone
        with pytest.raises(lbm.LbmError, match="lbm_set_stats: not available on a member of a batch"):
            batch.member(0).set_stats(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_run_until: lattice statistics are armed \(lbm_batch_set_stats\)"):
            batch.run_until(100, 10)
        assert batch.info()["steps_done"] == 3
        batch.run(8)
        assert batch.stats()[0].tolist() == [10]
        batch.set_stats(0)
        # the other way round: a member with a recorder of its own, the batch's forces
        for arm, disarm, kind in ((lambda: m.set_frames(10, 2), lambda: m.set_frames(0), "animation frames"),
                                  (lambda: m.set_probes([(1, 1)], 1, 4), lambda: m.set_probes([], 0), "point probes"),
                                  (lambda: m.set_mean(10), lambda: m.set_mean(0), "mean fields"),
                                  (lambda: m.set_field_frames(10, 2), lambda: m.set_field_frames(0), "field frames")):
            arm()
            with pytest.raises(lbm.LbmError, match="lbm_batch_set_stats: member 2 has %s armed" % kind):
                batch.set_stats(10, 4)
            disarm()
        batch.set_forces(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_stats: this batch has obstacle forces armed \(lbm_batch_set_forces\)"):
            batch.set_stats(10, 4)
        batch.set_stats(0)                                              # ... and leaves the forces alone
        batch.run(10)
        assert batch.forces()[0].tolist() == [20]
        batch.set_forces(0)
        batch.set_stats(10, 4)
        batch.run(10)
        assert batch.stats()[0].tolist() == [30]
