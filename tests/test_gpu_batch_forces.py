"""Obstacle forces of a batch (lbm_batch_set_forces / Batch.set_forces): every member's rows, lattice, av_vels (all as bit
patterns) and link counts are those of a single Engine armed with Engine.set_forces on the same inputs and advanced by
the same calls, and the rows are the numpy model's (tests/forces_model.py) over the oracle's lattices, bit for bit: the
engine takes the exact sum and rounds once, so there is no tolerance to derive.  The shapes are the smallest at which the
batched gather, the sub-call loop and the sub-batch launches can go wrong."""
import ctypes

import numpy as np
import pytest

import forces_model
from test_gpu_batch import random_members
from test_gpu_forces import Shared, assert_rows, bits, run_engine, small

pytestmark = pytest.mark.gpu


def run_batch(lbm, params, obstacles, cells, calls, every, bodies=None, n_bodies=None, capacity=0, unarmed_first=0):
    """`unarmed_first` steps, then forces armed, then `calls`, drained after each:
    ([(lattice, av_vels) per member], steps, rows [n, members, n_bodies, 2], links [members, n_bodies], info)"""
    steps, rows = [], []
    with lbm.Batch(params, obstacles, cells) as batch:
        if unarmed_first:
            batch.run(unarmed_first)
        batch.set_forces(every, capacity or 1 + sum(calls) // every, bodies, n_bodies)
        links = batch.force_links()
        for n in calls:
            batch.run(n)
            s, r = batch.forces()
            steps.append(s)
            rows.append(r)
        info = batch.info()
        total = unarmed_first + sum(calls)
        assert info["steps_done"] == total
        members = [(batch.member(i).cells(), batch.member(i).av_vels(total)) for i in range(len(params))]
    return members, np.concatenate(steps), np.concatenate(rows), links, info


def assert_members_equal_engines(lbm, params, obstacles, cells, calls, every, bodies, n_bodies, got, unarmed_first=0):
    members, steps, rows, links, _ = got
    assert rows.shape == (len(steps), len(params), n_bodies, 2) and links.shape == (len(params), n_bodies)
    for i, p in enumerate(params):
        lattice, av, e_steps, e_rows, e_links, _ = run_engine(lbm, p, obstacles[i], cells[i], calls, every,
                                                              None if bodies is None else bodies[i], n_bodies,
                                                              unarmed_first=unarmed_first)
        assert steps.tolist() == e_steps.tolist(), i
        assert np.array_equal(bits(rows[:, i]), bits(e_rows)), f"member {i}: rows differ from Engine.set_forces'"
        assert np.array_equal(bits(members[i][0]), bits(lattice)), f"member {i}: lattice"
        assert np.array_equal(bits(members[i][1]), bits(av)), f"member {i}: av_vels"
        assert links[i].tolist() == e_links.tolist(), i


def assert_member_equals_model(oracle, p, ob, cells, first, total, every, bodies, n_bodies, got, i, key=None):
    make = lambda: forces_model.oracle_forces(oracle, p, ob, cells, first, total, every, bodies, n_bodies)  # noqa: E731
    ref, want = Shared.get(key, make) if key else make()
    members, steps, rows, links, _ = got
    assert_rows(steps, rows[:, i], want)
    assert np.array_equal(bits(members[i][0]), bits(ref)), f"member {i}: recording changed the lattice"
    assert links[i].tolist() == forces_model.link_counts(ob, bodies, n_bodies)


def labels_for(obstacles, n_bodies):
    """a label map per member, each its own pattern; fluid cells carry labels too (ignored)"""
    ny, nx = obstacles[0].shape
    y, x = np.mgrid[0:ny, 0:nx]
    return [((x // (3 + i) + y + i) % n_bodies).astype(np.int32) for i in range(len(obstacles))]


def resident_members(lbm, nx, ny, n, seed):
    """members that differ in omega, accel, obstacles and labels; member 0 has blocked cells on the lid row and on the
    rows 3, 7, ...; member 2 has no blocked cell at all"""
    params, obstacles, cells = random_members(lbm, nx, ny, n, seed)
    obstacles = [ob.copy() for ob in obstacles]
    obstacles[0][ny - 2, ::5] = 1
    obstacles[0][3::4, ::7] = 1
    obstacles[2][:] = 0
    return params, obstacles, cells, labels_for(obstacles, 3)


CALLS, EVERY = [1, 2, 19, 5], 3


# ---- 1. members equal single engines and the model, resident one-XCD shape ---------------------------------------------
@pytest.mark.parametrize("min_steps", ["1", "3"])
@pytest.mark.parametrize("n_members", [3, 9])
def test_members_equal_engines_and_model_one_xcd(lbm, oracle, monkeypatch, n_members, min_steps):
    """LBM_RESIDENT_MIN_STEPS 1: every sub-call runs batched (9 members: two launches per chunk); 3: the sub-calls of one
    and two steps advance the members one after another on the per-pass kernels, and the parity copy happens"""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", min_steps)
    params, obstacles, cells, bodies = resident_members(lbm, 128, 16, n_members, seed=40)
    got = run_batch(lbm, params, obstacles, cells, CALLS, EVERY, bodies, 3)
    info = got[4]
    assert info["resident_steps"] > 0 and info["resident_min_steps"] == int(min_steps), info
    assert info["members_per_launch"] == 8 and info["launches_per_chunk"] == -(-n_members // 8), info
    assert len(got[1]) == 9
    assert_members_equal_engines(lbm, params, obstacles, cells, CALLS, EVERY, bodies, 3, got)
    for i in (0, 1):                  # (the members 0 .. 2 are those of either batch size)
        assert_member_equals_model(oracle, params[i], obstacles[i], cells[i], 0, sum(CALLS), EVERY, bodies[i], 3, got, i, key=("one-xcd", i))
    rows, links = got[2], got[3]
    assert links[2].tolist() == [0, 0, 0]
    assert np.all(rows[:, 2] == 0.0) and not np.signbit(rows[:, 2]).any()      # no obstacles: +0
    assert np.all(links[0] > 0) and np.all(rows[-1, 0] != 0.0)


# ---- 2. four-row bands -------------------------------------------------------------------------------------------------
def test_four_row_bands(lbm, monkeypatch):
    monkeypatch.setenv("LBM_RESIDENT_ROWS", "4")
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "3")
    params, obstacles, cells = random_members(lbm, 128, 64, 2, seed=64)
    obstacles = [ob.copy() for ob in obstacles]
    obstacles[0][62, ::5] = 1               # lid row
    obstacles[0][3::4, ::7] = 1             # seam rows of four-row bands
    bodies = labels_for(obstacles, 3)
    got = run_batch(lbm, params, obstacles, cells, CALLS, EVERY, bodies, 3)
    assert got[4]["resident_steps"] > 0
    with lbm.Batch(params, obstacles, cells) as batch:
        assert batch.member(0).info()["resident_rows"] == 4
    assert_members_equal_engines(lbm, params, obstacles, cells, CALLS, EVERY, bodies, 3, got)


# ---- 3. multi-XCD shapes: the members of one chunk run in several launches ---------------------------------------------
@pytest.mark.parametrize("n_members,nx,ny", [(2, 256, 256), (3, 128, 256)])
def test_multi_xcd_shapes(lbm, monkeypatch, n_members, nx, ny):
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "8")       # the sub-calls of 10 steps run batched, the first (1 step) does not
    params, obstacles, cells = random_members(lbm, nx, ny, n_members, seed=7 * nx + ny)
    got = run_batch(lbm, params, obstacles, cells, [50], 10)
    info = got[4]
    assert info["resident_steps"] > 0 and info["members_per_launch"] == 2 and info["launches_per_chunk"] == -(-n_members // 2), info
    assert got[1].tolist() == [0, 10, 20, 30, 40]
    assert_members_equal_engines(lbm, params, obstacles, cells, [50], 10, None, 1, got)
    assert np.all(got[2] != 0.0)


# ---- 4. a shape the resident kernel does not take --------------------------------------------------------------------
@pytest.mark.parametrize("every", [3, 4])
def test_non_resident_shape(lbm, oracle, every):
    params, obstacles, cells = random_members(lbm, 100, 40, 3, seed=140)
    bodies = labels_for(obstacles, 2)
    got = run_batch(lbm, params, obstacles, cells, [12, 9], every, bodies, 2)
    assert got[4]["resident_steps"] == 0
    assert got[1].tolist() == [tt for tt in range(21) if tt % every == 0]
    assert_members_equal_engines(lbm, params, obstacles, cells, [12, 9], every, bodies, 2, got)
    assert_member_equals_model(oracle, params[1], obstacles[1], cells[1], 0, 21, every, bodies[1], 2, got, 1)


# ---- 5. gather geometry across unequal members -------------------------------------------------------------------------
def test_unequal_members_share_one_grid(lbm, oracle):
    """The x-extent of the grid is that of member 0's body 0 (several workgroups); the other (member, body) pairs have
    20 links, a ragged last wave, or none: their spare workgroups return at once"""
    p, ob, c0 = small(lbm, 128, 32, 4)
    obstacles = [ob.copy() for _ in range(3)]
    bodies = [np.zeros_like(ob) for _ in range(3)]
    obstacles[0][2:30:2, 4:124:2] = 1         # body 0: 14 x 60 isolated cells, 8 links each
    obstacles[0][13:16, 61:64] = 1            # a solid 3 x 3 block: body 1 its rim, body 2 its enclosed centre
    bodies[0][13:16, 61:64] = 1
    bodies[0][14, 62] = 2
    obstacles[1][7:9, 50:52] = 1              # one 2 x 2 block, body 1
    bodies[1][:] = 1
    obstacles[2][5, 10:32] = 1                # a run along x (134 links), body 2
    bodies[2][:] = 2
    counts = [forces_model.link_counts(o, b, 3) for o, b in zip(obstacles, bodies)]
    assert counts[0][0] > 4 * 1024 and counts[0][1] > 0 and counts[0][2] == 0
    assert counts[1] == [0, 20, 0]
    assert counts[2][2] > 64 and counts[2][2] % 64 != 0 and counts[2][:2] == [0, 0]
    params = [lbm.Params(128, 32, 400, 10, 0.1, 0.005 + 0.001 * i, 1.85 - 0.1 * i) for i in range(3)]
    cells = [c0, small(lbm, 128, 32, 5)[2], small(lbm, 128, 32, 6)[2]]
    got = run_batch(lbm, params, obstacles, cells, [6], 3, bodies, 3)
    assert got[3].tolist() == counts
    for i in range(3):
        assert_member_equals_model(oracle, params[i], obstacles[i], cells[i], 0, 6, 3, bodies[i], 3, got, i)
    rows = got[2]
    assert np.all(rows[:, 0, 2] == 0.0) and not np.signbit(rows[:, 0, 2]).any()
    assert np.all(rows[:, 0, :2] != 0.0) and np.all(rows[:, 1, 1] != 0.0) and np.all(rows[:, 2, 2] != 0.0)


def test_max_bodies(lbm, oracle, monkeypatch):
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "2")
    p, ob, c0 = small(lbm, 128, 16, 5)
    obstacles, bodies = [ob.copy(), ob.copy()], [np.full_like(ob, -1), np.full_like(ob, -1)]   # fluid cells: labels outside the range
    for i in range(2):
        for b in range(lbm.LBM_MAX_BODIES):
            y, x = 1 + 2 * (b // 16), 3 + 8 * (b % 16) + i
            obstacles[i][y, x:x + 1 + (b + i) % 3] = 1
            bodies[i][y, x:x + 1 + (b + i) % 3] = b
    params = [p, lbm.Params(128, 16, 400, 10, 0.1, 0.004, 1.7)]
    cells = [c0, small(lbm, 128, 16, 6)[2]]
    got = run_batch(lbm, params, obstacles, cells, [4, 9], 3, bodies, lbm.LBM_MAX_BODIES)
    assert got[2].shape == (5, 2, 64, 2) and got[4]["resident_steps"] > 0
    for i in range(2):
        assert_member_equals_model(oracle, params[i], obstacles[i], cells[i], 0, 13, 3, bodies[i], 64, got, i)


def test_non_finite_term_makes_only_its_body_nan(lbm):
    """Member 1 starts with +inf in the population that moves from the fluid cell (8, 3) into body 0's blocked cell (7, 3):
    after the first step it sits on a boundary link of that body.  That body of that member is NaN in that row; the other
    body, 50 cells away, and the other member stay finite.  Every row is the single engine's, NaN included."""
    p, ob, c0 = small(lbm, 128, 16, 7)
    ob[3:5, 6:8] = 1
    ob[9:11, 60:62] = 1
    bodies = np.zeros_like(ob)
    bodies[9:11, 60:62] = 1
    cells = [c0, c0.copy()]
    cells[1][3, 8, 3] = np.inf
    got = run_batch(lbm, [p, p], [ob, ob], cells, [3], 1, [bodies, bodies], 2)
    rows = got[2]
    assert got[1].tolist() == [0, 1, 2] and np.isnan(rows[0, 1, 0]).all()
    assert np.isfinite(rows[:, 0]).all() and np.isfinite(rows[:, 1, 1]).all()
    assert_members_equal_engines(lbm, [p, p], [ob, ob], cells, [3], 1, [bodies, bodies], 2, got)


# ---- 6. the ring and the numbering -------------------------------------------------------------------------------------
def test_armed_after_unarmed_steps_and_ragged_split(lbm):
    params, obstacles, cells = random_members(lbm, 128, 16, 2, seed=16)
    whole = run_batch(lbm, params, obstacles, cells, [63], 4, unarmed_first=5)
    ragged = run_batch(lbm, params, obstacles, cells, [1, 2, 13, 4, 30, 1, 12], 4, unarmed_first=5)
    assert whole[1].tolist() == ragged[1].tolist() == [tt for tt in range(5, 68) if tt % 4 == 0]     # the first: 8
    assert np.array_equal(bits(whole[2]), bits(ragged[2]))
    for i in range(2):      # (not av_vels: calls of other lengths run other kernels, which sum |u| in another order)
        assert np.array_equal(bits(whole[0][i][0]), bits(ragged[0][i][0]))
    assert_members_equal_engines(lbm, params, obstacles, cells, [63], 4, None, 1, whole, unarmed_first=5)


def test_ring_overflow_drain_order_query_rearm_disarm(lbm):
    params, obstacles, cells = random_members(lbm, 128, 16, 3, seed=23)
    with lbm.Batch(params, obstacles, cells) as batch:
        n = batch.lib.lbm_batch_read_forces
        done = lambda: [batch.member(i).info()["steps_done"] for i in range(3)] + [batch.info()["steps_done"]]  # noqa: E731
        batch.set_forces(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run: 25 steps would record 3 rows.*holds 2.*lbm_batch_read_forces"):
            batch.run(25)                    # rows at 0, 10, 20
        assert done() == [0, 0, 0, 0]
        batch.run(15)                        # 0, 10
        with pytest.raises(lbm.LbmError, match="2 rows are waiting"):
            batch.run(10)
        assert done() == [15, 15, 15, 15]
        waiting = ctypes.c_int(-1)
        assert n(batch.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # the query form
        assert n(batch.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # ... drains nothing
        steps, first = batch.forces(1)
        assert steps.tolist() == [0] and first.shape == (1, 3, 1, 2)                                # oldest first
        batch.run(10)                        # 20 goes into the slot that 0 left
        steps, rows = batch.forces()
        assert steps.tolist() == [10, 20] and not np.array_equal(rows[0], rows[1])
        batch.run(6)                         # 30
        batch.set_forces(10, 2)              # re-arming discards the unread row
        assert batch.forces()[0].size == 0
        batch.run(10)                        # 40
        assert batch.forces()[0].tolist() == [40]
        batch.set_forces(0)                  # disarms and frees
        with pytest.raises(lbm.LbmError, match="not armed"):
            batch.force_links()
        batch.run(30)
        assert n(batch.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 0
        assert batch.forces()[0].size == 0
        assert done() == [71, 71, 71, 71]


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(lbm):
    params, obstacles, cells = random_members(lbm, 128, 16, 3, seed=31)
    with lbm.Batch(params, obstacles, cells) as batch:
        lib, h = batch.lib, batch.handle
        for n_bodies, every, cap, msg in ((0, 1, 4, "0 bodies, between 1 and LBM_MAX_BODIES = 64"),
                                          (65, 1, 4, "65 bodies, between 1 and LBM_MAX_BODIES = 64"),
                                          (1, -1, 4, "negative interval -1"), (1, 1, 0, "capacity 0, at least one row"),
                                          (1, 1, -2, "capacity -2"),
                                          (64, 1, 69906, "a ring of 69906 rows of 3 members of 64 bodies is 2.00 GiB, 2 GiB or more")):
            assert lib.lbm_batch_set_forces(h, n_bodies, None, every, cap) != 0
            assert lib.lbm_last_error().decode().startswith("lbm_batch_set_forces: ") and msg in lib.lbm_last_error().decode()
        lab = [np.zeros((16, 128), dtype=np.int32) for _ in range(3)]
        y, x = [int(v[-1]) for v in np.nonzero(obstacles[1])]
        for bad in (2, -1):
            lab[1][y, x] = bad
            with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_forces: member 1: the blocked cell \(%d, %d\) has body %d, outside 0 .. 1" % (x, y, bad)):
                batch.set_forces(10, 4, lab, 2)
        with pytest.raises(lbm.LbmError, match="not armed"):             # a failed arming leaves the batch disarmed ...
            batch.force_links()
        batch.run(3)                                                    # ... and runnable
        assert batch.forces()[0].size == 0
        lab[1][y, x] = 1
        lab[1][obstacles[1] == 0] = 77                                   # fluid cells: ignored
        batch.set_forces(10, 4, lab, 2)
        assert batch.force_links().sum(axis=1).tolist() == [len(forces_model.links(ob)) for ob in obstacles]
        # the member-level setters while the batch's forces are armed
        m = batch.member(2)
        for arm in (lambda: m.set_frames(10, 2), lambda: m.set_probes([(1, 1)], 1, 4), lambda: m.set_mean(10),
                    lambda: m.set_field_frames(10, 2)):
            with pytest.raises(lbm.LbmError, match=r"this batch has obstacle forces armed \(lbm_batch_set_forces\)"):
                arm()
        with pytest.raises(lbm.LbmError, match="lbm_set_forces: not available on a member of a batch"):
            batch.member(0).set_forces(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_run_until: obstacle forces are armed \(lbm_batch_set_forces\)"):
            batch.run_until(100, 10)
        assert batch.info()["steps_done"] == 3
        batch.set_forces(0)
        # a member with a recorder of its own
        for arm, disarm, kind in ((lambda: m.set_frames(10, 2), lambda: m.set_frames(0), "animation frames"),
                                  (lambda: m.set_probes([(1, 1)], 1, 4), lambda: m.set_probes([], 0), "point probes"),
                                  (lambda: m.set_mean(10), lambda: m.set_mean(0), "mean fields"),
                                  (lambda: m.set_field_frames(10, 2), lambda: m.set_field_frames(0), "field frames")):
            arm()
            with pytest.raises(lbm.LbmError, match="lbm_batch_set_forces: member 2 has %s armed" % kind):
                batch.set_forces(10, 4)
            disarm()
        batch.set_forces(10, 4)
        batch.run(8)
        assert batch.forces()[0].tolist() == [10]
    with lbm.Batch(params, obstacles, cells) as batch:
        with pytest.raises(lbm.LbmError, match="lbm_set_forces: not available on a member of a batch"):
            batch.member(0).set_forces(10, 4)
