"""Velocity residuals (lbm_set_residual / Engine.set_residual, lbm_batch_set_residual / Batch.set_residual): after every
global timestep tt with tt % every == 0 one row of how far the velocity field is from the field remembered at the last
sample (at first: at arming).  Every row is compared BIT FOR BIT with the numpy model (tests/residual_model.py) over the
oracle's lattices: the sums are exact and rounded once, the maximum does not depend on order, so every kernel path, call
splitting, slab count and a batch member give the same bits; recording never changes the lattice, and av_vels equals
that of the same run issued as calls split at the sample steps."""
import ctypes

import numpy as np
import pytest

import edge_lattice as el
import residual_model
import test_frames_format as model
from test_gpu_batch import random_members
from test_gpu_forces import FAMILIES, RESIDENT_SHAPES, Shared, bits, small
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu

BLOCK, MAX_GROUPS = 256, 512            # residual_gather: lanes per workgroup, the cap of the grid


def run_engine(lbm, p, ob, cells, calls, every=0, capacity=0, n_gpus=1, unarmed_first=0, tiled=False):
    """`unarmed_first` steps, then residuals armed, then `calls`, drained after each: (lattice, av_vels, steps, rows, info)"""
    steps, rows = [], []
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus, tiled=tiled) as eng:
        if unarmed_first:
            eng.run(unarmed_first)
        if every:
            eng.set_residual(every, capacity or 1 + sum(calls) // every)
        for n in calls:
            eng.run(n)
            if every:
                s, r = eng.residuals()
                steps.append(s)
                rows.append(r)
        total = unarmed_first + sum(calls)
        return (eng.cells(), eng.av_vels(total), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(rows) if rows else np.zeros(0, lbm.RESIDUAL_DTYPE), eng.info())


def assert_rows(steps, rows, want):
    """want: {tt: row of residual_model.row}"""
    assert steps.tolist() == sorted(want)
    for tt, row in zip(steps.tolist(), rows):
        diff = residual_model.same_bits(row, want[tt])
        print("step", tt, {k: row[k] for k in residual_model.FIELDS}, "differs:", diff)
        assert not diff, (tt, diff)


def split_calls(unarmed_first, calls, every):
    """the same steps as calls cut after every sample step, counted in global steps"""
    split, done = [], 0
    for n in [unarmed_first] + list(calls):
        end = done + n
        for c in [tt + 1 for tt in model.frame_steps(done, end, every) if tt >= unarmed_first] + [end]:
            if c > done:
                split.append(c - done)
                done = c
    return split


def same(a, b):
    """two lattices or series, bit for bit, NaN cells by position (a NaN's payload is not the arithmetic's to keep)"""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def check(lbm, oracle, p, ob, cells, calls, every, unarmed_first=0, n_gpus=1, want=None, ref=None, tiled_ob=None):
    """armed run against the model on the oracle's lattices; lattice and av_vels against the unarmed run split at the sample steps"""
    if want is None:
        start = cells.copy()
        with np.errstate(all="ignore"):
            oracle.run(p, start, ob, unarmed_first)
        ref, want = residual_model.oracle_rows(oracle, p, ob, start, unarmed_first, sum(calls), every)
    engine_ob = ob if tiled_ob is None else tiled_ob
    got, av, steps, rows, info = run_engine(lbm, p, engine_ob, cells, calls, every, n_gpus=n_gpus, unarmed_first=unarmed_first,
                                            tiled=tiled_ob is not None)
    assert_rows(steps, rows, want)
    assert same(ref, got), "recording changed the lattice"
    base, base_av, _, _, _ = run_engine(lbm, p, engine_ob, cells, split_calls(unarmed_first, calls, every), n_gpus=n_gpus,
                                        tiled=tiled_ob is not None)
    assert same(base, got)
    assert same(base_av, av), "recording changed av_vels"
    return steps, rows, info


def smallest(lbm):
    p, ob, cells = small(lbm, 16, 8)
    ob[3:5, 6:8] = 1
    return p, ob, cells


# ---- shapes: the smallest at which residual_gather can go wrong ---------------------------------------------------------
def test_smallest_case(lbm, oracle):
    p, ob, cells = smallest(lbm)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [5, 7], 1)
    assert len(steps) == 12 and len(set(rows["sum_du_sq"].tolist())) == 12 and np.all(rows["span"] == 1)
    assert np.all(rows["nonfinite"] == 0) and np.all(rows["max_du"] > 0)
    one = run_engine(lbm, p, ob, cells, [12], 1)
    assert one[2].tolist() == steps.tolist() and one[3].tobytes() == rows.tobytes()         # one call: the same bits


def test_baseline_after_unarmed_steps_and_rearming(lbm, oracle):
    p, ob, cells = smallest(lbm)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [12], 4, unarmed_first=6)
    assert steps.tolist() == [8, 12, 16] and rows["span"].tolist() == [3, 4, 4]
    # re-arming mid-run: the unread row of step 8 is gone, the baseline is the lattice after 11 steps
    start = cells.copy()
    oracle.run(p, start, ob, 11)
    ref, want = residual_model.oracle_rows(oracle, p, ob, start, 11, 7, 4)
    with lbm.Engine(p, ob, cells) as eng:
        eng.run(6)
        eng.set_residual(4, 4)
        eng.run(5)
        waiting = ctypes.c_int(-1)
        assert eng.lib.lbm_read_residual(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 1
        eng.set_residual(4, 4)
        assert eng.residuals()[0].size == 0
        eng.run(7)
        steps, rows = eng.residuals()
        assert_rows(steps, rows, want)
        assert steps.tolist() == [12, 16] and rows["span"].tolist() == [2, 4]
        assert same(ref, eng.cells())


@pytest.mark.parametrize("nx,ny", [(21, 3), (16, 4), (13, 5), (85, 3), (16, 16), (257, 3), (130, 6), (252, 4), (260, 4)])
def test_lane_wave_and_workgroup_edges(lbm, oracle, nx, ny):
    """cells just below, at and above a wave (63, 64, 65) and a workgroup (255, 256, 771 = 3 * 257); widths that are no
    multiple of 4 take one cell per lane and leave pitch padding behind every row of the lattice, none in the planes;
    252 x 4 and 260 x 4 put the four-cell units just below and above one workgroup's 256"""
    p, ob, cells = small(lbm, nx, ny, nx + ny)
    ob[1, 2:4] = 1
    ob[ny - 1, nx - 1] = 1                               # the last owned cell is blocked
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [5], 2)
    assert steps.tolist() == [0, 2, 4] and rows["span"].tolist() == [1, 2, 2]


@pytest.mark.parametrize("nx,ny", [(1024, 1024), (1030, 512)])
def test_capped_grid_every_workgroup_loops(lbm, oracle, nx, ny):
    """more units than the capped grid has lanes, twice over: every workgroup takes its loop at least twice (four cells
    per lane on 1024 x 1024, one on 1030 x 512)"""
    units = nx * ny // (4 if nx % 4 == 0 else 1)
    assert units >= 2 * MAX_GROUPS * BLOCK
    p, ob, cells = random_case(lbm, nx, ny, 11, walls=False)
    check(lbm, oracle, p, ob, cells, [1], 1)


def test_every_limb(lbm, oracle):
    """the lattice of tests/edge_lattice.py: populations over all the exponents the collision guards allow, so the limbs
    of both accumulators are used"""
    p, ob, cells, _ = el.build(lbm, 256, 40)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [el.STEPS], 1)
    assert len(steps) == el.STEPS


# ---- ties and rest --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_gpus", [1, 2])
def test_ties_take_the_smallest_cell(lbm, oracle, monkeypatch, n_gpus):
    """A channel from the uniform equilibrium stays x-invariant: a whole row ties and max_x must be 0.  One slab: the
    bottom row blocked.  Two slabs of eight rows: rows 4 and 8 blocked, which lie mirrored about the lid row 14, so the
    driven channel (rows 9 .. 15, 0 .. 3) is cut between the slabs."""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p = lbm.Params(64, 16, 400, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((16, 64), dtype=np.int32)
    ob[[0] if n_gpus == 1 else [4, 8], :] = 1
    steps, rows, info = check(lbm, oracle, p, ob, oracle.init_cells(p), [12], 4, n_gpus=n_gpus)
    assert info["n_slabs"] == n_gpus
    assert np.all(rows["max_x"] == 0) and np.all(rows["max_du"] > 0)


def test_nothing_moves_at_rest(lbm, oracle):
    """without acceleration the uniform equilibrium stays at rest: both sums are +0.0 and the first fluid cell, (3, 0),
    carries the maximum 0"""
    p = lbm.Params(16, 8, 400, 10, 0.1, 0.0, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[0, :3] = ob[3:5, 6:8] = 1
    steps, rows, _ = check(lbm, oracle, p, ob, oracle.init_cells(p), [4], 2)
    assert len(rows) == 2
    for r in rows:
        assert (r["max_du"], r["max_x"], r["max_y"]) == (0.0, 3, 0)
        for k in ("sum_du_sq", "sum_u_sq"):
            assert r[k] == 0.0 and not np.signbit(r[k])
    assert lbm.residual_l2(rows).tolist() == [0.0, 0.0]


# ---- non-finite cells -----------------------------------------------------------------------------------------------------
def test_nonfinite_cells_are_counted_and_left_out(lbm, oracle):
    p, ob, cells = smallest(lbm)
    steps, rows, _ = check(lbm, oracle, p, ob, residual_model.poisoned(cells), [3], 1)
    assert tuple(rows["nonfinite"].tolist()) == residual_model.POISON_COUNTS
    assert np.all(np.isfinite(rows["sum_du_sq"])) and np.all(rows["sum_du_sq"] > 0)           # the sums are taken over the rest


# ---- slabs ----------------------------------------------------------------------------------------------------------------
def slab_case(lbm, oracle):
    """128 x 96 from a 32 x 16 obstacle tile with blocked cells on its first and last row, so on the first and last row
    of every slab of 2 and of 3; armed after 5 steps; the model's rows every 4 steps over 21 more"""
    def make():
        tile = np.zeros((16, 32), dtype=np.int32)
        tile[0, 0] = tile[0, 11:14] = tile[15, 31] = tile[15, 20] = tile[5:8, 9:12] = 1
        ob = np.tile(tile, (6, 4))
        p, _, cells = random_case(lbm, 128, 96, 21, walls=False)
        for parts in (2, 3):
            for first, count in (lbm.partition_rows(96, parts, s) for s in range(parts)):
                assert ob[first].any() and ob[first + count - 1].any() and ob[first + count - 1, 127] and ob[first, 0]
        start = cells.copy()
        oracle.run(p, start, ob, 5)
        ref, want = residual_model.oracle_rows(oracle, p, ob, start, 5, 21, 4)
        # some maxima lie in the last of 2 slabs and in the second and third of 3: their cells must come out global
        assert {r["max_y"] // 48 for r in want.values()} == {0, 1} and {r["max_y"] // 32 for r in want.values()} == {0, 1, 2}
        return p, ob, tile, cells, ref, want
    return Shared.get(("residual", "slabs"), make)


@pytest.mark.parametrize("layout", ["1 slab", "2 slabs", "3 slabs", "tiled"])
def test_slabs_and_a_tiled_context(lbm, oracle, monkeypatch, layout):
    """each slab keeps its own planes and gathers into its own words with global cell indices; the host adds the limbs and
    takes the largest key: the four layouts give the model's bits, so identical ones"""
    p, ob, tile, cells, ref, want = slab_case(lbm, oracle)
    monkeypatch.setenv("LBM_HALO", "memcpy")
    n_gpus = {"1 slab": 1, "2 slabs": 2, "3 slabs": 3, "tiled": 1}[layout]
    steps, rows, info = check(lbm, oracle, p, ob, cells, [9, 12], 4, unarmed_first=5, n_gpus=n_gpus, want=want, ref=ref,
                              tiled_ob=tile if layout == "tiled" else None)
    assert info["n_slabs"] == n_gpus and steps.tolist() == [8, 12, 16, 20, 24] and rows["span"].tolist() == [4, 4, 4, 4, 4]
    first = Shared.get(("residual", "slabs", "bytes"), rows.tobytes)
    assert rows.tobytes() == first


# ---- kernel families ------------------------------------------------------------------------------------------------------
CALLS, EVERY = [1, 2, 19, 5], 3


@pytest.mark.parametrize("min_steps", ["1", "3"])
@pytest.mark.parametrize("shape", list(RESIDENT_SHAPES))
def test_resident_shapes(lbm, oracle, monkeypatch, shape, min_steps):
    nx, ny, env = RESIDENT_SHAPES[shape]

    def make():
        p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
        ref, want = residual_model.oracle_rows(oracle, p, ob, cells, 0, sum(CALLS), EVERY)
        return p, ob, cells, ref, want
    p, ob, cells, ref, want = Shared.get(("residual", shape), make)
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", min_steps)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    steps, rows, info = check(lbm, oracle, p, ob, cells, CALLS, EVERY, want=want, ref=ref)
    assert info["resident_steps"] > 0 and len(steps) == 9


@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_pass_families(lbm, oracle, monkeypatch, family):
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)

    def make():
        p, ob, _, cells, _, _ = slab_case(lbm, oracle)
        ref, want = residual_model.oracle_rows(oracle, p, ob, cells, 0, sum(CALLS), EVERY)
        return p, ob, cells, ref, want
    p, ob, cells, ref, want = Shared.get(("residual", "per-pass"), make)
    steps, rows, info = check(lbm, oracle, p, ob, cells, CALLS, EVERY, want=want, ref=ref)
    assert info["resident_steps"] == 0 and len(steps) == 9


# ---- against the statistics -------------------------------------------------------------------------------------------------
def test_sum_u_sq_is_the_statistics(lbm):
    p, ob, cells = random_case(lbm, 128, 64, 9, walls=False)
    with lbm.Engine(p, ob, cells) as a, lbm.Engine(p, ob, cells) as b:
        a.set_residual(5, 8)
        b.set_stats(5, 8)
        a.run(23)
        b.run(23)
        steps, rows = a.residuals()
        s_steps, s_rows = b.stats()
    assert steps.tolist() == s_steps.tolist() == [0, 5, 10, 15, 20]
    assert np.all(rows["nonfinite"] == 0) and np.all(s_rows["nonfinite"] == 0)
    assert np.array_equal(bits(rows["sum_u_sq"]), bits(s_rows["sum_u_sq"]))


# ---- the ring -------------------------------------------------------------------------------------------------------------
def test_ring_overflow_drain_order_query_disarm(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        n = eng.lib.lbm_read_residual
        eng.set_residual(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_run: 25 steps would record 3 rows.*holds 2.*lbm_read_residual"):
            eng.run(25)                      # rows at 0, 10, 20
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match="2 rows are waiting"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        waiting = ctypes.c_int(-1)
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # the query form
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # ... drains nothing
        steps, first = eng.residuals(1)
        assert steps.tolist() == [0] and first.shape == (1,) and first["span"].tolist() == [1]     # oldest first
        eng.run(10)                          # 20 goes into the slot that 0 left
        steps, rows = eng.residuals()
        assert steps.tolist() == [10, 20] and rows["span"].tolist() == [10, 10]
        assert rows[0]["sum_du_sq"] != rows[1]["sum_du_sq"] and first[0]["sum_du_sq"] != rows[1]["sum_du_sq"]
        eng.set_residual(0)                  # disarms and frees
        eng.run(30)
        assert eng.residuals()[0].size == 0
        assert eng.info()["steps_done"] == 55


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 4, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        for every, cap, msg in ((-1, 4, "lbm_set_residual: negative interval -1"), (1, 0, "lbm_set_residual: capacity 0, at least one row"),
                                (1, -2, "lbm_set_residual: capacity -2"),
                                (1, 2 ** 24, "lbm_set_residual: a ring of 16777216 rows is 2 GiB or more")):
            assert eng.lib.lbm_set_residual(eng.handle, every, cap) != 0
            assert msg in eng.lib.lbm_last_error().decode()
        assert eng.info()["steps_done"] == 0
        # one recorder per context, both directions
        for arm, disarm, name in ((lambda: eng.set_frames(10, 2), lambda: eng.set_frames(0), "animation frames"),
                                  (lambda: eng.set_probes([(1, 1)], 1, 4), lambda: eng.set_probes([], 0), "point probes"),
                                  (lambda: eng.set_mean(10), lambda: eng.set_mean(0), "mean fields"),
                                  (lambda: eng.set_field_frames(10, 2), lambda: eng.set_field_frames(0), "field frames"),
                                  (lambda: eng.set_forces(10, 4), lambda: eng.set_forces(0), "obstacle forces"),
                                  (lambda: eng.set_stats(10, 4), lambda: eng.set_stats(0), "lattice statistics")):
            arm()
            with pytest.raises(lbm.LbmError, match="lbm_set_residual: %s are armed" % name):
                eng.set_residual(10, 4)
            disarm()
            eng.set_residual(10, 4)
            with pytest.raises(lbm.LbmError, match=r"velocity residuals are armed \(lbm_set_residual\)"):
                arm()
            eng.set_residual(0)
        eng.set_residual(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_run_until: velocity residuals are armed"):
            eng.run_until(100, 10)
        assert eng.info()["steps_done"] == 0
    with lbm.Batch([p, p], [ob, ob], [cells, cells]) as batch:
        with pytest.raises(lbm.LbmError, match="lbm_set_residual: not available on a member of a batch"):
            batch.member(0).set_residual(10, 4)
    # a rank context (one rank, host message passing that is never called)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_set_residual: not available in a multi-process"):
            eng.set_residual(10, 4)


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_residual: the context runs the %s halo mode" % mode):
                eng.set_residual(10, 4)
        eng.set_halo_mode("sync")
        eng.set_residual(10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match=r"lbm_set_halo_mode: velocity residuals are armed \(lbm_set_residual\)"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0


# ---- batches --------------------------------------------------------------------------------------------------------------
def run_batch(lbm, params, obstacles, cells, calls, every, capacity=0, unarmed_first=0):
    """`unarmed_first` steps, then residuals armed, then `calls`, drained after each:
    ([(lattice, av_vels) per member], steps, rows [n, members], info)"""
    steps, rows = [], []
    with lbm.Batch(params, obstacles, cells) as batch:
        if unarmed_first:
            batch.run(unarmed_first)
        batch.set_residual(every, capacity or 1 + sum(calls) // every)
        for n in calls:
            batch.run(n)
            s, r = batch.residuals()
            steps.append(s)
            rows.append(r)
        info = batch.info()
        total = unarmed_first + sum(calls)
        assert info["steps_done"] == total
        members = [(batch.member(i).cells(), batch.member(i).av_vels(total)) for i in range(len(params))]
    return members, np.concatenate(steps), np.concatenate(rows), info


def assert_members_equal_engines(lbm, params, obstacles, cells, calls, every, got, unarmed_first=0):
    members, steps, rows, _ = got
    assert rows.shape == (len(steps), len(params)) and rows.dtype == lbm.RESIDUAL_DTYPE
    for i, p in enumerate(params):
        lattice, av, e_steps, e_rows, _ = run_engine(lbm, p, obstacles[i], cells[i], calls, every, unarmed_first=unarmed_first)
        assert steps.tolist() == e_steps.tolist(), i
        assert np.ascontiguousarray(rows[:, i]).tobytes() == e_rows.tobytes(), f"member {i}: rows differ from Engine.set_residual's"
        assert same(members[i][0], lattice), f"member {i}: lattice"
        assert same(members[i][1], av), f"member {i}: av_vels"


def test_batch_of_three_small_members(lbm, oracle):
    """3 members of 16 x 8 with their own omega, accel and obstacles (no resident shape: the member table is made at
    arming), armed after 3 steps; member 1 also against the model"""
    params, obstacles, cells = random_members(lbm, 16, 8, 3, seed=40)
    obstacles = [ob.copy() for ob in obstacles]
    obstacles[2][:] = 0
    obstacles[2][3:5, 6:8] = 1
    assert len({(p.omega, p.accel) for p in params}) == 3 and len({ob.tobytes() for ob in obstacles}) == 3
    calls, every = [5, 9], 4
    got = run_batch(lbm, params, obstacles, cells, calls, every, unarmed_first=3)
    members, steps, rows, info = got
    assert steps.tolist() == [4, 8, 12, 16] and np.all(rows["span"] == np.array([[2], [4], [4], [4]]))
    assert_members_equal_engines(lbm, params, obstacles, cells, calls, every, got, unarmed_first=3)
    start = cells[1].copy()
    oracle.run(params[1], start, obstacles[1], 3)
    ref, want = residual_model.oracle_rows(oracle, params[1], obstacles[1], start, 3, sum(calls), every)
    assert_rows(steps, rows[:, 1], want)
    assert same(members[1][0], ref)
    assert len({rows[-1, i]["sum_du_sq"] for i in range(3)}) == 3


def test_batch_of_eight_resident_members(lbm, monkeypatch):
    """8 members of 128 x 16; the calls straddle resident_min_steps = 8: the sub-calls of 10 steps run batched, the
    shorter ones advance the members one after another on the per-pass kernels"""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "8")
    params, obstacles, cells = random_members(lbm, 128, 16, 8, seed=77)
    calls, every = [1, 23, 7], 10
    got = run_batch(lbm, params, obstacles, cells, calls, every)
    assert got[3]["resident_steps"] > 0 and got[1].tolist() == [0, 10, 20, 30]
    assert got[2]["span"][:, 0].tolist() == [1, 10, 10, 10] and np.all(got[2]["nonfinite"] == 0)
    assert_members_equal_engines(lbm, params, obstacles, cells, calls, every, got)


def test_batch_refusals_and_a_run_without_room(lbm):
    params, obstacles, cells = random_members(lbm, 128, 16, 3, seed=31)
    with lbm.Batch(params, obstacles, cells) as batch:
        lib, h = batch.lib, batch.handle
        done = lambda: [batch.member(i).info()["steps_done"] for i in range(3)] + [batch.info()["steps_done"]]  # noqa: E731
        for every, cap, msg in ((-1, 4, "negative interval -1"), (1, 0, "capacity 0, at least one row"), (1, -2, "capacity -2"),
                                (1, 4473925, "a ring of 4473925 rows of 3 members is 2.00 GiB, 2 GiB or more")):
            assert lib.lbm_batch_set_residual(h, every, cap) != 0
            assert lib.lbm_last_error().decode().startswith("lbm_batch_set_residual: ") and msg in lib.lbm_last_error().decode()
        batch.set_residual(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run: 25 steps would record 3 rows.*holds 2.*lbm_batch_read_residual"):
            batch.run(25)                    # rows at 0, 10, 20
        assert done() == [0, 0, 0, 0]        # a run without room moves no member
        batch.run(3)
        # the member-level setters and the batch's other kinds, while the batch's residuals are armed
        m = batch.member(2)
        for arm in (lambda: m.set_frames(10, 2), lambda: m.set_probes([(1, 1)], 1, 4), lambda: m.set_mean(10),
                    lambda: m.set_field_frames(10, 2)):
            with pytest.raises(lbm.LbmError, match=r"this batch has velocity residuals armed \(lbm_batch_set_residual\)"):
                arm()
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_forces: this batch has velocity residuals armed \(lbm_batch_set_residual\)"):
            batch.set_forces(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_stats: this batch has velocity residuals armed \(lbm_batch_set_residual\)"):
            batch.set_stats(10, 4)
        batch.set_forces(0)                                             # disarming the others leaves the residuals alone
        batch.set_stats(0)
        with pytest.raises(lbm.LbmError, match="lbm_set_residual: not available on a member of a batch"):
            batch.member(0).set_residual(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_run_until: velocity residuals are armed \(lbm_batch_set_residual\)"):
            batch.run_until(100, 10)
        assert done() == [3, 3, 3, 3]
        batch.run(8)
        steps, rows = batch.residuals()
        assert steps.tolist() == [0, 10] and rows.shape == (2, 3) and rows["span"][:, 1].tolist() == [1, 10]
        batch.set_residual(0)
        # the other way round: a member with a recorder of its own, the batch's forces, the batch's statistics
        m.set_mean(10)
        with pytest.raises(lbm.LbmError, match="lbm_batch_set_residual: member 2 has mean fields armed"):
            batch.set_residual(10, 4)
        m.set_mean(0)
        batch.set_forces(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_residual: this batch has obstacle forces armed \(lbm_batch_set_forces\)"):
            batch.set_residual(10, 4)
        batch.set_residual(0)                                           # ... and leaves the forces alone
        batch.run(10)
        assert batch.forces()[0].tolist() == [20]
        batch.set_forces(0)
        batch.set_stats(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_residual: this batch has lattice statistics armed \(lbm_batch_set_stats\)"):
            batch.set_residual(10, 4)
        batch.set_stats(0)
        batch.set_residual(10, 4)
        batch.run(10)
        steps, rows = batch.residuals()
        assert steps.tolist() == [30] and np.all(rows["span"] == 10)     # armed after 21 steps: 31 - 21
