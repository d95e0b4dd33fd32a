"""Line profiles (lbm_set_profiles / Engine.set_profiles): after every global timestep tt with tt % every == 0 one record
of per-row lines (sums along x) and per-column lines (sums along y).  Every line of every record is compared BIT FOR BIT
with the numpy model (tests/profile_model.py) over the oracle's lattice of that step: the sums are exact and rounded
once, so every kernel path, call splitting, slab count and batch membership gives the same bits; recording never changes
the lattice, and av_vels equals that of the same run issued as calls split at the sample steps."""
import ctypes

import numpy as np
import pytest

import edge_lattice as el
import profile_model
from test_gpu_batch import random_members
from test_gpu_forces import FAMILIES, RESIDENT_SHAPES, Shared, bits, small
from test_gpu_parity import random_case
from test_gpu_stats import split_calls

pytestmark = pytest.mark.gpu

# profile_rows: a wave owns a row, its lanes stride along x V cells at a time (V = 4 where nx % 4 == 0, else 1)
WAVE, BLOCK = 64, 256                   # lanes per wave and per workgroup: a workgroup of profile_rows takes BLOCK / WAVE = 4 rows
# profile_columns: a workgroup owns COLUMNS columns (a lane a column) of a band of rows, its 4 waves interleaving the rows
COLUMNS, MIN_BAND, TARGET_GROUPS = 64, 8, 1024


def vector(nx):
    return 4 if nx % 4 == 0 else 1


def band_rows(rows, nx):
    """the band rule of profile_columns: about TARGET_GROUPS workgroups, a band no shorter than MIN_BAND rows"""
    col_groups = -(-nx // COLUMNS)
    bands = max(1, TARGET_GROUPS // col_groups)
    return max(MIN_BAND, -(-rows // bands))


AXES = {1: ("rows",), 2: ("columns",), 3: ("rows", "columns")}


def run_engine(lbm, p, ob, cells, calls, every=0, capacity=0, axes=3, n_gpus=1, unarmed_first=0, tiled=False):
    """`unarmed_first` steps, then profiles armed, then `calls`, drained after each: (lattice, av_vels, steps, {axis: lines [n][..]}, info)"""
    steps, recs = [], {k: [] for k in AXES[axes]}
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus, tiled=tiled) as eng:
        if unarmed_first:
            eng.run(unarmed_first)
        if every:
            eng.set_profiles(every, capacity or 1 + sum(calls) // every, axes)
        for n in calls:
            eng.run(n)
            if every:
                s, r = eng.profiles()
                assert sorted(r) == sorted(AXES[axes])
                steps.append(s)
                for k in r:
                    recs[k].append(r[k])
        total = unarmed_first + sum(calls)
        lines = {k: np.concatenate(v) for k, v in recs.items() if v}
        return eng.cells(), eng.av_vels(total), np.concatenate(steps) if steps else np.zeros(0, np.int32), lines, eng.info()


def assert_records(steps, lines, want, shape=None):
    """want: {tt: record of profile_model.record}"""
    assert steps.tolist() == sorted(want)
    for k, v in lines.items():
        assert v.shape[0] == len(steps)
        if shape:
            assert v.shape[1] == (shape[0] if k == "rows" else shape[1])
        for i, tt in enumerate(steps.tolist()):
            diff = profile_model.same_bits(v[i], want[tt][k])
            print("step", tt, k, "lines", len(v[i]), "first", v[i][0], "differs:", diff[:4])
            assert not diff, (tt, k, diff[:8])


def check(lbm, oracle, p, ob, cells, calls, every, unarmed_first=0, n_gpus=1, want=None, ref=None, tiled_ob=None, axes=3):
    """armed run against the model on the oracle's lattices; lattice and av_vels against the unarmed run split at the sample steps"""
    if want is None:
        start = cells.copy()
        oracle.run(p, start, ob, unarmed_first)
        ref, want = profile_model.oracle_records(oracle, p, ob, start, unarmed_first, sum(calls), every)
    engine_ob = ob if tiled_ob is None else tiled_ob
    got, av, steps, lines, info = run_engine(lbm, p, engine_ob, cells, calls, every, axes=axes, n_gpus=n_gpus, unarmed_first=unarmed_first,
                                             tiled=tiled_ob is not None)
    assert_records(steps, lines, want, (p.ny, p.nx))
    assert np.array_equal(bits(ref), bits(got)), "recording changed the lattice"
    base, base_av, _, _, _ = run_engine(lbm, p, engine_ob, cells, split_calls(unarmed_first, calls, every), n_gpus=n_gpus,
                                        tiled=tiled_ob is not None)
    assert np.array_equal(bits(base), bits(got))
    assert np.array_equal(bits(base_av), bits(av)), "recording changed av_vels"
    return steps, lines, info


# ---- shapes: the smallest at which the two kernels can go wrong -----------------------------------------------------------
def test_smallest_case(lbm, oracle):
    p, ob, cells = small(lbm, 16, 8)
    ob[3:5, 6:8] = 1
    steps, lines, _ = check(lbm, oracle, p, ob, cells, [5, 7], 1)
    assert len(steps) == 12 and lines["rows"].shape == (12, 8) and lines["columns"].shape == (12, 16)
    last = lines["rows"][-1]
    assert last["fluid"].tolist() == [16, 16, 16, 14, 14, 16, 16, 16] and np.all(last["nonfinite"] == 0) and last["sum_jx"][6] > 0.0
    assert lines["columns"][-1]["fluid"].tolist() == [8] * 6 + [6, 6] + [8] * 8


ROW_EDGES = [(63, 5), (64, 5), (65, 5), (252, 4), (256, 4), (260, 4), (21, 3), (130, 6)]
COLUMN_EDGES = ([(nx, 5) for nx in (COLUMNS - 1, COLUMNS, COLUMNS + 1, 2 * COLUMNS - 1, 2 * COLUMNS, 2 * COLUMNS + 1)] +
                [(20, ny) for ny in (3, MIN_BAND - 1, MIN_BAND, MIN_BAND + 1, 2 * MIN_BAND + 3)])


@pytest.mark.parametrize("nx,ny", sorted(set(ROW_EDGES + COLUMN_EDGES)))
def test_wave_group_and_band_edges(lbm, oracle, nx, ny):
    """profile_rows: nx just below, at and above one stride of a wave (63 / 64 / 65 cells at one cell per lane, 252 / 256 /
    260 at four) and widths that are no multiple of 4, which leave pitch padding behind every row; profile_columns: nx
    just below, at and above one and two column groups, ny of 3, one less than a band, a band, one more and no multiple of
    it.  An obstacle in row 1, the last owned cell blocked."""
    assert band_rows(ny, nx) == MIN_BAND
    p, ob, cells = small(lbm, nx, ny, nx + ny)
    ob[1, 2:4] = 1
    ob[ny - 1, nx - 1] = 1
    steps, lines, _ = check(lbm, oracle, p, ob, cells, [3], 2)
    assert lines["rows"][-1]["fluid"][1] == nx - 2 and lines["columns"][-1]["fluid"][nx - 1] == ny - 1


@pytest.mark.parametrize("nx,ny", [(1024, 1024), (1030, 512)])
def test_every_wave_and_workgroup_loops(lbm, oracle, nx, ny):
    """every wave of profile_rows strides along its row more than once (1024 / 4 = 256 units and 1030 units for 64
    lanes), every wave of profile_columns walks more than one row of its band, and the bands of a column meet in atomics"""
    assert nx // vector(nx) >= 2 * WAVE
    rows_per_band = band_rows(ny, nx)
    assert rows_per_band >= 2 * (BLOCK // WAVE) and -(-ny // rows_per_band) >= 2
    p, ob, cells = random_case(lbm, nx, ny, 11, walls=False)
    check(lbm, oracle, p, ob, cells, [1], 1)


def test_every_binade(lbm, oracle):
    """the lattice of tests/edge_lattice.py: populations over all the exponents the collision guards allow, so the limbs
    of every accumulator are used"""
    p, ob, cells, _ = el.build(lbm, 256, 40)
    steps, lines, _ = check(lbm, oracle, p, ob, cells, [el.STEPS], 1)
    assert np.all(lines["rows"]["nonfinite"] == 0) and np.all(lines["columns"]["nonfinite"] == 0)


# ---- blocked lines and non-finite cells -----------------------------------------------------------------------------------
def test_fully_blocked_row_and_column(lbm, oracle):
    p, ob, cells = small(lbm, 32, 8, 5)
    ob[2, :] = 1
    ob[:, 9] = 1
    steps, lines, _ = check(lbm, oracle, p, ob, cells, [3], 1)
    for line in list(lines["rows"][:, 2]) + list(lines["columns"][:, 9]):
        assert line["fluid"] == 0 and line["nonfinite"] == 0
        for k in profile_model.SUMS:
            assert line[k] == 0.0 and not np.signbit(line[k])
    assert np.all(lines["rows"]["fluid"][:, [0, 1, 3]] == 31) and np.all(lines["columns"]["fluid"][:, 8] == 7)


def test_nonfinite_cells_are_counted_on_their_lines_and_left_out(lbm, oracle):
    p, ob, cells = small(lbm, 32, 8, 5)
    ob[3:5, 6:8] = 1
    cells[6, 20, 3] = np.inf                              # a fluid cell
    cells[3, 7, 2] = np.nan                               # a blocked cell: counted nowhere
    ref, want = profile_model.oracle_records(oracle, p, ob, cells, 0, 3, 1)
    bad0 = [r["nonfinite"] for r in want[0]["rows"]]
    assert sum(bad0) >= 1 and sum(r["nonfinite"] for r in want[2]["rows"]) > sum(bad0) and bad0[0] == 0
    for calls, every in (([1], 1), ([3], 2)):
        got, _, steps, lines, _ = run_engine(lbm, p, ob, cells, calls, every)
        assert_records(steps, lines, {tt: want[tt] for tt in steps.tolist()})
        for v in lines.values():
            assert all(np.all(np.isfinite(v[k])) for k in profile_model.SUMS)
    assert steps.tolist() == [0, 2]
    assert lines["rows"]["nonfinite"][0].tolist() == bad0
    assert lines["rows"]["nonfinite"][0].sum() == lines["columns"]["nonfinite"][0].sum()
    # the lattice is the oracle's: the same cells are NaN (a NaN's payload is not the arithmetic's to keep), the rest bit for bit
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(got)) and np.array_equal(bits(ref)[~nan], bits(got)[~nan])


def test_all_nan_lattice(lbm):
    p, ob, cells = small(lbm, 20, 6)
    ob[2, 3] = 1
    cells[:] = np.nan
    _, _, steps, lines, _ = run_engine(lbm, p, ob, cells, [2], 1)
    assert lines["rows"]["nonfinite"][0].tolist() == [20, 20, 19, 20, 20, 20] and lines["columns"]["nonfinite"][1].tolist() == [6] * 3 + [5] + [6] * 16
    for v in lines.values():
        assert np.all(v["fluid"] == 0)
        for k in profile_model.SUMS:
            assert np.all(v[k] == 0.0) and not np.any(np.signbit(v[k]))


# ---- axes -----------------------------------------------------------------------------------------------------------------
def test_each_axis_alone_is_its_half_of_both(lbm, oracle):
    p, ob, cells = small(lbm, 68, 11, 3)
    ob[4:6, 30:33] = 1
    _, both, _ = check(lbm, oracle, p, ob, cells, [4, 3], 2, axes=3)
    for axes, key in ((1, "rows"), (2, "columns")):
        steps, lines, _ = check(lbm, oracle, p, ob, cells, [4, 3], 2, axes=axes)
        assert list(lines) == [key] and steps.tolist() == [0, 2, 4, 6]
        assert lines[key].tobytes() == both[key].tobytes()


# ---- paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_steps", ["1", "3"])
@pytest.mark.parametrize("shape", list(RESIDENT_SHAPES))
def test_resident_shapes(lbm, oracle, monkeypatch, shape, min_steps):
    nx, ny, env = RESIDENT_SHAPES[shape]
    calls, every = [1, 2, 19, 5], 3

    def make():
        p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
        ref, want = profile_model.oracle_records(oracle, p, ob, cells, 0, sum(calls), every)
        return p, ob, cells, ref, want
    p, ob, cells, ref, want = Shared.get(("profiles", shape), make)
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", min_steps)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    steps, lines, info = check(lbm, oracle, p, ob, cells, calls, every, want=want, ref=ref)
    assert info["resident_steps"] > 0 and len(steps) == 9


def per_pass_case(lbm, oracle):
    """128 x 96; armed after 5 steps; the oracle's records of every step from there"""
    def make():
        p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
        start = cells.copy()
        oracle.run(p, start, ob, 5)
        ref, all_steps = profile_model.oracle_records(oracle, p, ob, start, 5, 63, 1)
        return p, ob, cells, ref, all_steps
    return Shared.get(("profiles", "per-pass"), make)


@pytest.mark.parametrize("every", [1, 3, 4, 7])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_pass_families(lbm, oracle, monkeypatch, family, every):
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % every == 0}
    steps, lines, info = check(lbm, oracle, p, ob, cells, [23, 40], every, unarmed_first=5, want=want, ref=ref)
    assert info["resident_steps"] == 0 and steps[0] == (5 + every - 1) // every * every


def test_one_call_against_ragged_split_calls(lbm, oracle):
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
    whole = run_engine(lbm, p, ob, cells, [63], 4, unarmed_first=5)
    ragged = run_engine(lbm, p, ob, cells, [1, 2, 13, 4, 30, 1, 12], 4, unarmed_first=5)
    assert whole[2].tolist() == ragged[2].tolist() == [tt for tt in range(5, 68) if tt % 4 == 0]
    for k in ("rows", "columns"):
        assert whole[3][k].tobytes() == ragged[3][k].tobytes()
    assert np.array_equal(bits(whole[0]), bits(ragged[0])) and np.array_equal(bits(whole[0]), bits(ref))
    assert_records(whole[2], whole[3], {tt: v for tt, v in all_steps.items() if tt % 4 == 0})


# ---- slabs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny", [16, 64])
def test_slabs(lbm, oracle, monkeypatch, ny):
    """1, 2 and 3 slabs (of 6, 5 and 5 rows on ny = 16): a row line comes from the slab that owns the row, a column's limbs
    are added over the slabs before the one rounding -- the records of one slab, bit for bit"""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = small(lbm, 72, ny, ny)
    ob[1, 2:4] = ob[ny - 1, 71] = ob[5:7, 40] = 1
    ref, want = profile_model.oracle_records(oracle, p, ob, cells, 0, 7, 2)
    seen = []
    for n_gpus in (1, 2, 3):
        steps, lines, info = check(lbm, oracle, p, ob, cells, [4, 3], 2, n_gpus=n_gpus, want=want, ref=ref)
        assert info["n_slabs"] == n_gpus
        seen.append(lines)
    assert [lbm.partition_rows(16, 3, s)[1] for s in range(3)] == [6, 5, 5]
    for other in seen[1:]:
        for k in ("rows", "columns"):
            assert other[k].tobytes() == seen[0][k].tobytes()


def test_tiled_context(lbm, oracle):
    p, tile, _ = small(lbm, 32, 16)
    tile[0, 0] = tile[15, 31] = tile[5:8, 9:12] = 1
    p = lbm.Params(128, 48, 400, 10, 0.1, 0.005, 1.85)
    ob = np.tile(tile, (3, 4))
    cells = small(lbm, 128, 48, 8)[2]
    ref, want = profile_model.oracle_records(oracle, p, ob, cells, 0, 9, 2)
    expanded = check(lbm, oracle, p, ob, cells, [9], 2, want=want, ref=ref)[1]
    for n_gpus in (1, 2):
        _, lines, info = check(lbm, oracle, p, ob, cells, [9], 2, n_gpus=n_gpus, want=want, ref=ref, tiled_ob=tile)
        assert info["n_slabs"] == n_gpus
        for k in ("rows", "columns"):
            assert lines[k].tobytes() == expanded[k].tobytes()


# ---- batches --------------------------------------------------------------------------------------------------------------
def run_batch(lbm, params, obstacles, cells, calls, every, axes=3, capacity=0):
    steps, recs = [], {k: [] for k in AXES[axes]}
    with lbm.Batch(params, obstacles, cells) as batch:
        batch.set_profiles(every, capacity or 1 + sum(calls) // every, axes)
        for n in calls:
            batch.run(n)
            s, r = batch.profiles()
            steps.append(s)
            for k in r:
                recs[k].append(r[k])
        info = batch.info()
        total = sum(calls)
        assert info["steps_done"] == total
        members = [(batch.member(i).cells(), batch.member(i).av_vels(total)) for i in range(len(params))]
    return members, np.concatenate(steps), {k: np.concatenate(v) for k, v in recs.items()}, info


@pytest.mark.parametrize("nx,ny,resident", [(128, 128, True), (100, 40, False), (102, 12, False)])
def test_batch_members_equal_engines_and_model(lbm, oracle, monkeypatch, nx, ny, resident):
    """three members that differ in omega, acceleration and obstacle map, on a resident shape (the calls straddle
    resident_min_steps = 8) and on two that are not (100 x 40: four cells per lane; 102 x 12: one)"""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "8")
    params, obstacles, cells = random_members(lbm, nx, ny, 3, nx + 3)
    assert len({(p.omega, p.accel) for p in params}) == 3
    calls, every = ([1, 23, 7], 10) if resident else ([12, 9], 4)
    members, steps, lines, info = run_batch(lbm, params, obstacles, cells, calls, every)
    assert (info["resident_steps"] > 0) == resident
    assert lines["rows"].shape == (len(steps), 3, ny) and lines["columns"].shape == (len(steps), 3, nx)
    for i, p in enumerate(params):
        lattice, av, e_steps, e_lines, _ = run_engine(lbm, p, obstacles[i], cells[i], calls, every)
        assert steps.tolist() == e_steps.tolist()
        for k in ("rows", "columns"):
            assert np.ascontiguousarray(lines[k][:, i]).tobytes() == e_lines[k].tobytes(), f"member {i}: {k} differ from Engine.set_profiles'"
        assert np.array_equal(bits(members[i][0]), bits(lattice)) and np.array_equal(bits(members[i][1]), bits(av)), f"member {i}"
    i = 1
    ref, want = profile_model.oracle_records(oracle, params[i], obstacles[i], cells[i], 0, sum(calls), every)
    assert_records(steps, {k: v[:, i] for k, v in lines.items()}, want, (ny, nx))
    assert np.array_equal(bits(members[i][0]), bits(ref))


def test_batch_ring_and_refusals(lbm):
    params, obstacles, cells = random_members(lbm, 128, 16, 3, 23)
    with lbm.Batch(params, obstacles, cells) as batch:
        lib, h = batch.lib, batch.handle
        n = lib.lbm_batch_read_profiles
        done = lambda: [batch.member(i).info()["steps_done"] for i in range(3)] + [batch.info()["steps_done"]]  # noqa: E731
        member_bytes = (16 + 128) * 384
        too_many = -(-2 ** 31 // (3 * member_bytes))
        for every, cap, axes, msg in ((-1, 4, 3, "negative interval -1"), (1, 0, 3, "capacity 0, at least one record"), (1, 4, 0, "axes 0"),
                                      (1, 4, 4, "axes 4"), (1, too_many, 3, "a ring of %d records of 3 members is 2.00 GiB, 2 GiB or more" % too_many)):
            assert lib.lbm_batch_set_profiles(h, every, cap, axes) != 0
            assert lib.lbm_last_error().decode().startswith("lbm_batch_set_profiles: ") and msg in lib.lbm_last_error().decode()
        batch.set_profiles(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run: 25 steps would record 3 records.*holds 2.*lbm_batch_read_profiles"):
            batch.run(25)                    # records at 0, 10, 20
        assert done() == [0, 0, 0, 0]        # a run without room moves no member
        batch.run(15)
        with pytest.raises(lbm.LbmError, match="2 records are waiting"):
            batch.run(10)
        assert done() == [15, 15, 15, 15]
        waiting = ctypes.c_int(-1)
        assert n(h, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2       # the query form drains nothing
        steps, first = batch.profiles(1)
        assert steps.tolist() == [0] and first["rows"].shape == (1, 3, 16) and first["columns"].shape == (1, 3, 128)
        batch.run(10)
        assert batch.profiles()[0].tolist() == [10, 20]
        # the member-level setters and the three other batch kinds, while the batch's profiles are armed
        m = batch.member(2)
        for arm in (lambda: m.set_frames(10, 2), lambda: m.set_probes([(1, 1)], 1, 4), lambda: m.set_mean(10), lambda: m.set_field_frames(10, 2)):
            with pytest.raises(lbm.LbmError, match=r"this batch has line profiles armed \(lbm_batch_set_profiles\)"):
                arm()
        for name, arm, off in (("forces", lambda: batch.set_forces(10, 4), lambda: batch.set_forces(0)),
                               ("stats", lambda: batch.set_stats(10, 4), lambda: batch.set_stats(0)),
                               ("residual", lambda: batch.set_residual(10, 4), lambda: batch.set_residual(0))):
            with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_%s: this batch has line profiles armed \(lbm_batch_set_profiles\)" % name):
                arm()
            off()                                                       # disarming another kind leaves the profiles alone
        with pytest.raises(lbm.LbmError, match="lbm_set_profiles: not available on a member of a batch"):
            m.set_profiles(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_run_until: line profiles are armed \(lbm_batch_set_profiles\)"):
            batch.run_until(100, 10)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_run_until_residual: line profiles are armed"):
            batch.run_until_residual(100, 10, 1e-3)
        batch.run(6)                         # 30
        batch.set_profiles(10, 2, 1)         # re-arming discards the unread record
        assert batch.profiles()[0].size == 0
        batch.run(10)                        # 40
        steps, lines = batch.profiles()
        assert steps.tolist() == [40] and list(lines) == ["rows"]
        batch.set_profiles(0)                # disarms and frees
        # the other way round
        m.set_mean(10)
        with pytest.raises(lbm.LbmError, match="lbm_batch_set_profiles: member 2 has mean fields armed"):
            batch.set_profiles(10, 4)
        m.set_mean(0)
        batch.set_stats(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_profiles: this batch has lattice statistics armed \(lbm_batch_set_stats\)"):
            batch.set_profiles(10, 4)
        batch.set_profiles(0)                # ... and leaves the statistics alone
        batch.run(10)
        assert batch.stats()[0].tolist() == [50]
        assert done() == [51, 51, 51, 51]


# ---- the ring -------------------------------------------------------------------------------------------------------------
def test_ring_overflow_drain_order_query_rearm_disarm(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        n = eng.lib.lbm_read_profiles
        eng.set_profiles(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_run: 25 steps would record 3 records.*holds 2.*lbm_read_profiles"):
            eng.run(25)                      # records at 0, 10, 20
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match="2 records are waiting"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        waiting = ctypes.c_int(-1)
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # the query form
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # ... drains nothing
        steps, first = eng.profiles(1)
        assert steps.tolist() == [0] and first["rows"].shape == (1, 128) and first["columns"].shape == (1, 128)      # oldest first
        eng.run(10)                          # 20 goes into the slot that 0 left
        steps, lines = eng.profiles()
        rows = lines["rows"]
        assert steps.tolist() == [10, 20] and rows[0]["sum_jx"][5] != rows[1]["sum_jx"][5] and first["rows"][0]["sum_jx"][5] != rows[1]["sum_jx"][5]
        eng.run(6)                           # 30
        eng.set_profiles(10, 2, ("columns",))   # re-arming discards the unread record
        assert eng.profiles()[0].size == 0
        eng.run(10)                          # 40
        steps, lines = eng.profiles()
        assert steps.tolist() == [40] and list(lines) == ["columns"] and lines["columns"].shape == (1, 128)
        eng.set_profiles(0)                  # disarms and frees
        eng.run(30)
        steps, lines = eng.profiles()
        assert steps.size == 0 and lines == {}
        assert eng.info()["steps_done"] == 71


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 4, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        too_many, too_many_rows = -(-2 ** 31 // (256 * 384)), -(-2 ** 31 // (128 * 384))     # the first capacities of 2 GiB or more
        for every, cap, axes, msg in ((-1, 4, 3, "lbm_set_profiles: negative interval -1"), (1, 0, 3, "lbm_set_profiles: capacity 0, at least one record"),
                                      (1, -2, 3, "lbm_set_profiles: capacity -2"), (1, 4, 0, "lbm_set_profiles: axes 0"), (1, 4, 4, "lbm_set_profiles: axes 4"),
                                      (1, 4, -1, "lbm_set_profiles: axes -1"),
                                      (1, too_many, 3, "lbm_set_profiles: a ring of %d records is 2 GiB or more (98304 bytes per record and slab)" % too_many),
                                      (1, too_many_rows, 1, "lbm_set_profiles: a ring of %d records is 2 GiB or more (49152 bytes" % too_many_rows)):
            assert eng.lib.lbm_set_profiles(eng.handle, every, cap, axes) != 0
            assert msg in eng.lib.lbm_last_error().decode()
        assert eng.info()["steps_done"] == 0
        # one recorder per context, both directions
        for arm, disarm, name in ((lambda: eng.set_frames(10, 2), lambda: eng.set_frames(0), "animation frames"),
                                  (lambda: eng.set_probes([(1, 1)], 1, 4), lambda: eng.set_probes([], 0), "point probes"),
                                  (lambda: eng.set_mean(10), lambda: eng.set_mean(0), "mean fields"),
                                  (lambda: eng.set_field_frames(10, 2), lambda: eng.set_field_frames(0), "field frames"),
                                  (lambda: eng.set_forces(10, 4), lambda: eng.set_forces(0), "obstacle forces"),
                                  (lambda: eng.set_stats(10, 4), lambda: eng.set_stats(0), "lattice statistics"),
                                  (lambda: eng.set_residual(10, 4), lambda: eng.set_residual(0), "velocity residuals")):
            arm()
            with pytest.raises(lbm.LbmError, match="lbm_set_profiles: %s are armed" % name):
                eng.set_profiles(10, 4)
            disarm()
            eng.set_profiles(10, 4)
            with pytest.raises(lbm.LbmError, match=r"line profiles are armed \(lbm_set_profiles\)"):
                arm()
            eng.set_profiles(0)
        eng.set_profiles(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_run_until: line profiles are armed"):
            eng.run_until(100, 10)
        with pytest.raises(lbm.LbmError, match="lbm_run_until_residual: line profiles are armed"):
            eng.run_until_residual(100, 10, 1e-3)
        assert eng.info()["steps_done"] == 0
    # a rank context (one rank, host message passing that is never called)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_set_profiles: not available in a multi-process"):
            eng.set_profiles(10, 4)


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_profiles: the context runs the %s halo mode" % mode):
                eng.set_profiles(10, 4)
        eng.set_halo_mode("sync")
        eng.set_profiles(10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match=r"lbm_set_halo_mode: line profiles are armed \(lbm_set_profiles\)"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0
