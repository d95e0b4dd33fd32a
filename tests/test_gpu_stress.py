"""Stress fields and stress rows (lbm_read_stress / Engine.stress, lbm_set_stress / Engine.set_stress and the batch
twins): the three planes of the kinematic non-equilibrium stress of the stored lattice and one row of its whole-lattice
sums after every global timestep tt with tt % every == 0.  Every row and every plane is compared BIT FOR BIT with the
numpy model (tests/stress_model.py) over the oracle's lattice of that step: the sums are exact and rounded once, the
maximum does not depend on order, so every kernel path, call splitting and slab count gives the same bits; recording
never changes the lattice, and av_vels equals that of the same run issued as calls split at the sample steps.  Unless a
case says otherwise the model's rows have nonfinite == 0, asserted, so that no case passes by leaving cells out."""
import math

import numpy as np
import pytest

import edge_lattice as el
import stress_model as sm
from test_gpu_batch import random_members
from test_gpu_forces import FAMILIES, RESIDENT_SHAPES, Shared, bits, small
from test_gpu_parity import random_case
from test_gpu_stats import BLOCK, MAX_GROUPS, split_calls

pytestmark = pytest.mark.gpu


def run_engine(lbm, p, ob, cells, calls, every=0, capacity=0, n_gpus=1, unarmed_first=0, tiled=False, fields=False):
    """`unarmed_first` steps, then the stress armed, then `calls`, drained after each:
    (lattice, av_vels, steps, rows, info, [stress() after each call] if fields)"""
    steps, rows, ts = [], [], []
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus, tiled=tiled) as eng:
        if unarmed_first:
            eng.run(unarmed_first)
        if every:
            eng.set_stress(every, capacity or 1 + sum(calls) // every)
        for n in calls:
            eng.run(n)
            if fields:
                ts.append(eng.stress())
            if every:
                s, r = eng.stress_rows()
                steps.append(s)
                rows.append(r)
        total = unarmed_first + sum(calls)
        return (eng.cells(), eng.av_vels(total), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(rows) if rows else np.zeros(0, lbm.STRESS_DTYPE), eng.info(), ts)


def assert_rows(steps, rows, want, clean=True):
    """want: {tt: row of stress_model.row}"""
    assert steps.tolist() == sorted(want)
    for tt, row in zip(steps.tolist(), rows):
        diff = sm.same_bits(row, want[tt])
        print("step", tt, {k: row[k] for k in sm.FIELDS}, "differs:", diff)
        assert not diff, (tt, diff)
        if clean:
            assert want[tt]["nonfinite"] == 0 and want[tt]["fluid"] > 0 and want[tt]["max_q"] > 0


def assert_fields(got, want, what):
    assert sorted(got) == ["txx", "txy", "tyy"] and all(v.dtype == np.float32 for v in got.values())
    assert sm.same_fields(got, want) == [], what


def call_ends(unarmed_first, calls):
    return [unarmed_first + sum(calls[:i + 1]) - 1 for i in range(len(calls))]


def check(lbm, oracle, p, ob, cells, calls, every, unarmed_first=0, n_gpus=1, want=None, ref=None, fields=None, tiled_ob=None, clean=True):
    """armed run against the model on the oracle's lattices, the planes after every call; lattice and av_vels against the
    unarmed run split at the sample steps"""
    ends = call_ends(unarmed_first, calls)
    if want is None:
        start = cells.copy()
        oracle.run(p, start, ob, unarmed_first)
        ref, want, fields = sm.oracle_rows(oracle, p, ob, start, unarmed_first, sum(calls), every, fields_at=ends)
    engine_ob = ob if tiled_ob is None else tiled_ob
    got, av, steps, rows, info, ts = run_engine(lbm, p, engine_ob, cells, calls, every, n_gpus=n_gpus, unarmed_first=unarmed_first,
                                                tiled=tiled_ob is not None, fields=True)
    assert_rows(steps, rows, want, clean)
    for tt, t in zip(ends, ts):
        assert_fields(t, fields[tt], ("stress() after step", tt))
    assert np.array_equal(bits(ref), bits(got)), "recording changed the lattice"
    base, base_av, _, _, _, _ = run_engine(lbm, p, engine_ob, cells, split_calls(unarmed_first, calls, every), n_gpus=n_gpus,
                                           tiled=tiled_ob is not None)
    assert np.array_equal(bits(base), bits(got))
    assert np.array_equal(bits(base_av), bits(av)), "recording changed av_vels"
    return steps, rows, info


# ---- shapes: the smallest at which stress_gather can go wrong -----------------------------------------------------------
def test_smallest_case(lbm, oracle):
    p, ob, cells = small(lbm, 16, 8)
    ob[3:5, 6:8] = 1
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [5, 7], 1)
    assert len(steps) == 12 and np.all(rows["fluid"] == 124) and np.all(rows["sum_q"] > 0)
    assert rows[-1]["sum_q"] < rows[0]["sum_q"]                         # the random start relaxes


@pytest.mark.parametrize("nx,ny", [(21, 3), (16, 4), (13, 5), (85, 3), (16, 16), (257, 3), (130, 6), (252, 4), (260, 4)])
def test_lane_wave_and_workgroup_edges(lbm, oracle, nx, ny):
    """test_gpu_stats' shapes: cells just below, at and above a wave (63, 64, 65) and a workgroup (255, 256, 771); widths
    that are no multiple of 4 take one cell per lane and leave pitch padding behind every row; 252 x 4 and 260 x 4 put
    the four-cell units just below and above one workgroup's 256.  The last owned cell is blocked: its planes are 0"""
    p, ob, cells = small(lbm, nx, ny, nx + ny)
    ob[1, 2:4] = 1
    ob[ny - 1, nx - 1] = 1
    check(lbm, oracle, p, ob, cells, [3], 2)


@pytest.mark.parametrize("nx,ny", [(1024, 1024), (1030, 512)])
def test_capped_grid_every_workgroup_loops(lbm, oracle, nx, ny):
    """more units than the capped grid has lanes, twice over: every workgroup takes its loop at least twice (four cells
    per lane on 1024 x 1024, one on 1030 x 512)"""
    units = nx * ny // (4 if nx % 4 == 0 else 1)
    assert units >= 2 * MAX_GROUPS * BLOCK
    p, ob, cells = random_case(lbm, nx, ny, 11, walls=False)
    check(lbm, oracle, p, ob, cells, [1], 1)


def test_every_binade(lbm, oracle):
    """the lattice of tests/edge_lattice.py: populations over all the exponents the collision guards allow, so the limbs
    of both accumulators are used"""
    p, ob, cells, _ = el.build(lbm, 256, 40)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [el.STEPS], 1)
    assert np.all(rows["nonfinite"] == 0)


def test_a_reader_chunk_boundary(lbm, oracle):
    """lbm_read_stress stages 16 MiB of a plane at a time: 4096 x 1030 cells are 1024 rows and a chunk of 6, which starts
    at a row of its own (one step; the planes alone, the rows' path has no chunks)"""
    nx, ny = 4096, 1030
    p, ob, cells = random_case(lbm, nx, ny, 5, walls=False)
    ob[1023:1025, 7:9] = 1
    with lbm.Engine(p, ob, cells) as eng:
        got = eng.stress()
    assert_fields(got, sm.field(cells, ob)[0], "two chunks")


# ---- ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_gpus", [1, 2])
def test_ties_take_the_smallest_cell(lbm, oracle, monkeypatch, n_gpus):
    """an open channel from the uniform equilibrium stays x-invariant: a whole row ties and max_x is 0"""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p = lbm.Params(64, 16, 400, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((16, 64), dtype=np.int32)
    ob[[0] if n_gpus == 1 else [4, 8], :] = 1
    steps, rows, info = check(lbm, oracle, p, ob, oracle.init_cells(p), [12], 4, n_gpus=n_gpus)
    assert info["n_slabs"] == n_gpus and np.all(rows["max_x"] == 0) and np.all(rows["max_q"] > 0)


# ---- non-finite cells -----------------------------------------------------------------------------------------------------
def nonfinite_cases(cells):
    nan_fluid, empty, nan_blocked = cells.copy(), cells.copy(), cells.copy()
    nan_fluid[6, 20, 3] = np.nan                          # a NaN population in one fluid cell
    empty[1, 12, :] = 0.0                                 # rho == 0 in one fluid cell: 0 / 0
    nan_blocked[3, 7, 2] = np.nan                         # a NaN in a blocked cell
    return {"nan-fluid": (nan_fluid, 1), "rho-zero": (empty, 1), "nan-blocked": (nan_blocked, 0)}


@pytest.mark.parametrize("which", ["nan-fluid", "rho-zero", "nan-blocked"])
def test_nonfinite_cells_are_counted_and_left_out(lbm, oracle, which):
    """each is counted exactly as the model counts it; sums and the key skip those cells; the planes store them as computed"""
    p, ob, cells = small(lbm, 32, 8, 5)
    ob[3:5, 6:8] = 1
    bad, count = nonfinite_cases(cells)[which]
    now = sm.row(bad, ob)
    assert now["nonfinite"] == count and now["fluid"] == 252 - count
    ref, after, _ = sm.oracle_rows(oracle, p, ob, bad, 0, 2, 1)
    if which == "nan-fluid":                              # the steps spread the NaN (the emptied cell fills up again)
        assert after[1]["nonfinite"] > after[0]["nonfinite"] >= 1
    with lbm.Engine(p, ob, bad) as eng:
        t = eng.stress()
        eng.set_stress(1, 4)
        eng.run(2)
        steps, rows = eng.stress_rows()
        later = eng.stress()
    model_t = sm.field(bad, ob)[0]
    assert sum(int(np.isnan(model_t[k]).sum()) for k in ("txx", "txy", "tyy")) == 3 * count
    assert_fields(t, model_t, which)
    assert_fields(later, sm.field(ref, ob)[0], which + " after two steps")
    assert_rows(steps, rows, after, clean=False)
    # the same lattice without stepping: a row's sums are those of the planes' finite fluid cells
    q = sm.q_of_planes(t["txx"], t["txy"], t["tyy"])
    keep = (ob == 0) & np.isfinite(q)
    assert keep.sum() == now["fluid"] and math.fsum(float(v) for v in q[keep]) == now["sum_q"]


def test_all_nan_lattice(lbm):
    p, ob, cells = small(lbm, 20, 6)
    ob[2, 3] = 1
    cells[:] = np.nan
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_stress(1, 4)
        eng.run(2)
        _, rows = eng.stress_rows()
        t = eng.stress()
    for k in ("txx", "txy", "tyy"):
        assert np.isnan(t[k]).sum() == 119 and t[k][2, 3] == 0 and not np.signbit(t[k][2, 3])
    for r in rows:
        assert r["nonfinite"] == 119 and r["fluid"] == 0 and r["max_q"] == 0 and (r["max_x"], r["max_y"]) == (-1, -1)
        for k in ("sum_q", "sum_txy"):
            assert r[k] == 0.0 and not np.signbit(r[k])


# ---- paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_steps", ["1", "3"])
@pytest.mark.parametrize("shape", list(RESIDENT_SHAPES))
def test_resident_shapes(lbm, oracle, monkeypatch, shape, min_steps):
    """sub-calls above and below resident_min_steps"""
    nx, ny, env = RESIDENT_SHAPES[shape]
    calls, every = [1, 2, 19, 5], 3

    def make():
        p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
        ref, want, fields = sm.oracle_rows(oracle, p, ob, cells, 0, sum(calls), every, fields_at=call_ends(0, calls))
        return p, ob, cells, ref, want, fields
    p, ob, cells, ref, want, fields = Shared.get(("stress", shape), make)
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", min_steps)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    steps, rows, info = check(lbm, oracle, p, ob, cells, calls, every, want=want, ref=ref, fields=fields)
    assert info["resident_steps"] > 0 and len(steps) == 9


def per_pass_case(lbm, oracle):
    """128 x 96; armed after 5 unarmed steps; the oracle's rows of every step from there and the planes at the ends of the calls"""
    def make():
        p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
        start = cells.copy()
        oracle.run(p, start, ob, 5)
        ref, all_steps, fields = sm.oracle_rows(oracle, p, ob, start, 5, 63, 1, fields_at=call_ends(5, [23, 40]))
        return p, ob, cells, ref, all_steps, fields
    return Shared.get(("stress", "per-pass"), make)


@pytest.mark.parametrize("every", [1, 4])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_pass_families(lbm, oracle, monkeypatch, family, every):
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    p, ob, cells, ref, all_steps, fields = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % every == 0}
    steps, rows, info = check(lbm, oracle, p, ob, cells, [23, 40], every, unarmed_first=5, want=want, ref=ref, fields=fields)
    assert info["resident_steps"] == 0 and steps[0] == (5 + every - 1) // every * every


@pytest.mark.parametrize("n_gpus", [2, 3, 8])
def test_slabs(lbm, oracle, monkeypatch, n_gpus):
    """each slab gathers into its own words; the host adds the limbs and takes the largest key: the rows of one slab, and
    the planes' rows land at the slabs' places"""
    p, ob, cells, ref, all_steps, fields = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % 4 == 0}
    monkeypatch.setenv("LBM_HALO", "memcpy")
    steps, rows, info = check(lbm, oracle, p, ob, cells, [23, 40], 4, unarmed_first=5, n_gpus=n_gpus, want=want, ref=ref, fields=fields)
    assert info["n_slabs"] == n_gpus


def test_one_call_against_ragged_split_calls(lbm, oracle):
    p, ob, cells, ref, all_steps, _ = per_pass_case(lbm, oracle)
    whole = run_engine(lbm, p, ob, cells, [63], 4, unarmed_first=5)
    ragged = run_engine(lbm, p, ob, cells, [1, 2, 13, 4, 30, 1, 12], 4, unarmed_first=5)
    assert whole[2].tolist() == ragged[2].tolist() == [tt for tt in range(5, 68) if tt % 4 == 0]
    assert whole[3].tobytes() == ragged[3].tobytes()
    assert np.array_equal(bits(whole[0]), bits(ragged[0])) and np.array_equal(bits(whole[0]), bits(ref))
    assert_rows(whole[2], whole[3], {tt: v for tt, v in all_steps.items() if tt % 4 == 0})


def test_tiled_context(lbm, oracle):
    p, tile, _ = small(lbm, 32, 16)
    tile[0, 0] = tile[15, 31] = tile[5:8, 9:12] = 1
    p = lbm.Params(128, 48, 400, 10, 0.1, 0.005, 1.85)
    ob = np.tile(tile, (3, 4))
    cells = small(lbm, 128, 48, 8)[2]
    ref, want, fields = sm.oracle_rows(oracle, p, ob, cells, 0, 9, 2, fields_at=[8])
    for n_gpus in (1, 2):
        _, _, info = check(lbm, oracle, p, ob, cells, [9], 2, n_gpus=n_gpus, want=want, ref=ref, fields=fields, tiled_ob=tile)
        assert info["n_slabs"] == n_gpus


# ---- lbm_read_stress ---------------------------------------------------------------------------------------------------------
def test_null_planes_are_accepted_and_nothing_is_armed_afterwards(lbm):
    p, ob, cells = small(lbm, 24, 6, 3)
    ob[2, 5] = 1
    want = sm.field(cells, ob)[0]
    with lbm.Engine(p, ob, cells) as eng:
        for names in (("txx",), ("txy",), ("tyy",), ("txx", "tyy"), ()):
            out = {k: np.full((6, 24), np.float32(7.0)) for k in names}
            ptr = [out[k].ctypes.data if k in out else None for k in ("txx", "txy", "tyy")]
            assert eng.lib.lbm_read_stress(eng.handle, *ptr) == 0, names
            assert all(sm.same_field(out[k], want[k]) for k in names), names
        eng.set_stats(1, 4)                                 # any recorder arms: the reader left nothing armed
        eng.set_stats(0)
        assert eng.stress_rows()[0].size == 0
        eng.run(3)
        assert eng.stress_rows()[0].size == 0 and eng.info()["steps_done"] == 3


@pytest.mark.parametrize("n_gpus", [1, 3])
def test_the_planes_tie_to_the_row_of_the_same_step(lbm, oracle, monkeypatch, n_gpus):
    """math.fsum of q recomputed in float32 from the returned planes is sum_q of the row taken at the same step, bit for
    bit, and txy's is sum_txy"""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 260, 40, 6, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        eng.set_stress(5, 4)
        eng.run(11)                                         # the last step, 10, is a sample step
        t = eng.stress()
        steps, rows = eng.stress_rows()
    assert steps.tolist() == [0, 5, 10] and rows[-1]["nonfinite"] == 0
    fluid = ob == 0
    q = sm.q_of_planes(t["txx"], t["txy"], t["tyy"])
    assert rows[-1]["fluid"] == fluid.sum()
    assert np.float64(math.fsum(float(v) for v in q[fluid])).view(np.uint64) == np.float64(rows[-1]["sum_q"]).view(np.uint64)
    assert np.float64(math.fsum(float(v) for v in t["txy"][fluid])).view(np.uint64) == np.float64(rows[-1]["sum_txy"]).view(np.uint64)
    at = int(np.argmax(np.where(fluid, q, np.float32(-1.0))))
    assert (rows[-1]["max_q"], rows[-1]["max_x"], rows[-1]["max_y"]) == (q.reshape(-1)[at], at % 260, at // 260)
    # ... and the conversions agree on the two
    assert lbm.dissipation(rows, p.omega)[-1] > 0 and lbm.shear_rate_max(rows, p.omega)[-1] > 0
    s = lbm.strain_rate(t, p.omega)
    peak = np.sqrt(2 * (s["S_xx"] ** 2 + s["S_yy"] ** 2 + 2 * s["S_xy"] ** 2)).reshape(-1)[at]
    assert lbm.shear_rate_max(rows, p.omega)[-1] == pytest.approx(peak, rel=1e-6)


# ---- batches ---------------------------------------------------------------------------------------------------------------
def test_batch_members_equal_engines(lbm, oracle, monkeypatch):
    """3 members with different obstacles and omega: one launch per sample; every member's rows, lattice and av_vels are a
    single engine's, its rows the model's, and a member handle's stress() is the model's planes"""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "8")
    params, obstacles, cells = random_members(lbm, 128, 16, 3, 31)
    assert len({p.omega for p in params}) == 3 and any(not np.array_equal(obstacles[0], ob) for ob in obstacles[1:])
    calls, every = [1, 23, 7], 5
    steps, rows = [], []
    with lbm.Batch(params, obstacles, cells) as batch:
        with pytest.raises(lbm.LbmError, match="lbm_set_stress: not available on a member of a batch"):
            batch.member(0).set_stress(10, 4)
        batch.set_stress(every, 8)
        for n in calls:
            batch.run(n)
            s, r = batch.stress_rows()
            steps.append(s)
            rows.append(r)
        fields = [batch.member(i).stress() for i in range(3)]
        members = [(batch.member(i).cells(), batch.member(i).av_vels(sum(calls))) for i in range(3)]
    steps, rows = np.concatenate(steps), np.concatenate(rows)
    assert steps.tolist() == [0, 5, 10, 15, 20, 25, 30] and rows.shape == (7, 3) and rows.dtype == lbm.STRESS_DTYPE
    for i, p in enumerate(params):
        lattice, av, e_steps, e_rows, _, _ = run_engine(lbm, p, obstacles[i], cells[i], calls, every)
        assert e_steps.tolist() == steps.tolist()
        assert np.ascontiguousarray(rows[:, i]).tobytes() == e_rows.tobytes(), f"member {i}: rows differ from Engine.set_stress's"
        assert np.array_equal(bits(members[i][0]), bits(lattice)) and np.array_equal(bits(members[i][1]), bits(av))
        ref, want, model_t = sm.oracle_rows(oracle, p, obstacles[i], cells[i], 0, sum(calls), every, fields_at=[sum(calls) - 1])
        assert_rows(steps, rows[:, i], want)
        assert_fields(fields[i], model_t[sum(calls) - 1], f"member {i}")
        assert np.array_equal(bits(ref), bits(lattice))


# ---- repeatability -----------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_the_reader_changes_nothing(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 260, 40, 6, walls=False)
    same = lambda x, y: all(np.array_equal(bits(x[k]), bits(y[k])) for k in ("txx", "txy", "tyy"))
    for n_gpus in (1, 3):
        a = run_engine(lbm, p, ob, cells, [7, 6], 2, n_gpus=n_gpus, fields=True)
        b = run_engine(lbm, p, ob, cells, [7, 6], 2, n_gpus=n_gpus, fields=True)
        assert a[3].tobytes() == b[3].tobytes() and all(same(x, y) for x, y in zip(a[5], b[5]))
        plain = run_engine(lbm, p, ob, cells, [7, 6], 0, n_gpus=n_gpus, fields=False)     # never reads the planes
        read = run_engine(lbm, p, ob, cells, [7, 6], 0, n_gpus=n_gpus, fields=True)       # stress() between the two run calls
        assert np.array_equal(bits(plain[0]), bits(read[0])) and np.array_equal(bits(plain[1]), bits(read[1]))
        assert np.array_equal(bits(plain[0]), bits(a[0])) and all(same(x, y) for x, y in zip(a[5], read[5]))
