"""The stream function (lbm_read_psi / Engine.psi, lbm_set_psi / Engine.set_psi and the batch twins): psi of the stored
lattice and one row of its extrema after every global timestep tt with tt % every == 0.  Every field and every row is
compared BIT FOR BIT, through uint64 views, with the integer model (tests/psi_model.py) over the oracle's lattice of that
step: every prefix is an exact sum rounded once, so the band height of the scan, the slab count, the kernel family and the
call splitting give the same bits; recording never changes the lattice, and av_vels equals that of the same run issued as
calls split at the sample steps.  Unless a case says otherwise the model's rows have nonfinite == 0, asserted, so that no
case passes by leaving cells out."""
import ctypes
import math
import os

import numpy as np
import pytest

import psi_model as pm
from conftest import ROOT
from test_gpu_batch import random_members
from test_gpu_forces import FAMILIES, Shared, bits, small
from test_gpu_parity import random_case
from test_gpu_stats import split_calls

pytestmark = pytest.mark.gpu

BAND = 8                     # LBM_PSI_BAND_ROWS of the small shapes: 37 rows are four full bands and one of five rows
STRIP = pm.COLUMNS           # columns of a workgroup of the scan


@pytest.fixture(autouse=True)
def small_bands(monkeypatch):
    monkeypatch.setenv("LBM_PSI_BAND_ROWS", str(BAND))
    monkeypatch.setenv("LBM_HALO", "memcpy")             # several slabs on one device


def run_engine(lbm, p, ob, cells, calls, every=0, capacity=0, n_gpus=1, unarmed_first=0, tiled=False, fields=False):
    """`unarmed_first` steps, then psi armed, then `calls`, drained after each:
    (lattice, av_vels, steps, rows, info, [psi() after each call] if fields)"""
    steps, rows, fs = [], [], []
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus, tiled=tiled) as eng:
        if unarmed_first:
            eng.run(unarmed_first)
        if every:
            eng.set_psi(every, capacity or 1 + sum(calls) // every)
        for n in calls:
            eng.run(n)
            if fields:
                fs.append(eng.psi())
            if every:
                s, r = eng.psi_rows()
                steps.append(s)
                rows.append(r)
        total = unarmed_first + sum(calls)
        return (eng.cells(), eng.av_vels(total), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(rows) if rows else np.zeros(0, lbm.PSI_DTYPE), eng.info(), fs)


def assert_rows(steps, rows, want, clean=True):
    """want: {tt: row of psi_model.row}"""
    assert steps.tolist() == sorted(want)
    for tt, row in zip(steps.tolist(), rows):
        diff = pm.same_bits(row, want[tt])
        print("step", tt, {k: row[k] for k in pm.FIELDS}, "differs:", diff)
        assert not diff, (tt, diff)
        if clean:
            assert want[tt]["nonfinite"] == 0 and want[tt]["fluid"] > 0


def oracle_case(oracle, p, ob, cells, unarmed_first, total, every=1):
    """(final lattice, {tt: row} of EVERY sample step, {tt: psi} at every step) -- computed once per case and shared"""
    ref = cells.copy()
    oracle.run(p, ref, ob, unarmed_first)
    rows, fields = {}, {}
    for tt in range(unarmed_first, unarmed_first + total):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, 1)
        psi, counted, bad = pm.field(ref, ob)
        fields[tt] = psi
        if tt % every == 0:
            lo, lx, ly, hi, hx, hy = pm.extrema(psi, counted)
            rows[tt] = {"psi_min": lo, "psi_max": hi, "nonfinite": int(bad.sum()), "min_x": lx, "min_y": ly, "max_x": hx, "max_y": hy,
                        "fluid": int(counted.sum()), "reserved": 0}
    return ref, rows, fields


def check(lbm, p, ob, cells, calls, every, case, unarmed_first=0, n_gpus=1, tiled_ob=None, clean=True):
    """armed run against the model's rows of `case` (oracle_case), psi() after every call against its fields; lattice and
    av_vels against the unarmed run split at the sample steps"""
    ref, all_rows, fields = case
    want = {tt: r for tt, r in all_rows.items() if tt % every == 0 and unarmed_first <= tt < unarmed_first + sum(calls)}
    ends = [unarmed_first + sum(calls[:i + 1]) - 1 for i in range(len(calls))]
    engine_ob = ob if tiled_ob is None else tiled_ob
    got, av, steps, rows, info, fs = run_engine(lbm, p, engine_ob, cells, calls, every, n_gpus=n_gpus, unarmed_first=unarmed_first,
                                                tiled=tiled_ob is not None, fields=True)
    assert_rows(steps, rows, want, clean)
    for tt, f in zip(ends, fs):
        assert f.dtype == np.float64 and pm.same_field(f, fields[tt]), ("psi() after step", tt)
    if ends[-1] == max(fields):
        assert np.array_equal(bits(ref), bits(got)), "recording changed the lattice"
    base, base_av, _, _, _, _ = run_engine(lbm, p, engine_ob, cells, split_calls(unarmed_first, calls, every), n_gpus=n_gpus,
                                           tiled=tiled_ob is not None)
    assert np.array_equal(bits(base), bits(got)), "recording changed the lattice"
    assert np.array_equal(bits(base_av), bits(av)), "recording changed av_vels"
    assert info["n_slabs"] == n_gpus
    return steps, rows, info


# ---- shapes: the smallest at which the scan can go wrong -----------------------------------------------------------------
def ragged_case(lbm, oracle):
    """262 x 37: one strip of 256 columns and six more (nx % 4 != 0); with bands of 8 rows four bands and one of five; on
    2, 3 and 8 slabs the seams fall inside and between bands; blocks straddle a band seam and the strip seam"""
    def make():
        nx, ny = STRIP + 6, 37
        p, ob, cells = small(lbm, nx, ny, 41)
        ob[7:9, 10:12] = ob[15:17, STRIP - 1:STRIP + 1] = ob[0, 3] = ob[ny - 1, nx - 1] = ob[18, 100] = 1
        return p, ob, cells, oracle_case(oracle, p, ob, cells, 0, 9)
    return Shared.get(("psi", "ragged"), make)


@pytest.mark.parametrize("n_gpus", [1, 2, 3, 8])
def test_ragged_bands_and_strips_every_step(lbm, oracle, n_gpus):
    """every = 1 over 9 steps in one call, then the same steps as split calls: rows and fields are the model's on 1, 2, 3
    and 8 slabs"""
    p, ob, cells, case = ragged_case(lbm, oracle)
    assert pm.band_rows(37, 262, BAND) == 8 and -(-37 // 8) == 5 and 37 % 8 != 0 and 262 % 4 != 0
    steps, rows, _ = check(lbm, p, ob, cells, [9], 1, case, n_gpus=n_gpus)
    assert len(steps) == 9 and np.all(rows["fluid"] == 262 * 37 - int(ob.sum()))
    assert np.all(rows["psi_min"] < 0) and np.all(rows["psi_max"] > 0)
    check(lbm, p, ob, cells, [1, 3, 5], 1, case, n_gpus=n_gpus)


@pytest.mark.parametrize("band", ["1", "5", "37", "64", "0"])
def test_the_band_height_changes_no_bit(lbm, oracle, monkeypatch, band):
    """bands of one row, of a height that divides nothing, of exactly and of more than all rows, and the host's own rule"""
    monkeypatch.setenv("LBM_PSI_BAND_ROWS", band)
    p, ob, cells, case = ragged_case(lbm, oracle)
    check(lbm, p, ob, cells, [4], 2, case, n_gpus=1)
    check(lbm, p, ob, cells, [4], 2, case, n_gpus=3)


@pytest.mark.parametrize("nx,ny", [(1, 2), (1, 37), (5, 2), (STRIP, 8), (STRIP + 1, 9), (2 * STRIP, 16)])
def test_smallest_shapes(lbm, oracle, nx, ny):
    """one column, two rows; a strip exactly full, one cell over, two strips; one band exactly, one row over"""
    p, ob, cells = small(lbm, nx, ny, 3 + nx + ny)
    if nx > 4:
        ob[ny // 2, nx // 2] = ob[0, nx - 1] = 1
    check(lbm, p, ob, cells, [3], 1, oracle_case(oracle, p, ob, cells, 0, 3))


# ---- the 128 x 128 data set ----------------------------------------------------------------------------------------------
def cavity_case(lbm, oracle):
    """the reference's 128 x 128 data set with its own obstacles; the model's rows and fields of its first 40 steps"""
    def make():
        inputs = os.path.join(ROOT, "tests", "golden", "inputs")
        p = lbm.read_params(os.path.join(inputs, "input_128x128.params"))
        ob = lbm.read_obstacles(os.path.join(inputs, "obstacles_128x128.dat"), p.nx, p.ny)
        cells = oracle.init_cells(p)
        return p, ob, cells, oracle_case(oracle, p, ob, cells, 0, 40)
    return Shared.get(("psi", "cavity"), make)


@pytest.mark.parametrize("n_gpus", [1, 2, 3, 8])
def test_the_field_of_the_128_data_set_after_0_1_and_40_steps(lbm, oracle, n_gpus):
    p, ob, cells, (ref, rows, fields) = cavity_case(lbm, oracle)
    assert ob.sum() > 0
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        assert eng.info()["n_slabs"] == n_gpus
        psi0 = eng.psi()
        assert psi0.dtype == np.float64 and psi0.shape == (128, 128) and pm.same_field(psi0, pm.field(cells, ob)[0])
        assert np.all(psi0.view(np.uint64) == 0)                     # the uniform equilibrium: +0.0 everywhere
        eng.run(1)
        assert pm.same_field(eng.psi(), fields[0])
        eng.run(39)
        psi40 = eng.psi()
        assert pm.same_field(psi40, fields[39]) and np.array_equal(bits(eng.cells()), bits(ref))
        assert pm.same_field(eng.psi(), fields[39])                  # the reader changes nothing
    assert np.any(psi40 != 0) and np.isfinite(psi40).all()


@pytest.mark.parametrize("path,n_gpus", [("resident", 1), ("per-pass", 1), ("per-pass", 2), ("per-pass", 3), ("per-pass", 8)])
def test_rows_of_the_128_data_set_every_4_over_40_steps(lbm, oracle, monkeypatch, path, n_gpus):
    """every = 4 >= resident_min_steps: on one slab the sub-calls run the resident kernel, or, forced, the per-pass
    kernels; several slabs run per-pass sub-calls; one call, then split calls"""
    p, ob, cells, case = cavity_case(lbm, oracle)
    if path == "resident":
        monkeypatch.setenv("LBM_RESIDENT", "1")
        monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "4")
    else:
        monkeypatch.setenv("LBM_RESIDENT", "0")
    steps, rows, info = check(lbm, p, ob, cells, [40], 4, case, n_gpus=n_gpus)
    assert (info["resident_steps"] > 0) == (path == "resident") and steps.tolist() == list(range(0, 40, 4))
    check(lbm, p, ob, cells, [1, 2, 19, 18], 4, case, n_gpus=n_gpus)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_pass_families_every_step(lbm, oracle, monkeypatch, family):
    """every = 1 over 9 steps, armed after 5 unarmed steps, on each per-pass kernel family"""
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    p, ob, cells, case = cavity_case(lbm, oracle)
    steps, rows, info = check(lbm, p, ob, cells, [3, 6], 1, case, unarmed_first=5)
    assert info["resident_steps"] == 0 and steps.tolist() == list(range(5, 14))


def test_tiled_context(lbm, oracle):
    p, tile, _ = small(lbm, 32, 16)
    tile[0, 0] = tile[15, 31] = tile[5:8, 9:12] = 1
    p = lbm.Params(128, 48, 400, 10, 0.1, 0.005, 1.85)
    ob = np.tile(tile, (3, 4))
    cells = small(lbm, 128, 48, 8)[2]
    case = oracle_case(oracle, p, ob, cells, 0, 9)
    for n_gpus in (1, 2):
        check(lbm, p, ob, cells, [9], 2, case, n_gpus=n_gpus, tiled_ob=tile)


# ---- exactness -------------------------------------------------------------------------------------------------------------
def cancellation_lattice(nx, ny, x, rows):
    """cells_aos [ny, nx, 9] at rest (g0 = 1) but for column x, whose cells at the three `rows` carry jx = 2^60, 2^-60 and
    -2^60 exactly: only g1 or only g3 is non-zero there, so jx is that population and ux = +-1"""
    cells = np.zeros((ny, nx, 9), dtype=np.float32)
    cells[:, :, 0] = 1.0
    for y, (k, v) in zip(rows, ((1, 2.0 ** 60), (1, 2.0 ** -60), (3, 2.0 ** 60))):
        cells[y, x, :] = 0.0
        cells[y, x, k] = v
    return cells


@pytest.mark.parametrize("n_gpus,rows", [(1, (6, 7, 8)), (1, (2, 12, 30)), (2, (17, 18, 19)), (2, (3, 18, 36)), (3, (11, 12, 13)),
                                         (3, (12, 24, 25)), (3, (5, 20, 30))])
def test_cancellation_across_band_and_slab_seams(lbm, n_gpus, rows):
    """2^60, 2^-60, -2^60 down one column (zero steps): the prefix after the third term is exactly 2^-60, which a float64
    running sum loses.  The three terms lie around a band seam (rows 7 | 8), in three different bands, around the slab
    seams of 2 slabs (18 | 19) and of 3 slabs (12 | 13, 24 | 25), and one in each of three slabs"""
    nx, ny, x = 20, 37, 13
    first = [lbm.partition_rows(ny, n_gpus, s)[0] for s in range(n_gpus)]
    assert first == {1: [0], 2: [0, 19], 3: [0, 13, 25]}[n_gpus]
    p = lbm.Params(nx, ny, 4, 10, 0.1, 0.0, 1.85)
    ob = np.zeros((ny, nx), dtype=np.int32)
    cells = cancellation_lattice(nx, ny, x, rows)
    want = pm.field(cells, ob)[0]
    assert want[rows[2], x] == 2.0 ** -60 and want[ny - 1, x] == 2.0 ** -60 and want[rows[1], x] == 2.0 ** 60
    assert np.cumsum(pm.terms(cells, ob)[0].astype(np.float64), axis=0)[rows[2], x] == 0.0      # what a double accumulator gives
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        assert eng.info()["n_slabs"] == n_gpus
        psi = eng.psi()
    print("psi of the column", psi[:, x])
    assert psi[rows[2], x] == 2.0 ** -60
    assert pm.same_field(psi, want)


def test_every_binade(lbm, oracle):
    """the lattice of tests/edge_lattice.py: populations over all the exponents the collision guards allow, so many limbs
    of a column's accumulator are used"""
    import edge_lattice as el
    p, ob, cells, _ = el.build(lbm, 256, 40)
    check(lbm, p, ob, cells, [el.STEPS], 1, oracle_case(oracle, p, ob, cells, 0, el.STEPS))


# ---- non-finite cells, blocked cells, ties ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_gpus", [1, 3])
def test_a_nonfinite_cell_adds_nothing_and_is_counted(lbm, oracle, n_gpus):
    """an infinite population in one fluid cell (zero steps for the field; the row after the one step that spreads it): the
    cell adds 0, is counted in nonfinite and is left out of the extrema; the cells above carry the prefix without it"""
    p, ob, cells = small(lbm, 20, 37, 5)
    ob[20, 4] = 1
    bad = cells.copy()
    bad[9, 7, 1] = np.inf                                 # jx = +inf
    want, counted, is_bad = pm.field(bad, ob)
    clean = pm.field(cells, ob)[0]
    t = pm.terms(cells, ob)[0]
    assert is_bad.sum() == 1 and is_bad[9, 7] and np.isfinite(want).all()
    assert want[9, 7].view(np.uint64) == want[8, 7].view(np.uint64)
    assert np.array_equal(np.delete(want, 7, axis=1).view(np.uint64), np.delete(clean, 7, axis=1).view(np.uint64))
    with lbm.Engine(p, ob, bad, n_gpus=n_gpus) as eng:
        psi = eng.psi()
        eng.set_psi(1, 4)
        eng.run(1)
        steps, rows = eng.psi_rows()
    assert pm.same_field(psi, want)
    step = bad.copy()
    with np.errstate(all="ignore"):
        oracle.run(p, step, ob, 1)
    after = pm.row(step, ob)
    # (the step moves the one population to the next cell, whose collision spoils all nine of that cell)
    assert after["nonfinite"] >= 1 and after["fluid"] == 20 * 37 - 1 - after["nonfinite"]
    assert_rows(steps, rows, {0: after}, clean=False)
    counted_after = pm.field(step, ob)[1]                 # the extrema sit at finite fluid cells
    assert counted_after[rows[0]["min_y"], rows[0]["min_x"]] and counted_after[rows[0]["max_y"], rows[0]["max_x"]]


def test_all_nan_lattice(lbm):
    p, ob, cells = small(lbm, 20, 6)
    ob[2, 3] = 1
    cells[:] = np.nan
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_psi(1, 4)
        eng.run(2)
        _, rows = eng.psi_rows()
        psi = eng.psi()
    assert np.all(psi.view(np.uint64) == 0)
    for r in rows:
        assert r["nonfinite"] == 119 and r["fluid"] == 0 and (r["min_x"], r["min_y"], r["max_x"], r["max_y"]) == (-1, -1, -1, -1)
        for k in ("psi_min", "psi_max"):
            assert r[k] == 0.0 and not np.signbit(r[k])


def test_blocked_cells_add_nothing(lbm, oracle):
    """after a few steps the blocked cells hold rebounded populations with a non-zero jx; psi passes through them unchanged"""
    p, ob, cells, (ref, rows, fields) = ragged_case(lbm, oracle)
    g = ref.reshape(37, 262, 9)
    jx = g[..., 1] + g[..., 5] + g[..., 8] - (g[..., 3] + g[..., 6] + g[..., 7])
    assert np.all(jx[ob != 0] != 0)
    with lbm.Engine(p, ob, ref) as eng:
        psi = eng.psi()
    assert pm.same_field(psi, fields[8])
    for y, x in zip(*np.nonzero(ob)):
        if y > 0:
            assert psi[y, x].view(np.uint64) == psi[y - 1, x].view(np.uint64)
    assert math.fsum(float(v) for v in jx[:, 10]) != psi[-1, 10]                      # the blocked cells' jx would show


@pytest.mark.parametrize("n_gpus", [1, 2])
def test_ties_go_to_the_smallest_cell(lbm, oracle, n_gpus):
    """the uniform equilibrium without a driving force has jx = +0 in every cell and stays so: psi is +0.0 everywhere, at
    step 0 and after, every fluid cell ties, and both extrema sit at the first fluid cell"""
    p = lbm.Params(STRIP + 6, 20, 40, 10, 0.1, 0.0, 1.85)
    ob = np.zeros((20, STRIP + 6), dtype=np.int32)
    ob[0, :5] = ob[3, 9] = 1
    cells = oracle.init_cells(p)
    case = oracle_case(oracle, p, ob, cells, 0, 4)
    assert all(np.all(f.view(np.uint64) == 0) for f in case[2].values())
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        assert np.all(eng.psi().view(np.uint64) == 0)                # step 0
    steps, rows, _ = check(lbm, p, ob, cells, [4], 1, case, n_gpus=n_gpus)
    for r in rows:
        assert (r["min_x"], r["min_y"], r["max_x"], r["max_y"]) == (5, 0, 5, 0)
        assert r["psi_min"] == 0.0 and r["psi_max"] == 0.0 and not np.signbit(r["psi_min"]) and not np.signbit(r["psi_max"])


@pytest.mark.parametrize("n_gpus", [1, 3])
def test_an_all_blocked_grid_has_no_extrema(lbm, oracle, n_gpus):
    p, ob, cells = small(lbm, 24, 12, 2)
    ob[:] = 1
    steps, rows, _ = check(lbm, p, ob, cells, [2], 1, oracle_case(oracle, p, ob, cells, 0, 2), n_gpus=n_gpus, clean=False)
    for r in rows:
        assert (r["min_x"], r["min_y"], r["max_x"], r["max_y"], r["fluid"], r["nonfinite"]) == (-1, -1, -1, -1, 0, 0)
        assert r["psi_min"] == 0.0 and r["psi_max"] == 0.0


# ---- the tie to the line profiles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_gpus", [1, 3])
def test_the_last_row_is_the_profiles_column_sum_of_jx(lbm, oracle, n_gpus):
    """psi[ny - 1, x] and sum_jx of column line x of lbm_set_profiles, on the same lattice, bit for bit"""
    p, ob, cells, _ = ragged_case(lbm, oracle)
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        eng.set_profiles(4, 2, ("columns",))
        eng.run(1)                                       # the sample of tt = 0: the lattice after one step
        steps, lines = eng.profiles()
        psi = eng.psi()
        assert eng.info()["n_slabs"] == n_gpus
    assert steps.tolist() == [0]
    sum_jx = np.ascontiguousarray(lines["columns"][0]["sum_jx"])
    assert sum_jx.shape == (262,) and np.any(sum_jx != 0)
    assert np.array_equal(psi[-1].view(np.uint64), sum_jx.view(np.uint64))


# ---- batches ---------------------------------------------------------------------------------------------------------------
def test_batch_members_equal_engines(lbm, oracle, monkeypatch):
    """3 members with different obstacles and omega: one launch of each kernel per sample; every member's rows, lattice and
    av_vels are a single engine's, its rows the model's, and a member's psi() is the model's field"""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "8")
    params, obstacles, cells = random_members(lbm, 128, 16, 3, 31)
    assert len({p.omega for p in params}) == 3 and any(not np.array_equal(obstacles[0], ob) for ob in obstacles[1:])
    calls, every = [1, 23, 7], 5
    steps, rows = [], []
    with lbm.Batch(params, obstacles, cells) as batch:
        with pytest.raises(lbm.LbmError, match="lbm_set_psi: not available on a member of a batch"):
            batch.member(0).set_psi(10, 4)
        batch.set_psi(every, 8)
        for n in calls:
            batch.run(n)
            s, r = batch.psi_rows()
            steps.append(s)
            rows.append(r)
        fields = [batch.member(i).psi() for i in range(3)]
        members = [(batch.member(i).cells(), batch.member(i).av_vels(sum(calls))) for i in range(3)]
    steps, rows = np.concatenate(steps), np.concatenate(rows)
    assert steps.tolist() == [0, 5, 10, 15, 20, 25, 30] and rows.shape == (7, 3) and rows.dtype == lbm.PSI_DTYPE
    for i, p in enumerate(params):
        lattice, av, e_steps, e_rows, _, _ = run_engine(lbm, p, obstacles[i], cells[i], calls, every)
        assert e_steps.tolist() == steps.tolist()
        assert np.ascontiguousarray(rows[:, i]).tobytes() == e_rows.tobytes(), f"member {i}: rows differ from Engine.set_psi's"
        assert np.array_equal(bits(members[i][0]), bits(lattice)) and np.array_equal(bits(members[i][1]), bits(av))
        ref, want, model = oracle_case(oracle, p, obstacles[i], cells[i], 0, sum(calls), every)
        assert_rows(steps, rows[:, i], want)
        assert pm.same_field(fields[i], model[sum(calls) - 1]) and np.array_equal(bits(ref), bits(lattice))


def test_batch_ring_and_refusals(lbm):
    params, obstacles, cells = random_members(lbm, 128, 16, 2, 7)
    with lbm.Batch(params, obstacles, cells) as batch:
        batch.set_psi(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run: 25 steps would record 3 rows.*holds 2.*lbm_batch_read_psi_rows"):
            batch.run(25)
        assert batch.info()["steps_done"] == 0
        for arm in (lambda: batch.set_stats(10, 2), lambda: batch.set_residual(10, 2), lambda: batch.set_profiles(10, 2),
                    lambda: batch.set_forces(10, 2), lambda: batch.set_enstrophy(10, 2)):
            with pytest.raises(lbm.LbmError, match=r"this batch has stream function rows armed \(lbm_batch_set_psi\)"):
                arm()
        with pytest.raises(lbm.LbmError, match=r"this batch has stream function rows armed \(lbm_batch_set_psi\)"):
            batch.member(1).set_frames(10, 2)                       # a kind a member may arm on its own
        with pytest.raises(lbm.LbmError, match="lbm_batch_run_until: stream function rows are armed"):
            batch.run_until(100, 10)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run_until_residual: stream function rows are armed"):
            batch.run_until_residual(100, 10)
        batch.run(15)
        assert batch.psi_rows(1)[0].tolist() == [0]
        batch.run(10)                                               # 20 goes into the slot that 0 left
        steps, rows = batch.psi_rows()
        assert steps.tolist() == [10, 20] and rows.shape == (2, 2)
        batch.set_psi(0)
        batch.set_stats(10, 2)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_psi: this batch has lattice statistics armed"):
            batch.set_psi(10, 2)


# ---- the ring ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_gpus", [1, 2])
def test_ring_overflow_drain_order_query_rearm_disarm(lbm, n_gpus):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        n = eng.lib.lbm_read_psi_rows
        eng.set_psi(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_run: 25 steps would record 3 rows.*holds 2.*lbm_read_psi_rows"):
            eng.run(25)                      # rows at 0, 10, 20: refused before any work
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match="2 rows are waiting"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        waiting = ctypes.c_int(-1)
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # the query form
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # ... drains nothing
        steps, first = eng.psi_rows(1)
        assert steps.tolist() == [0] and first.shape == (1,)                                      # oldest first
        eng.run(10)                          # 20 goes into the slot that 0 left: the drain crosses the wrap
        steps, rows = eng.psi_rows()
        assert steps.tolist() == [10, 20] and rows[0]["psi_min"] != rows[1]["psi_min"] != first[0]["psi_min"]
        eng.run(6)                           # 30
        eng.set_psi(10, 2)                   # re-arming discards the unread row
        assert eng.psi_rows()[0].size == 0
        eng.run(10)                          # 40
        assert eng.psi_rows()[0].tolist() == [40]
        eng.set_psi(0)                       # disarms and frees
        eng.run(30)
        assert eng.psi_rows()[0].size == 0
        assert eng.info()["steps_done"] == 71


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 4, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        for every, cap, msg in ((-1, 4, "lbm_set_psi: negative interval -1"), (1, 0, "lbm_set_psi: capacity 0, at least one row"),
                                (1, -2, "lbm_set_psi: capacity -2"), (1, 2 ** 25, "lbm_set_psi: a ring of 33554432 rows is 2 GiB or more")):
            assert eng.lib.lbm_set_psi(eng.handle, every, cap) != 0
            assert msg in eng.lib.lbm_last_error().decode()
        assert eng.info()["steps_done"] == 0
        # one recorder per context, both directions
        for arm, disarm, name in ((lambda: eng.set_frames(10, 2), lambda: eng.set_frames(0), "animation frames"),
                                  (lambda: eng.set_probes([(1, 1)], 1, 4), lambda: eng.set_probes([], 0), "point probes"),
                                  (lambda: eng.set_mean(10), lambda: eng.set_mean(0), "mean fields"),
                                  (lambda: eng.set_field_frames(10, 2), lambda: eng.set_field_frames(0), "field frames"),
                                  (lambda: eng.set_forces(10, 4), lambda: eng.set_forces(0), "obstacle forces"),
                                  (lambda: eng.set_stats(10, 4), lambda: eng.set_stats(0), "lattice statistics"),
                                  (lambda: eng.set_residual(10, 4), lambda: eng.set_residual(0), "velocity residuals"),
                                  (lambda: eng.set_profiles(10, 4), lambda: eng.set_profiles(0), "line profiles"),
                                  (lambda: eng.set_enstrophy(10, 4), lambda: eng.set_enstrophy(0), "enstrophy rows")):
            arm()
            with pytest.raises(lbm.LbmError, match="lbm_set_psi: %s are armed" % name):
                eng.set_psi(10, 4)
            eng.psi()                                               # the reader needs nothing armed and disturbs nothing armed
            disarm()
            eng.set_psi(10, 4)
            with pytest.raises(lbm.LbmError, match=r"stream function rows are armed \(lbm_set_psi\)"):
                arm()
            eng.set_psi(0)
        eng.set_psi(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_run_until: stream function rows are armed"):
            eng.run_until(100, 10)
        with pytest.raises(lbm.LbmError, match="lbm_run_until_residual: stream function rows are armed"):
            eng.run_until_residual(100, 10)
        assert eng.info()["steps_done"] == 0
    # a rank context (one rank, host message passing that is never called)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_set_psi: not available in a multi-process"):
            eng.set_psi(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_read_psi: not available in a multi-process"):
            eng.psi()


def test_refused_in_stale_and_freshest_halo_modes(lbm):
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_psi: the context runs the %s halo mode" % mode):
                eng.set_psi(10, 4)
        eng.set_halo_mode("sync")
        eng.set_psi(10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match=r"lbm_set_halo_mode: stream function rows are armed \(lbm_set_psi\)"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0


# ---- repeatability -----------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(lbm, oracle):
    p, ob, cells, _ = ragged_case(lbm, oracle)
    for n_gpus in (1, 3):
        a = run_engine(lbm, p, ob, cells, [7, 6], 2, n_gpus=n_gpus, fields=True)
        b = run_engine(lbm, p, ob, cells, [7, 6], 2, n_gpus=n_gpus, fields=True)
        assert a[3].tobytes() == b[3].tobytes() and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[5], b[5]))
