"""Lattice statistics (lbm_set_stats / Engine.set_stats): one row of whole-lattice sums, the largest |u| and the count of
non-finite cells after every global timestep tt with tt % every == 0.  Every row is compared BIT FOR BIT with the numpy
model (tests/stats_model.py) over the oracle's lattice of that step: the sums are exact and rounded once, the maximum
does not depend on order, so every kernel path, call splitting and slab count gives the same bits; recording never
changes the lattice, and av_vels equals that of the same run issued as calls split at the sample steps."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import edge_lattice as el
import stats_model
import test_frames_format as model
from conftest import GOLDEN
from test_gpu_forces import FAMILIES, RESIDENT_SHAPES, Shared, bits, small
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu

BLOCK, MAX_GROUPS = 256, 512            # stats_gather: lanes per workgroup, the cap of the grid


def run_engine(lbm, p, ob, cells, calls, every=0, capacity=0, n_gpus=1, unarmed_first=0, tiled=False):
    """`unarmed_first` steps, then statistics armed, then `calls`, drained after each: (lattice, av_vels, steps, rows, info, mass)"""
    steps, rows = [], []
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus, tiled=tiled) as eng:
        if unarmed_first:
            eng.run(unarmed_first)
        if every:
            eng.set_stats(every, capacity or 1 + sum(calls) // every)
        for n in calls:
            eng.run(n)
            if every:
                s, r = eng.stats()
                steps.append(s)
                rows.append(r)
        total = unarmed_first + sum(calls)
        return (eng.cells(), eng.av_vels(total), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(rows) if rows else np.zeros(0, lbm.STATS_DTYPE), eng.info(), eng.total_density())


def assert_rows(steps, rows, want):
    """want: {tt: row of stats_model.row}"""
    assert steps.tolist() == sorted(want)
    for tt, row in zip(steps.tolist(), rows):
        diff = stats_model.same_bits(row, want[tt])
        print("step", tt, {k: row[k] for k in stats_model.FIELDS}, "differs:", diff)
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


def check(lbm, oracle, p, ob, cells, calls, every, unarmed_first=0, n_gpus=1, want=None, ref=None, tiled_ob=None):
    """armed run against the model on the oracle's lattices; lattice and av_vels against the unarmed run split at the sample steps"""
    if want is None:
        start = cells.copy()
        oracle.run(p, start, ob, unarmed_first)
        ref, want = stats_model.oracle_rows(oracle, p, ob, start, unarmed_first, sum(calls), every)
    engine_ob = ob if tiled_ob is None else tiled_ob
    got, av, steps, rows, info, mass = run_engine(lbm, p, engine_ob, cells, calls, every, n_gpus=n_gpus, unarmed_first=unarmed_first,
                                                  tiled=tiled_ob is not None)
    assert_rows(steps, rows, want)
    assert np.array_equal(bits(ref), bits(got)), "recording changed the lattice"
    base, base_av, _, _, _, _ = run_engine(lbm, p, engine_ob, cells, split_calls(unarmed_first, calls, every), n_gpus=n_gpus,
                                           tiled=tiled_ob is not None)
    assert np.array_equal(bits(base), bits(got))
    assert np.array_equal(bits(base_av), bits(av)), "recording changed av_vels"
    # the mass against lbm_total_density, which sums the same terms in double in one fixed order
    if len(rows) and steps[-1] == unarmed_first + sum(calls) - 1 and rows[-1]["nonfinite"] == 0:
        limit = stats_model.bound(ref, ob)["mass"]
        print("|mass - total_density|", abs(rows[-1]["mass"] - mass), "bound", limit)
        assert abs(rows[-1]["mass"] - mass) <= limit
    return steps, rows, info


# ---- shapes: the smallest at which stats_gather can go wrong ------------------------------------------------------------
def test_smallest_case(lbm, oracle):
    p, ob, cells = small(lbm, 16, 8)
    ob[3:5, 6:8] = 1
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [5, 7], 1)
    assert len(steps) == 12 and rows[-1]["mom_x"] > 0.0 and rows[-1]["nonfinite"] == 0


@pytest.mark.parametrize("nx,ny", [(21, 3), (16, 4), (13, 5), (85, 3), (16, 16), (257, 3), (130, 6), (252, 4), (260, 4)])
def test_lane_wave_and_workgroup_edges(lbm, oracle, nx, ny):
    """cells just below, at and above a wave (63, 64, 65) and a workgroup (255, 256, 771 = 3 * 257); widths that are no
    multiple of 4 take one cell per lane and leave pitch padding behind every row; 252 x 4 and 260 x 4 put the four-cell
    units just below and above one workgroup's 256"""
    p, ob, cells = small(lbm, nx, ny, nx + ny)
    ob[1, 2:4] = 1
    ob[ny - 1, nx - 1] = 1                               # the last owned cell is blocked: its rho is mass all the same
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
    of every accumulator are used"""
    p, ob, cells, _ = el.build(lbm, 256, 40)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [el.STEPS], 1)
    assert np.all(rows["nonfinite"] == 0)


# ---- ties ---------------------------------------------------------------------------------------------------------------
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
    assert np.all(rows["max_x"] == 0) and np.all(rows["max_u"] > 0)


@pytest.mark.parametrize("n_gpus", [1, 2, 3])
def test_every_fluid_cell_ties_at_rest(lbm, oracle, monkeypatch, n_gpus):
    """without acceleration the uniform equilibrium stays at rest: every fluid cell of every slab ties at |u| = +0 and
    the first fluid cell of the grid, (0, 1), is reported"""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p = lbm.Params(64, 24, 400, 10, 0.1, 0.0, 1.85)
    ob = np.zeros((24, 64), dtype=np.int32)
    ob[0, :] = 1
    steps, rows, info = check(lbm, oracle, p, ob, oracle.init_cells(p), [6], 2, n_gpus=n_gpus)
    assert info["n_slabs"] == n_gpus
    for r in rows:
        assert (r["max_u"], r["max_x"], r["max_y"]) == (0.0, 0, 1) and r["mom_x"] == r["mom_y"] == r["sum_u_sq"] == 0.0


# ---- non-finite cells -----------------------------------------------------------------------------------------------------
def test_nonfinite_cells_are_counted_and_left_out(lbm, oracle):
    p, ob, cells = small(lbm, 32, 8, 5)
    ob[3:5, 6:8] = 1
    cells[6, 20, 3] = np.inf                              # a fluid cell
    cells[3, 7, 2] = np.nan                               # a blocked cell
    ref, want = stats_model.oracle_rows(oracle, p, ob, cells, 0, 3, 1)
    assert want[0]["nonfinite"] >= 2 and want[2]["nonfinite"] > want[0]["nonfinite"]
    for calls, every in (([1], 1), ([3], 2)):
        got, _, steps, rows, _, _ = run_engine(lbm, p, ob, cells, calls, every)
        assert_rows(steps, rows, {tt: want[tt] for tt in steps.tolist()})
    assert steps.tolist() == [0, 2]
    # the lattice is the oracle's: the same cells are NaN (a NaN's payload is not the arithmetic's to keep), the rest bit for bit
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(got)) and np.array_equal(bits(ref)[~nan], bits(got)[~nan])


def test_all_nan_lattice(lbm):
    p, ob, cells = small(lbm, 20, 6)
    ob[2, 3] = 1
    cells[:] = np.nan
    _, _, steps, rows, _, _ = run_engine(lbm, p, ob, cells, [2], 1)
    for r in rows:
        assert r["nonfinite"] == 120 and r["max_u"] == 0 and (r["max_x"], r["max_y"]) == (-1, -1)
        for k in ("mass", "mom_x", "mom_y", "sum_u_sq"):
            assert r[k] == 0.0 and not np.signbit(r[k])


# ---- paths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_steps", ["1", "3"])
@pytest.mark.parametrize("shape", list(RESIDENT_SHAPES))
def test_resident_shapes(lbm, oracle, monkeypatch, shape, min_steps):
    nx, ny, env = RESIDENT_SHAPES[shape]
    calls, every = [1, 2, 19, 5], 3

    def make():
        p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
        ref, want = stats_model.oracle_rows(oracle, p, ob, cells, 0, sum(calls), every)
        return p, ob, cells, ref, want
    p, ob, cells, ref, want = Shared.get(("stats", shape), make)
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", min_steps)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    steps, rows, info = check(lbm, oracle, p, ob, cells, calls, every, want=want, ref=ref)
    assert info["resident_steps"] > 0 and len(steps) == 9


def per_pass_case(lbm, oracle):
    """128 x 96; armed after 5 steps; the oracle's rows of every step from there"""
    def make():
        p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
        start = cells.copy()
        oracle.run(p, start, ob, 5)
        ref, all_steps = stats_model.oracle_rows(oracle, p, ob, start, 5, 63, 1)
        return p, ob, cells, ref, all_steps
    return Shared.get(("stats", "per-pass"), make)


@pytest.mark.parametrize("every", [1, 3, 4, 7])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_pass_families(lbm, oracle, monkeypatch, family, every):
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % every == 0}
    steps, rows, info = check(lbm, oracle, p, ob, cells, [23, 40], every, unarmed_first=5, want=want, ref=ref)
    assert info["resident_steps"] == 0 and steps[0] == (5 + every - 1) // every * every


@pytest.mark.parametrize("n_gpus", [2, 3])
def test_slabs(lbm, oracle, monkeypatch, n_gpus):
    """each slab gathers into its own words; the host adds the limbs and takes the largest key: the rows of one slab"""
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % 4 == 0}
    monkeypatch.setenv("LBM_HALO", "memcpy")
    steps, rows, info = check(lbm, oracle, p, ob, cells, [23, 40], 4, unarmed_first=5, n_gpus=n_gpus, want=want, ref=ref)
    assert info["n_slabs"] == n_gpus


def test_one_call_against_ragged_split_calls(lbm, oracle):
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
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
    ref, want = stats_model.oracle_rows(oracle, p, ob, cells, 0, 9, 2)
    for n_gpus in (1, 2):
        _, _, info = check(lbm, oracle, p, ob, cells, [9], 2, n_gpus=n_gpus, want=want, ref=ref, tiled_ob=tile)
        assert info["n_slabs"] == n_gpus


# ---- the ring -------------------------------------------------------------------------------------------------------------
def test_ring_overflow_drain_order_query_rearm_disarm(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        n = eng.lib.lbm_read_stats
        eng.set_stats(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_run: 25 steps would record 3 rows.*holds 2.*lbm_read_stats"):
            eng.run(25)                      # rows at 0, 10, 20
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match="2 rows are waiting"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        waiting = ctypes.c_int(-1)
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # the query form
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # ... drains nothing
        steps, first = eng.stats(1)
        assert steps.tolist() == [0] and first.shape == (1,)                                      # oldest first
        eng.run(10)                          # 20 goes into the slot that 0 left
        steps, rows = eng.stats()
        assert steps.tolist() == [10, 20] and rows[0]["mom_x"] != rows[1]["mom_x"] and first[0]["mom_x"] != rows[1]["mom_x"]
        eng.run(6)                           # 30
        eng.set_stats(10, 2)                 # re-arming discards the unread row
        assert eng.stats()[0].size == 0
        eng.run(10)                          # 40
        assert eng.stats()[0].tolist() == [40]
        eng.set_stats(0)                     # disarms and frees
        eng.run(30)
        assert eng.stats()[0].size == 0
        assert eng.info()["steps_done"] == 71


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 4, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        for every, cap, msg in ((-1, 4, "lbm_set_stats: negative interval -1"), (1, 0, "lbm_set_stats: capacity 0, at least one row"),
                                (1, -2, "lbm_set_stats: capacity -2"), (1, 2 ** 23, "lbm_set_stats: a ring of 8388608 rows is 2 GiB or more")):
            assert eng.lib.lbm_set_stats(eng.handle, every, cap) != 0
            assert msg in eng.lib.lbm_last_error().decode()
        assert eng.info()["steps_done"] == 0
        # one recorder per context, both directions
        for arm, disarm, name in ((lambda: eng.set_frames(10, 2), lambda: eng.set_frames(0), "animation frames"),
                                  (lambda: eng.set_probes([(1, 1)], 1, 4), lambda: eng.set_probes([], 0), "point probes"),
                                  (lambda: eng.set_mean(10), lambda: eng.set_mean(0), "mean fields"),
                                  (lambda: eng.set_field_frames(10, 2), lambda: eng.set_field_frames(0), "field frames"),
                                  (lambda: eng.set_forces(10, 4), lambda: eng.set_forces(0), "obstacle forces")):
            arm()
            with pytest.raises(lbm.LbmError, match="lbm_set_stats: %s are armed" % name):
                eng.set_stats(10, 4)
            disarm()
            eng.set_stats(10, 4)
            with pytest.raises(lbm.LbmError, match=r"lattice statistics are armed \(lbm_set_stats\)"):
                arm()
            eng.set_stats(0)
        eng.set_stats(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_run_until: lattice statistics are armed"):
            eng.run_until(100, 10)
        assert eng.info()["steps_done"] == 0
    with lbm.Batch([p, p], [ob, ob], [cells, cells]) as batch:
        with pytest.raises(lbm.LbmError, match="lbm_set_stats: not available on a member of a batch"):
            batch.member(0).set_stats(10, 4)
    # a rank context (one rank, host message passing that is never called)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_set_stats: not available in a multi-process"):
            eng.set_stats(10, 4)


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_stats: the context runs the %s halo mode" % mode):
                eng.set_stats(10, 4)
        eng.set_halo_mode("sync")
        eng.set_stats(10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match=r"lbm_set_halo_mode: lattice statistics are armed \(lbm_set_stats\)"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_cli_writes_stats_dat(lbm, datasets, tmp_path):
    """d2q9-bgk with LBM_STATS=50 on 128^2 for 1 000 steps: stats.dat has one row per sample step and is write_stats of
    Engine.stats, byte for byte; final_state.dat as without the variable, which writes no stats.dat."""
    p, ob = datasets("128x128")
    p.max_iters = 1000
    of = os.path.join(GOLDEN, "inputs", "obstacles_128x128.dat")
    outs = {}
    for label, extra in (("plain", {}), ("stats", {"LBM_STATS": "50"})):
        d = tmp_path / label
        d.mkdir()
        pf = d / "input.params"
        pf.write_text("%d\n%d\n%d\n%d\n%.9g\n%.9g\n%.9g\n" % (p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel, p.omega))
        out = subprocess.run([lbm.CLI_PATH, str(pf), of], cwd=d, capture_output=True, text=True, env=dict(os.environ, **extra), timeout=120)
        assert out.returncode == 0, out.stderr
        assert "not finite" not in out.stderr
        outs[label] = d
    md5 = [hashlib.md5((outs[k] / "final_state.dat").read_bytes()).hexdigest() for k in ("plain", "stats")]
    assert md5[0] == md5[1]
    assert not (outs["plain"] / "stats.dat").exists()
    with lbm.Engine(p, ob) as eng:
        eng.set_stats(50, 32)
        eng.run(1000)
        steps, rows = eng.stats()
    assert steps.tolist() == list(range(0, 1000, 50))
    lines = (outs["stats"] / "stats.dat").read_text().splitlines()
    assert [int(line.split(":")[0]) for line in lines] == steps.tolist()
    parsed = np.array([[float(v) for v in line.split(":")[1].split()] for line in lines])
    assert parsed.shape == (20, 8)
    assert np.allclose(parsed[:, 0], rows["mass"], rtol=1e-12, atol=0.0) and np.all(parsed[:, 7] == 0) and np.all(rows["max_u"] > 0)
    twin = tmp_path / "twin.dat"
    lbm.write_stats(str(twin), steps, rows)
    assert (outs["stats"] / "stats.dat").read_bytes() == twin.read_bytes()
