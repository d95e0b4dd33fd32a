"""Vorticity and enstrophy (lbm_read_vorticity / Engine.vorticity, lbm_set_enstrophy / Engine.set_enstrophy and the batch
twins): the field of the stored lattice and one row of its whole-lattice sums after every global timestep tt with
tt % every == 0.  Every row and every field is compared BIT FOR BIT with the numpy model (tests/vorticity_model.py) over
the oracle's lattice of that step: the sums are exact and rounded once, the maximum does not depend on order, so every
kernel path, call splitting and slab count gives the same bits; recording never changes the lattice, and av_vels equals
that of the same run issued as calls split at the sample steps.  Unless a case says otherwise the model's rows have
nonfinite == 0, asserted, so that no case passes by leaving cells out."""
import ctypes

import numpy as np
import pytest

import edge_lattice as el
import vorticity_model as vm
from test_gpu_batch import random_members
from test_gpu_forces import FAMILIES, RESIDENT_SHAPES, Shared, bits, small
from test_gpu_parity import random_case
from test_gpu_stats import split_calls

pytestmark = pytest.mark.gpu


def run_engine(lbm, p, ob, cells, calls, every=0, capacity=0, n_gpus=1, unarmed_first=0, tiled=False, fields=False):
    """`unarmed_first` steps, then the enstrophy armed, then `calls`, drained after each:
    (lattice, av_vels, steps, rows, info, [vorticity() after each call] if fields)"""
    steps, rows, ws = [], [], []
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus, tiled=tiled) as eng:
        if unarmed_first:
            eng.run(unarmed_first)
        if every:
            eng.set_enstrophy(every, capacity or 1 + sum(calls) // every)
        for n in calls:
            eng.run(n)
            if fields:
                ws.append(eng.vorticity())
            if every:
                s, r = eng.enstrophy()
                steps.append(s)
                rows.append(r)
        total = unarmed_first + sum(calls)
        return (eng.cells(), eng.av_vels(total), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(rows) if rows else np.zeros(0, lbm.ENSTROPHY_DTYPE), eng.info(), ws)


def assert_rows(steps, rows, want, clean=True):
    """want: {tt: row of vorticity_model.row}"""
    assert steps.tolist() == sorted(want)
    for tt, row in zip(steps.tolist(), rows):
        diff = vm.same_bits(row, want[tt])
        print("step", tt, {k: row[k] for k in vm.FIELDS}, "differs:", diff)
        assert not diff, (tt, diff)
        if clean:
            assert want[tt]["nonfinite"] == 0 and want[tt]["fluid"] > 0


def call_ends(unarmed_first, calls):
    return [unarmed_first + sum(calls[:i + 1]) - 1 for i in range(len(calls))]


def check(lbm, oracle, p, ob, cells, calls, every, unarmed_first=0, n_gpus=1, want=None, ref=None, fields=None, tiled_ob=None, clean=True):
    """armed run against the model on the oracle's lattices, the field after every call; lattice and av_vels against the
    unarmed run split at the sample steps"""
    ends = call_ends(unarmed_first, calls)
    if want is None:
        start = cells.copy()
        oracle.run(p, start, ob, unarmed_first)
        ref, want, fields = vm.oracle_rows(oracle, p, ob, start, unarmed_first, sum(calls), every, fields_at=ends)
    engine_ob = ob if tiled_ob is None else tiled_ob
    got, av, steps, rows, info, ws = run_engine(lbm, p, engine_ob, cells, calls, every, n_gpus=n_gpus, unarmed_first=unarmed_first,
                                                tiled=tiled_ob is not None, fields=True)
    assert_rows(steps, rows, want, clean)
    for tt, w in zip(ends, ws):
        assert w.dtype == np.float32 and vm.same_field(w, fields[tt]), ("vorticity() after step", tt)
    assert np.array_equal(bits(ref), bits(got)), "recording changed the lattice"
    base, base_av, _, _, _, _ = run_engine(lbm, p, engine_ob, cells, split_calls(unarmed_first, calls, every), n_gpus=n_gpus,
                                           tiled=tiled_ob is not None)
    assert np.array_equal(bits(base), bits(got))
    assert np.array_equal(bits(base_av), bits(av)), "recording changed av_vels"
    return steps, rows, info


# ---- shapes: the smallest at which vorticity_gather can go wrong -------------------------------------------------------
def test_smallest_case(lbm, oracle):
    p, ob, cells = small(lbm, 16, 8)
    ob[3:5, 6:8] = 1
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [5, 7], 1)
    assert len(steps) == 12 and np.all(rows["fluid"] == 124) and np.all(rows["max_abs_w"] > 0)
    assert 8e-3 < rows[0]["enstrophy"] < 1.1e-2 and 3e-3 < rows[-1]["enstrophy"] < 4.5e-3      # the random start relaxes


@pytest.mark.parametrize("nx,ny", [(1, 2), (2, 2), (3, 3), (5, 2), (4, 2)])
def test_coinciding_wraps(lbm, oracle, nx, ny):
    """nx of 1 or 2: both x neighbours are one cell and dvdx is exactly 0; ny == 2: likewise dudy"""
    p, ob, cells = small(lbm, nx, ny, 3 + nx)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [3], 1)
    if nx <= 2 and ny == 2:
        assert np.all(rows["enstrophy"] == 0.0) and np.all(rows["max_abs_w"] == 0.0) and np.all(rows["max_x"] == 0)


def strip_edge_obstacles(nx, ny, span):
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[1, 0] = ob[3, nx - 1] = 1                                        # both ends of a row: each is the other's neighbour over the wrap
    for x0 in range(span, nx, span):                                    # the last cell of a strip and the first of the next, in different rows
        ob[2, x0 - 1] = ob[0, x0] = 1
    return ob


@pytest.mark.parametrize("nx", [252, 256, 260, 508, 512, 516, 63, 64, 65, 127, 129])
def test_strip_and_lane_edges(lbm, oracle, nx):
    """widths one unit below, at and above one and two strips of a wave (4 cells per lane where nx % 4 == 0: strips of 256;
    else one: strips of 64); a blocked cell at x = 0, at x = nx - 1 and on both sides of every strip boundary, so that a
    wrong edge-lane neighbour changes w; the ragged last strip must take cell 0 for its last cell's neighbour"""
    ny, span = 5, 64 * vm.vector(nx)
    p, _, cells = small(lbm, nx, ny, nx)
    ob = strip_edge_obstacles(nx, ny, span)
    assert vm.strips(nx) == -(-nx // span) and ob.sum() == 2 + 2 * (vm.strips(nx) - 1)
    check(lbm, oracle, p, ob, cells, [2], 1)


@pytest.mark.parametrize("ny", [7, 8, 9, 20])
def test_band_edges(lbm, oracle, ny):
    """rows one below, at, one above and no multiple of the band height: the last band is short, the rows around every
    band come from the neighbouring bands' rows (or over the wrap)"""
    nx = 24
    assert vm.band_rows(ny, nx) == 8 and vm.groups(ny, nx) == 1 and -(-ny // 8) == {7: 1, 8: 1, 9: 2, 20: 3}[ny]
    p, ob, cells = small(lbm, nx, ny, ny)
    ob[0, 5] = ob[ny - 1, 9] = ob[min(8, ny - 1), 3] = 1
    check(lbm, oracle, p, ob, cells, [3], 2)


def test_tall_bands(lbm, oracle):
    """the band rule's other branch: one strip of more than 4096 * 8 rows has bands of 9 rows, the last one shorter; the
    capped grid makes every wave take several units"""
    nx, ny = 8, 4096 * 8 + 8
    assert vm.groups(ny, nx) == 512 and -(-ny // 9) == 3642 and ny % 9 != 0
    assert vm.band_rows(ny, nx) == 9                                      # the smallest grid whose bands are taller than the minimum
    p = lbm.Params(nx, ny, 4, 10, 0.1, 0.005, 1.85)
    rng = np.random.default_rng(9)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32) * np.float32(p.density)
    cells = (w * (1.0 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[8:11, 3] = ob[ny - 1, 0] = 1
    check(lbm, oracle, p, ob, cells, [1], 1)


def test_obstacles_on_all_four_edges_and_corners(lbm, oracle):
    """a blocked neighbour is 0, 0 over the x wrap, the y wrap (the mask's halo rows) and both"""
    p, ob, cells = small(lbm, 16, 8, 2)
    ob[0, 0] = ob[7, 15] = ob[0, 15] = ob[7, 0] = ob[0, 9] = ob[7, 4] = ob[3, 0] = ob[5, 15] = 1
    check(lbm, oracle, p, ob, cells, [9], 2)


# ---- seams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,n_gpus", [(20, 7, 2), (20, 7, 3), (16, 16, 8)])
def test_seams(lbm, oracle, monkeypatch, nx, ny, n_gpus):
    """slabs of 4/3 and 3/2/2 rows and eight of 2 rows (both rows are edges): a block straddles a seam, one lies on a
    slab's first row; every = 1 over 9 steps, so a stale edge row would show, then two further calls, whose passes run
    behind the copies of the rows they overwrite.  Rows and field are the model's, hence those of one slab."""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = small(lbm, nx, ny, nx + n_gpus)
    first = [lbm.partition_rows(ny, n_gpus, s)[0] for s in range(n_gpus)]
    ob[first[1] - 1:first[1] + 1, 4:6] = 1                              # straddles the seam below slab 1
    ob[first[-1], 11] = 1                                               # a slab's first row
    ob[0, 17 % nx] = ob[ny - 1, 2] = 1                                  # the periodic seam between the last slab and slab 0
    steps, rows, info = check(lbm, oracle, p, ob, cells, [9, 4, 3], 1, n_gpus=n_gpus)
    assert info["n_slabs"] == n_gpus and len(steps) == 16


@pytest.mark.parametrize("n_gpus", [1, 2])
def test_ties_take_the_smallest_cell(lbm, oracle, monkeypatch, n_gpus):
    """an open channel from the uniform equilibrium stays x-invariant: dvdx is +0 everywhere, a whole row ties and max_x is 0"""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p = lbm.Params(64, 16, 400, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((16, 64), dtype=np.int32)
    ob[[0] if n_gpus == 1 else [4, 8], :] = 1
    steps, rows, info = check(lbm, oracle, p, ob, oracle.init_cells(p), [12], 4, n_gpus=n_gpus)
    assert info["n_slabs"] == n_gpus and np.all(rows["max_x"] == 0) and np.all(rows["max_abs_w"] > 0)


# ---- paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_steps", ["1", "3"])
@pytest.mark.parametrize("shape", list(RESIDENT_SHAPES))
def test_resident_shapes(lbm, oracle, monkeypatch, shape, min_steps):
    nx, ny, env = RESIDENT_SHAPES[shape]
    calls, every = [1, 2, 19, 5], 3

    def make():
        p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
        ref, want, fields = vm.oracle_rows(oracle, p, ob, cells, 0, sum(calls), every, fields_at=call_ends(0, calls))
        return p, ob, cells, ref, want, fields
    p, ob, cells, ref, want, fields = Shared.get(("enstrophy", shape), make)
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", min_steps)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    steps, rows, info = check(lbm, oracle, p, ob, cells, calls, every, want=want, ref=ref, fields=fields)
    assert info["resident_steps"] > 0 and len(steps) == 9


def per_pass_case(lbm, oracle):
    """128 x 96; armed after 5 steps; the oracle's rows of every step from there and the fields at the ends of the calls"""
    def make():
        p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
        start = cells.copy()
        oracle.run(p, start, ob, 5)
        ref, all_steps, fields = vm.oracle_rows(oracle, p, ob, start, 5, 63, 1, fields_at=call_ends(5, [23, 40]))
        return p, ob, cells, ref, all_steps, fields
    return Shared.get(("enstrophy", "per-pass"), make)


@pytest.mark.parametrize("every", [1, 4])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_pass_families(lbm, oracle, monkeypatch, family, every):
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    p, ob, cells, ref, all_steps, fields = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % every == 0}
    steps, rows, info = check(lbm, oracle, p, ob, cells, [23, 40], every, unarmed_first=5, want=want, ref=ref, fields=fields)
    assert info["resident_steps"] == 0 and steps[0] == (5 + every - 1) // every * every


@pytest.mark.parametrize("n_gpus", [2, 3])
def test_slabs_of_the_per_pass_case(lbm, oracle, monkeypatch, n_gpus):
    p, ob, cells, ref, all_steps, fields = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % 4 == 0}
    monkeypatch.setenv("LBM_HALO", "memcpy")
    steps, rows, info = check(lbm, oracle, p, ob, cells, [23, 40], 4, unarmed_first=5, n_gpus=n_gpus, want=want, ref=ref, fields=fields)
    assert info["n_slabs"] == n_gpus


def test_tiled_context(lbm, oracle):
    p, tile, _ = small(lbm, 32, 16)
    tile[0, 0] = tile[15, 31] = tile[5:8, 9:12] = 1
    p = lbm.Params(128, 48, 400, 10, 0.1, 0.005, 1.85)
    ob = np.tile(tile, (3, 4))
    cells = small(lbm, 128, 48, 8)[2]
    ref, want, fields = vm.oracle_rows(oracle, p, ob, cells, 0, 9, 2, fields_at=[8])
    for n_gpus in (1, 2):
        _, _, info = check(lbm, oracle, p, ob, cells, [9], 2, n_gpus=n_gpus, want=want, ref=ref, fields=fields, tiled_ob=tile)
        assert info["n_slabs"] == n_gpus


def test_every_binade(lbm, oracle):
    """the lattice of tests/edge_lattice.py: populations over all the exponents the collision guards allow, so the limbs
    of both accumulators are used"""
    p, ob, cells, _ = el.build(lbm, 256, 40)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [el.STEPS], 1)
    assert np.all(rows["nonfinite"] == 0)


def test_the_difference_is_halved_once(lbm):
    """0.5f * (dvdx - dudy) against 0.5f * dvdx - 0.5f * dudy: halving is exact except where it rounds a subnormal, so the
    two orders differ only there.  A lattice at rest with rho = 1 and single populations of m = 2^-149: u_y = 3 m east of
    the cell (2, 1), u_x = m above it, so dvdx = 3 m, dudy = m and w = m; halved first, 1.5 m rounds to 2 m and 0.5 m to 0"""
    p = lbm.Params(8, 4, 4, 10, 0.1, 0.0, 1.85)
    ob = np.zeros((4, 8), dtype=np.int32)
    m = np.float32(2.0 ** -149)
    cells = np.zeros((4, 8, 9), dtype=np.float32)
    cells[..., 0] = 1.0
    cells[1, 3, 2] = np.float32(3.0) * m              # u_y(3, 1) = 3 m
    cells[2, 2, 1] = m                                # u_x(2, 2) = m
    model_w = vm.field(cells, ob)[0]
    assert model_w[1, 2] == m and model_w[1, 2] > 0 and np.float32(0.5) * (np.float32(3.0) * m) - np.float32(0.5) * m == np.float32(2.0) * m
    with lbm.Engine(p, ob, cells) as eng:
        w = eng.vorticity()
    assert w[1, 2].view(np.uint32) == 1 and vm.same_field(w, model_w)


# ---- non-finite cells ------------------------------------------------------------------------------------------------------
def test_nonfinite_populations(lbm, oracle):
    """a NaN and an Inf population in one fluid cell each: the cell and its four fluid neighbours are counted, beside a
    block one fewer; vorticity() holds NaN exactly where the model does"""
    p, ob, cells = small(lbm, 32, 8, 5)
    ob[3:5, 6:8] = 1
    with lbm.Engine(p, ob, cells) as eng:
        clean = eng.vorticity()
    assert vm.row(cells, ob)["nonfinite"] == 0 and vm.same_field(clean, vm.field(cells, ob)[0])
    for (y, x, k, value), count in (((6, 20, 3, np.nan), 5), ((1, 12, 8, np.inf), 5), ((3, 5, 2, np.nan), 4), ((0, 0, 5, np.inf), 5)):
        # (population 5 or 8 enters rho, jx and jy: Inf / Inf leaves neither velocity finite)
        bad = cells.copy()
        bad[y, x, k] = value
        want = vm.row(bad, ob)
        assert want["nonfinite"] == count and want["fluid"] == 252 - count
        with lbm.Engine(p, ob, bad) as eng:
            w = eng.vorticity()
            eng.set_enstrophy(1, 4)
            eng.run(2)
            steps, rows = eng.enstrophy()
        model_w = vm.field(bad, ob)[0]
        assert np.isnan(model_w).sum() == count - 1 and vm.same_field(w, model_w)
        ref, after, _ = vm.oracle_rows(oracle, p, ob, bad, 0, 2, 1)
        # the first step moves the one population to one cell, whose collision spoils all nine; the second spreads them
        assert after[1]["nonfinite"] > after[0]["nonfinite"] >= 3
        assert_rows(steps, rows, after, clean=False)


def test_all_nan_lattice(lbm):
    p, ob, cells = small(lbm, 20, 6)
    ob[2, 3] = 1
    cells[:] = np.nan
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_enstrophy(1, 4)
        eng.run(2)
        _, rows = eng.enstrophy()
        w = eng.vorticity()
    assert np.isnan(w).sum() == 119 and w[2, 3] == 0 and not np.signbit(w[2, 3])
    for r in rows:
        assert r["nonfinite"] == 119 and r["fluid"] == 0 and r["max_abs_w"] == 0 and (r["max_x"], r["max_y"]) == (-1, -1)
        for k in ("enstrophy", "circulation"):
            assert r[k] == 0.0 and not np.signbit(r[k])


# ---- large grids -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(1024, 1024), (1030, 512)])
def test_large_grids(lbm, oracle, nx, ny):
    """hundreds of bands that meet in the atomics, every wave sweeping its rows (four cells per lane on 1024 x 1024, one on
    1030 x 512, whose 17th strip is 6 cells wide)"""
    assert vm.strips(nx) * -(-ny // vm.band_rows(ny, nx)) >= 512 and vm.groups(ny, nx) >= 128
    p, ob, cells = random_case(lbm, nx, ny, 11, walls=False)
    check(lbm, oracle, p, ob, cells, [1], 1)


# ---- batches ---------------------------------------------------------------------------------------------------------------
def test_batch_members_equal_engines(lbm, oracle, monkeypatch):
    """3 members with different obstacles and omega: one launch per sample; every member's rows, lattice and av_vels are a
    single engine's, its rows the model's, and a member's vorticity() is the model's field"""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "8")
    params, obstacles, cells = random_members(lbm, 128, 16, 3, 31)
    assert len({p.omega for p in params}) == 3 and any(not np.array_equal(obstacles[0], ob) for ob in obstacles[1:])
    calls, every = [1, 23, 7], 5
    steps, rows, fields = [], [], []
    with lbm.Batch(params, obstacles, cells) as batch:
        with pytest.raises(lbm.LbmError, match="lbm_set_enstrophy: not available on a member of a batch"):
            batch.member(0).set_enstrophy(10, 4)
        batch.set_enstrophy(every, 8)
        for n in calls:
            batch.run(n)
            s, r = batch.enstrophy()
            steps.append(s)
            rows.append(r)
        fields = [batch.member(i).vorticity() for i in range(3)]
        members = [(batch.member(i).cells(), batch.member(i).av_vels(sum(calls))) for i in range(3)]
    steps, rows = np.concatenate(steps), np.concatenate(rows)
    assert steps.tolist() == [0, 5, 10, 15, 20, 25, 30] and rows.shape == (7, 3) and rows.dtype == lbm.ENSTROPHY_DTYPE
    for i, p in enumerate(params):
        lattice, av, e_steps, e_rows, _, _ = run_engine(lbm, p, obstacles[i], cells[i], calls, every)
        assert e_steps.tolist() == steps.tolist()
        assert np.ascontiguousarray(rows[:, i]).tobytes() == e_rows.tobytes(), f"member {i}: rows differ from Engine.set_enstrophy's"
        assert np.array_equal(bits(members[i][0]), bits(lattice)) and np.array_equal(bits(members[i][1]), bits(av))
        ref, want, model_w = vm.oracle_rows(oracle, p, obstacles[i], cells[i], 0, sum(calls), every, fields_at=[sum(calls) - 1])
        assert_rows(steps, rows[:, i], want)
        assert vm.same_field(fields[i], model_w[sum(calls) - 1]) and np.array_equal(bits(ref), bits(lattice))


def test_batch_ring_and_refusals(lbm):
    params, obstacles, cells = random_members(lbm, 128, 16, 2, 7)
    with lbm.Batch(params, obstacles, cells) as batch:
        batch.set_enstrophy(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run: 25 steps would record 3 rows.*holds 2.*lbm_batch_read_enstrophy"):
            batch.run(25)
        assert batch.info()["steps_done"] == 0
        for arm in (lambda: batch.set_stats(10, 2), lambda: batch.set_residual(10, 2), lambda: batch.set_profiles(10, 2),
                    lambda: batch.set_forces(10, 2)):
            with pytest.raises(lbm.LbmError, match=r"this batch has enstrophy rows armed \(lbm_batch_set_enstrophy\)"):
                arm()
        with pytest.raises(lbm.LbmError, match=r"this batch has enstrophy rows armed \(lbm_batch_set_enstrophy\)"):
            batch.member(1).set_frames(10, 2)                       # a kind a member may arm on its own
        with pytest.raises(lbm.LbmError, match="lbm_batch_run_until: enstrophy rows are armed"):
            batch.run_until(100, 10)
        batch.run(15)
        assert batch.enstrophy(1)[0].tolist() == [0]
        batch.run(10)                                               # 20 goes into the slot that 0 left
        steps, rows = batch.enstrophy()
        assert steps.tolist() == [10, 20] and rows.shape == (2, 2)
        batch.set_enstrophy(0)
        batch.set_stats(10, 2)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_enstrophy: this batch has lattice statistics armed"):
            batch.set_enstrophy(10, 2)


# ---- the ring ----------------------------------------------------------------------------------------------------------------
def test_ring_overflow_drain_order_query_rearm_disarm(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        n = eng.lib.lbm_read_enstrophy
        eng.set_enstrophy(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_run: 25 steps would record 3 rows.*holds 2.*lbm_read_enstrophy"):
            eng.run(25)                      # rows at 0, 10, 20
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match="2 rows are waiting"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        waiting = ctypes.c_int(-1)
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # the query form
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # ... drains nothing
        steps, first = eng.enstrophy(1)
        assert steps.tolist() == [0] and first.shape == (1,)                                      # oldest first
        eng.run(10)                          # 20 goes into the slot that 0 left: the drain crosses the wrap
        steps, rows = eng.enstrophy()
        assert steps.tolist() == [10, 20] and rows[0]["enstrophy"] != rows[1]["enstrophy"] != first[0]["enstrophy"]
        eng.run(6)                           # 30
        eng.set_enstrophy(10, 2)             # re-arming discards the unread row
        assert eng.enstrophy()[0].size == 0
        eng.run(10)                          # 40
        assert eng.enstrophy()[0].tolist() == [40]
        eng.set_enstrophy(0)                 # disarms and frees
        eng.run(30)
        assert eng.enstrophy()[0].size == 0
        assert eng.info()["steps_done"] == 71


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 4, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        for every, cap, msg in ((-1, 4, "lbm_set_enstrophy: negative interval -1"), (1, 0, "lbm_set_enstrophy: capacity 0, at least one row"),
                                (1, -2, "lbm_set_enstrophy: capacity -2"), (1, 2 ** 24, "lbm_set_enstrophy: a ring of 16777216 rows is 2 GiB or more")):
            assert eng.lib.lbm_set_enstrophy(eng.handle, every, cap) != 0
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
                                  (lambda: eng.set_profiles(10, 4), lambda: eng.set_profiles(0), "line profiles")):
            arm()
            with pytest.raises(lbm.LbmError, match="lbm_set_enstrophy: %s are armed" % name):
                eng.set_enstrophy(10, 4)
            w = eng.vorticity()                                     # the reader needs nothing armed and disturbs nothing armed
            disarm()
            eng.set_enstrophy(10, 4)
            with pytest.raises(lbm.LbmError, match=r"enstrophy rows are armed \(lbm_set_enstrophy\)"):
                arm()
            eng.set_enstrophy(0)
        eng.set_enstrophy(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_run_until: enstrophy rows are armed"):
            eng.run_until(100, 10)
        with pytest.raises(lbm.LbmError, match="lbm_run_until_residual: enstrophy rows are armed"):
            eng.run_until_residual(100, 10)
        assert eng.info()["steps_done"] == 0
    # a rank context (one rank, host message passing that is never called)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_set_enstrophy: not available in a multi-process"):
            eng.set_enstrophy(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_read_vorticity: not available in a multi-process"):
            eng.vorticity()


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_enstrophy: the context runs the %s halo mode" % mode):
                eng.set_enstrophy(10, 4)
        eng.set_halo_mode("sync")
        eng.set_enstrophy(10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match=r"lbm_set_halo_mode: enstrophy rows are armed \(lbm_set_enstrophy\)"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0


# ---- repeatability -----------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_the_reader_changes_nothing(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 260, 40, 6, walls=False)
    for n_gpus in (1, 3):
        a = run_engine(lbm, p, ob, cells, [7, 6], 2, n_gpus=n_gpus, fields=True)
        b = run_engine(lbm, p, ob, cells, [7, 6], 2, n_gpus=n_gpus, fields=True)
        assert a[3].tobytes() == b[3].tobytes() and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[5], b[5]))
        plain = run_engine(lbm, p, ob, cells, [7, 6], 0, n_gpus=n_gpus, fields=False)     # never reads the field
        read = run_engine(lbm, p, ob, cells, [7, 6], 0, n_gpus=n_gpus, fields=True)       # vorticity() between the two run calls
        assert np.array_equal(bits(plain[0]), bits(read[0])) and np.array_equal(bits(plain[1]), bits(read[1]))
        assert np.array_equal(bits(plain[0]), bits(a[0])) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[5], read[5]))
