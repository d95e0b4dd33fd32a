"""Tracer particles (lbm_set_tracers / Engine.set_tracers, lbm_batch_set_tracers / Batch.set_tracers): positions advected
on the device through the velocity field of the stored lattice, once per sample step, by the midpoint rule over the steps
since the last sample.  Every row is compared BIT FOR BIT with the numpy model (tests/tracer_model.py, written from the
definition in include/lbm_hip.h) over the oracle's final_state of each sample step; recording never changes the lattice,
and av_vels equals that of the same run issued as calls split at the sample steps.  Each case asserts on the MODEL's
output that it shows the property it is named for (edges crossed, tracers lost, tracers at rest ...), so none passes
vacuously."""
import ctypes

import numpy as np
import pytest

import tracer_model as tm
from test_gpu_batch import random_members
from test_gpu_forces import FAMILIES, RESIDENT_SHAPES, Shared, bits, small
from test_gpu_parity import random_case
from test_gpu_residual import same
from test_gpu_stats import split_calls

pytestmark = pytest.mark.gpu


def run_engine(lbm, p, ob, cells, xy, calls, every=0, capacity=None, unarmed_first=0, tiled=False):
    """`unarmed_first` steps, then the tracers armed, then `calls`, drained after each (capacity 0: never):
    (lattice, av_vels, steps, rows, tracers() at the end, info)"""
    steps, rows, now = [], [], None
    with lbm.Engine(p, ob, cells, tiled=tiled) as eng:
        if unarmed_first:
            eng.run(unarmed_first)
        if every:
            eng.set_tracers(xy, every, 1 + sum(calls) // every if capacity is None else capacity)
        for n in calls:
            eng.run(n)
            if every and capacity != 0:
                s, r = eng.tracer_rows()
                steps.append(s)
                rows.append(r)
        if every:
            now = eng.tracers()
        total = unarmed_first + sum(calls)
        return (eng.cells(), eng.av_vels(total), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(rows) if rows else np.zeros((0, len(xy), 2)), now, eng.info())


def assert_rows(steps, rows, want):
    """want: {tt: positions} of tracer_model.oracle_rows"""
    assert steps.tolist() == sorted(want)
    for tt, row in zip(steps.tolist(), rows):
        ok = tm.same_bits(row, want[tt])
        if not ok:
            bad = np.nonzero(~((bits(row) == bits(want[tt])) | (np.isnan(row) & np.isnan(want[tt]))).all(axis=-1))[0]
            print("step", tt, "tracers", bad[:8], "got", row[bad[:8]], "want", want[tt][bad[:8]])
        assert ok, tt


def check(lbm, oracle, p, ob, cells, xy, calls, every, unarmed_first=0, want=None, ref=None, tiled_ob=None):
    """armed run against the model on the oracle's fields; tracers() is the last row; lattice and av_vels against the
    unarmed run split at the sample steps"""
    if want is None:
        start = cells.copy()
        with np.errstate(all="ignore"):
            oracle.run(p, start, ob, unarmed_first)
        ref, want = tm.oracle_rows(oracle, p, ob, start, unarmed_first, sum(calls), every, xy)
    engine_ob = ob if tiled_ob is None else tiled_ob
    got, av, steps, rows, now, info = run_engine(lbm, p, engine_ob, cells, xy, calls, every, unarmed_first=unarmed_first, tiled=tiled_ob is not None)
    assert rows.dtype == np.float64 and rows.shape == (len(want), len(xy), 2)
    assert_rows(steps, rows, want)
    assert tm.same_bits(now, rows[-1] if len(rows) else np.asarray(xy, dtype=np.float64))
    assert same(ref, got), "recording changed the lattice"
    base, base_av, _, _, _, _ = run_engine(lbm, p, engine_ob, cells, xy, split_calls(unarmed_first, calls, every), tiled=tiled_ob is not None)
    assert same(base, got)
    assert same(base_av, av), "recording changed av_vels"
    return steps, rows, info


def seeds(rng, nx, ny, n):
    """n positions: random ones, then as many as fit of the exact cell centres (fx == 0), the last doubles' neighbourhood
    below the far corner and the origin"""
    special = np.concatenate([np.stack(np.meshgrid(np.arange(nx), np.arange(ny)), axis=-1).reshape(-1, 2).astype(np.float64),
                              [[nx - 2.0 ** -40, ny - 2.0 ** -40], [0.0, 0.0]]])
    rng.shuffle(special[:-2])
    xy = rng.random((n, 2)) * (nx, ny)
    k = min(n // 2, len(special))
    if k:
        xy[n - k:] = special[len(special) - k:]                       # (the corner and the origin first)
    return xy


def moved(xy, want):
    """the smallest share, over the samples, of the live tracers that the sample moves: nothing passes by standing still
    (1.0 without obstacles; a tracer seeded at a blocked cell's centre rests)"""
    prev, share = np.asarray(xy, dtype=np.float64), 1.0
    for tt in sorted(want):
        live = np.isfinite(want[tt]).all(axis=-1)
        share = min(share, float((want[tt][live] != prev[live]).any(axis=-1).mean()))
        prev = want[tt]
    return share


# ---- 1, 2: shapes -------------------------------------------------------------------------------------------------------------
def test_smallest_case(lbm, oracle):
    p, ob, cells = small(lbm, 13, 5)
    xy = np.array([[6.3, 2.7]])
    steps, rows, _ = check(lbm, oracle, p, ob, cells, xy, [3], 1)
    assert steps.tolist() == [0, 1, 2] and len({r.tobytes() for r in rows}) == 3 and np.all(np.isfinite(rows))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_the_deal_of_tracers_over_lanes_waves_and_workgroups(lbm, oracle, n):
    """a lane per tracer, 256 lanes per workgroup: counts just below, at and above a wave, a workgroup and four of them;
    random positions, exact cell centres, the last doubles below the far corner, the origin"""
    def make():
        p, ob, cells = small(lbm, 21, 3, 24)
        ob[1, 2:4] = 1
        return p, ob, cells
    p, ob, cells = Shared.get(("tracers", "21x3"), make)
    xy = seeds(np.random.default_rng(n), 21, 3, n)
    if n >= 2:
        assert [0.0, 0.0] in xy.tolist()
    if n >= 63:
        assert [21 - 2.0 ** -40, 3 - 2.0 ** -40] in xy.tolist()
    if n >= 63:
        assert (xy == np.floor(xy)).all(axis=1).sum() >= 30
    ref, want = tm.oracle_rows(oracle, p, ob, cells, 0, 5, 2, xy)
    assert moved(xy, want) >= (1.0 if n < 63 else 0.9)                              # (a centre amid blocked cells may rest)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, xy, [5], 2, want=want, ref=ref)
    assert steps.tolist() == [0, 2, 4]


# ---- 3: both wraps, both directions -------------------------------------------------------------------------------------------
def drift_lattice(lbm, nx, ny, ux, uy):
    """every cell in equilibrium at u = (ux, uy), accel = 0: the field stays uniform"""
    p = lbm.Params(nx, ny, 400, 10, 0.1, 0.0, 1.85)
    c = np.array([[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1], [1, 1], [-1, 1], [-1, -1], [1, -1]], dtype=np.float64)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
    cu = c @ np.array([ux, uy])
    f = (w * p.density * (1 + 3 * cu + 4.5 * cu * cu - 1.5 * (ux * ux + uy * uy))).astype(np.float32)
    return p, np.zeros((ny, nx), dtype=np.int32), np.tile(f, (ny, nx, 1))


@pytest.mark.parametrize("ux,uy", [(0.1, 0.08), (-0.1, 0.08), (0.1, -0.08), (-0.1, -0.08)])
def test_both_wraps_in_both_directions(lbm, oracle, ux, uy):
    nx, ny, every, total = 14, 6, 4, 12
    p, ob, cells = drift_lattice(lbm, nx, ny, ux, uy)
    d = every * np.array([abs(ux), abs(uy)])                          # one span's drift: 0.4 x 0.32 cells
    xy = []
    for ex in (0.0, 0.5 * d[0], nx - 0.5 * d[0], nx - 2.0 ** -40, nx / 2):             # within one span of each edge ...
        for ey in (0.0, 0.5 * d[1], ny - 0.5 * d[1], ny - 2.0 ** -40, ny / 2):         # ... and corner
            xy.append([ex, ey])
    xy += [[nx - 1.0, 2.0], [nx - 0.9, 3.5], [nx - 0.75, 0.0]]        # i0 == nx - 1: the cells wrap, the tracers do not cross at first
    xy = np.array(xy)
    crossed = np.zeros(4, dtype=bool)
    span, pos, fields, ref = tm.spans(0, total, every), xy, {}, cells.copy()
    for tt in range(total):
        oracle.run(p, ref, ob, 1)
        if tt in span:
            fs = oracle.final_state(p, ref, ob)
            assert len(set(bits(fs["u_x"]).ravel().tolist())) == 1 and len(set(bits(fs["u_y"]).ravel().tolist())) == 1       # uniform
            fields[tt] = (float(fs["u_x"][0, 0]), float(fs["u_y"][0, 0]), span[tt])
            pos, ends = tm.advance(fs["u_x"], fs["u_y"], pos, span[tt], unwrapped=True)
            crossed |= np.array(tm.crossed(ends, nx, ny))
            if tt == 0:
                first_ends = ends
    assert crossed.tolist() == [ux < 0, ux > 0, uy < 0, uy > 0]       # over the four cases every edge is crossed, from the model
    assert np.all((first_ends[-3:, 0] >= 0) & (first_ends[-3:, 0] < nx)) and np.all(np.floor(xy[-3:, 0]) == nx - 1)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, xy, [total], every)
    # independent of the model: in a uniform field the displacement is the sum of span * u over the samples, modulo the grid
    drift = np.array([sum(h * u for u, _, h in fields.values()), sum(h * v for _, v, h in fields.values())])
    assert np.allclose(drift, total * np.array([ux, uy]) * (9 / 12), rtol=1e-4)         # (spans 1 + 4 + 4 = 9 of the 12 steps)
    off = (rows[-1] - (xy + drift)) / (nx, ny)
    off -= np.round(off)
    err = np.abs(off * (nx, ny)).max() / np.abs(drift).min()
    print("largest deviation from x0 + sum(span * u), relative to the drift:", err)
    assert err < 1e-9


# ---- 4, 5: pitch, obstacles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(130, 6), (257, 3)])
def test_pitch_is_not_nx(lbm, oracle, nx, ny):
    """widths that leave padding behind every row of the lattice and of the mask; obstacles, and the lid row's acceleration"""
    p, ob, cells = small(lbm, nx, ny, nx + ny)
    ob[1, 2:4] = 1
    ob[ny - 1, nx - 1] = 1
    ob[ny - 2, 7] = 1                                                  # on the lid row
    xy = seeds(np.random.default_rng(nx), nx, ny, 300)
    ref, want = tm.oracle_rows(oracle, p, ob, cells, 0, 6, 2, xy)
    assert np.isfinite(want[4]).all() and nx % 64 != 0
    check(lbm, oracle, p, ob, cells, xy, [6], 2, want=want, ref=ref)


def test_obstacles(lbm, oracle):
    """21 x 8 with a 3 x 3 block (cells 9 .. 11 x 3 .. 5): tracers beside every face and corner; one at the centre of the
    enclosed blocked cell, one off-centre between four blocked centres and one at a blocked corner cell's centre (they must
    not move: V is 0 there); one inside the block's rim, between blocked and fluid centres (the velocity falls linearly to
    0 at blocked centres: it creeps)"""
    p, ob, cells = small(lbm, 21, 8, 9)
    ob[3:6, 9:12] = 1
    beside = [[x, y] for x in (8.4, 10.0, 12.6) for y in (2.4, 4.0, 6.6) if (x, y) != (10.0, 4.0)]
    xy = np.array(beside + [[10.0, 4.0], [10.6, 4.3], [9.0, 3.0], [11.3, 4.3], [8.5, 3.5]])
    rest = [8, 9, 10]
    ref, want = tm.oracle_rows(oracle, p, ob, cells, 0, 9, 3, xy)
    for tt in want:
        assert bits(want[tt][rest]).tolist() == bits(xy[rest]).tolist()                  # at rest inside the body, every sample
    assert moved(np.delete(xy, rest, axis=0), {tt: np.delete(v, rest, axis=0) for tt, v in want.items()}) == 1.0
    # the populations of blocked cells are not at rest (bounce-back swaps what streams in): were their moments used,
    # the tracers inside the body would move
    state = cells.copy()
    oracle.run(p, state, ob, 1)
    rho = state.sum(axis=2)
    jx = (state[..., [1, 5, 8]].sum(axis=2) - state[..., [3, 6, 7]].sum(axis=2)) / rho
    assert np.all(jx[3:6, 9:12] != 0)
    steps, rows, _ = check(lbm, oracle, p, ob, cells, xy, [9], 3, want=want, ref=ref)
    assert bits(rows[:, rest]).tolist() == [bits(xy[rest]).tolist()] * 3


# ---- 6: the span --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("armed_at,first_span", [(5, 4), (6, 3)])
def test_the_span_of_the_first_sample(lbm, oracle, armed_at, first_span):
    """every = 4, armed between two sample steps: the first row is at tt = 8.  Armed at steps_done = 6 its span is 3 (steps
    6, 7, 8: lbm_residual_row.span's rule, as tests/test_gpu_residual.py has it), later rows span 4.  Armed at steps_done =
    5 the span is 4 by the same rule (steps 5 .. 8) -- the issue's text names 3 there, which is the rule at 6; both are run.
    One call and ragged split calls give the same rows; lattice and av_vels are the unarmed split run's (check)"""
    p, ob, cells = small(lbm, 32, 8, 5)
    ob[3:5, 6:8] = 1
    xy = seeds(np.random.default_rng(1), 32, 8, 70)
    total = 20 - armed_at                                             # up to the step before the sample step 20
    assert list(tm.spans(armed_at, total, 4).items()) == [(8, first_span), (12, 4), (16, 4)]
    start = cells.copy()
    oracle.run(p, start, ob, armed_at)
    ref, want = tm.oracle_rows(oracle, p, ob, start, armed_at, total, 4, xy)
    wrong = tm.advance(*[oracle_field(oracle, p, ob, cells, 9)[k] for k in ("u_x", "u_y")], xy, 4 if first_span == 3 else 3)
    assert not tm.same_bits(wrong, want[8])                           # the other span gives other bits
    steps, rows, _ = check(lbm, oracle, p, ob, cells, xy, [total], 4, unarmed_first=armed_at, want=want, ref=ref)
    ragged = run_engine(lbm, p, ob, cells, xy, [1, 2, 6, 1, total - 10], 4, capacity=4, unarmed_first=armed_at)
    assert ragged[2].tolist() == steps.tolist() == [8, 12, 16] and ragged[3].tobytes() == rows.tobytes()
    assert same(ragged[0], ref)


def oracle_field(oracle, p, ob, cells, steps):
    ref = cells.copy()
    oracle.run(p, ref, ob, steps)
    return oracle.final_state(p, ref, ob)


# ---- 7: kernel families ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_steps", ["1", "3"])
@pytest.mark.parametrize("shape", list(RESIDENT_SHAPES))
def test_resident_shapes(lbm, oracle, monkeypatch, shape, min_steps):
    """sub-calls above and below resident_min_steps: the launch reads the lattice the last kernel wrote, whichever it was"""
    nx, ny, env = RESIDENT_SHAPES[shape]
    calls, every = [1, 2, 19, 5], 3

    def make():
        p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
        xy = seeds(np.random.default_rng(3), nx, ny, 300)
        ref, want = tm.oracle_rows(oracle, p, ob, cells, 0, sum(calls), every, xy)
        return p, ob, cells, xy, ref, want
    p, ob, cells, xy, ref, want = Shared.get(("tracers", shape), make)
    assert np.isfinite(want[24]).all()
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", min_steps)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    steps, rows, info = check(lbm, oracle, p, ob, cells, xy, calls, every, want=want, ref=ref)
    assert info["resident_steps"] > 0 and len(steps) == 9


def per_pass_case(lbm, oracle):
    """128 x 96; armed after 5 unarmed steps; the oracle's fields of every step from there"""
    def make():
        p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
        xy = seeds(np.random.default_rng(4), 128, 96, 500)
        start = cells.copy()
        oracle.run(p, start, ob, 5)
        out = {}
        for every in (1, 4):
            ref, out[every] = tm.oracle_rows(oracle, p, ob, start, 5, 63, every, xy)
        return p, ob, cells, xy, ref, out
    return Shared.get(("tracers", "per-pass"), make)


@pytest.mark.parametrize("every", [1, 4])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_pass_families(lbm, oracle, monkeypatch, family, every):
    """each family leaves the current lattice in the one or the other buffer after its passes: a launch that read the wrong
    one would see the field of a step before"""
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    p, ob, cells, xy, ref, want = per_pass_case(lbm, oracle)
    assert np.isfinite(want[every][67 // every * every]).all() and moved(xy, want[every]) > 0.9
    steps, rows, info = check(lbm, oracle, p, ob, cells, xy, [23, 40], every, unarmed_first=5, want=want[every], ref=ref)
    assert info["resident_steps"] == 0 and steps[0] == (5 + every - 1) // every * every


# ---- 8: the ring ------------------------------------------------------------------------------------------------------------------
def test_ring_end_partial_drains_full_ring_and_no_ring(lbm, oracle):
    p, ob, cells = small(lbm, 32, 8, 6)
    ob[3:5, 6:8] = 1
    xy = seeds(np.random.default_rng(2), 32, 8, 65)
    ref, want = tm.oracle_rows(oracle, p, ob, cells, 0, 40, 2, xy)
    assert moved(xy, want) > 0.9
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_tracers(xy, 2, 3)
        assert tm.same_bits(eng.tracers(), xy)                        # before the first sample: the start
        eng.run(5)                                                    # rows of steps 0, 2, 4: the ring is full
        assert eng.lib.lbm_run(eng.handle, 2) == 1                    # refused before any work
        assert eng.lib.lbm_last_error().decode() == ("lbm_run: 2 steps would record 1 rows, but the row buffer holds 3 and 3 rows are "
                                                     "waiting (lbm_read_tracers drains them)")
        assert eng.info()["steps_done"] == 5 and tm.same_bits(eng.tracers(), want[4])
        steps, rows = eng.tracer_rows(2)                              # a partial drain
        assert steps.tolist() == [0, 2]
        assert_rows(steps, rows, {0: want[0], 2: want[2]})
        eng.run(4)                                                    # steps 6 and 8 go into slots 0 and 1, behind 4 in slot 2
        assert tm.same_bits(eng.tracers(), want[8])
        n = ctypes.c_int(-1)
        assert eng.lib.lbm_read_tracers(eng.handle, 0, None, None, ctypes.byref(n)) == 0 and n.value == 3
        assert tm.same_bits(eng.tracers(), want[8])                   # ... which drains nothing
        steps, rows = eng.tracer_rows()                               # across the ring's end
        assert_rows(steps, rows, {tt: want[tt] for tt in (4, 6, 8)})
        assert eng.tracer_rows()[0].size == 0
        # no ring: a long run never refuses, the reader does, tracers() is the model's
        eng.set_tracers(rows[-1], 2, 0)
        eng.run(31)
        with pytest.raises(lbm.LbmError, match=r"lbm_read_tracers: tracer particles are armed without a ring \(capacity 0\): no row is recorded"):
            eng.tracer_rows()
        assert tm.same_bits(eng.tracers(), want[38]) and same(eng.cells(), ref)
        eng.set_tracers(xy[:0], 2, 4)                                 # no tracers: disarms
        with pytest.raises(lbm.LbmError, match="lbm_tracers_now"):
            eng.tracers()
        eng.set_stats(1, 4)                                           # ... so another kind arms


# ---- 9: lost tracers ----------------------------------------------------------------------------------------------------------------
def test_lost_tracers(lbm, oracle):
    """a NaN population in one fluid cell of the start lattice (as the statistics tests build it): the tracers whose cells
    of either stage touch a NaN velocity turn (NaN, NaN) at the first sample and stay so; the NaN spreads with the steps"""
    p, ob, cells = small(lbm, 32, 8, 5)
    ob[3:5, 6:8] = 1
    cells[6, 20, 3] = np.nan
    # (after the first step the NaN population has streamed west, into cell (19, 6), whose collision spreads it over its nine)
    xy = np.concatenate([seeds(np.random.default_rng(8), 32, 8, 120), [[18.5, 5.5], [19.0, 6.0], [19.7, 6.9], [2.0, 1.0], [28.5, 2.5]]])
    with np.errstate(all="ignore"):
        ref, want = tm.oracle_rows(oracle, p, ob, cells, 0, 3, 1, xy)
    lost = [np.isnan(want[tt]).all(axis=-1) for tt in (0, 1, 2)]
    assert lost[0][-5:].tolist() == [True, True, True, False, False]
    assert 3 <= lost[0].sum() < lost[1].sum() < lost[2].sum() < len(xy)                  # more are lost with every step, never all
    assert all(np.all(l1[l0]) for l0, l1 in zip(lost, lost[1:]))                         # ... and stay so
    assert all(np.array_equal(np.isnan(want[tt][:, 0]), np.isnan(want[tt][:, 1])) for tt in want)
    with np.errstate(all="ignore"):
        steps, rows, _ = check(lbm, oracle, p, ob, cells, xy, [3], 1, want=want, ref=ref)
    assert np.isnan(rows[0, -5:-2]).all() and np.isfinite(rows[2][~lost[2]]).all()


# ---- 10: batches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [3, 9])
def test_batch_members_equal_engines(lbm, oracle, monkeypatch, members):
    """128 x 12 members (one XCD each; with 9 one lands in the second launch of a chunk) with different omega and
    obstacles, 70 tracers each: one launch per sample; every member's rows, lattice and av_vels are a single engine's"""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "8")
    params, obstacles, cells = random_members(lbm, 128, 12, members, 31)
    assert len({p.omega for p in params}) == members and any(not np.array_equal(obstacles[0], ob) for ob in obstacles[1:])
    rng = np.random.default_rng(members)
    xy = np.stack([seeds(rng, 128, 12, 70) for _ in range(members)])
    calls, every = [1, 23, 7], 5
    steps, rows = [], []
    with lbm.Batch(params, obstacles, cells) as batch:
        if members == 9:
            assert batch.info()["launches_per_chunk"] >= 2
        with pytest.raises(lbm.LbmError, match="lbm_set_tracers: not available on a member of a batch"):
            batch.member(0).set_tracers(xy[0], 10, 4)
        batch.set_tracers(xy, every, 8)
        assert tm.same_bits(batch.tracers(), xy)
        for n in calls:
            batch.run(n)
            s, r = batch.tracer_rows()
            steps.append(s)
            rows.append(r)
        now = batch.tracers()
        got = [(batch.member(i).cells(), batch.member(i).av_vels(sum(calls))) for i in range(members)]
    steps, rows = np.concatenate(steps), np.concatenate(rows)
    assert steps.tolist() == [0, 5, 10, 15, 20, 25, 30] and rows.shape == (7, members, 70, 2) and tm.same_bits(now, rows[-1])
    for i, p in enumerate(params):
        lattice, av, e_steps, e_rows, _, _ = run_engine(lbm, p, obstacles[i], cells[i], xy[i], calls, every)
        assert e_steps.tolist() == steps.tolist()
        assert tm.same_bits(rows[:, i], e_rows), f"member {i}: rows differ from Engine.set_tracers'"
        assert same(got[i][0], lattice) and same(got[i][1], av)
        if i in (0, members - 1):                                     # ... and the model's (the oracle is the slow part)
            ref, want = tm.oracle_rows(oracle, p, obstacles[i], cells[i], 0, sum(calls), every, xy[i])
            assert_rows(steps, rows[:, i], want)
            assert same(ref, lattice) and moved(xy[i], want) > 0.75      # (walls: a seed at a blocked centre rests)
    assert len({rows[-1, i].tobytes() for i in range(members)}) == members               # every member has a flow of its own


# ---- 11, 12, 13 -------------------------------------------------------------------------------------------------------------------------
def test_tiled_context(lbm, oracle):
    """lbm_create_tiled with one slab: the same bits as the untiled map"""
    p, tile, _ = small(lbm, 32, 16)
    tile[0, 0] = tile[15, 31] = tile[5:8, 9:12] = 1
    p = lbm.Params(128, 48, 400, 10, 0.1, 0.005, 1.85)
    ob = np.tile(tile, (3, 4))
    cells = small(lbm, 128, 48, 8)[2]
    xy = seeds(np.random.default_rng(5), 128, 48, 200)
    ref, want = tm.oracle_rows(oracle, p, ob, cells, 0, 9, 2, xy)
    _, _, info = check(lbm, oracle, p, ob, cells, xy, [9], 2, want=want, ref=ref, tiled_ob=tile)
    assert info["n_slabs"] == 1
    check(lbm, oracle, p, ob, cells, xy, [9], 2, want=want, ref=ref)


def test_volume(lbm, oracle):
    """1024 x 64, 65 536 random tracers (256 workgroups), 3 samples at every = 4, against the vectorised model"""
    p, ob, cells = random_case(lbm, 1024, 64, 12, walls=False)
    xy = np.random.default_rng(6).random((65536, 2)) * (1024, 64)
    ref, want = tm.oracle_rows(oracle, p, ob, cells, 0, 9, 4, xy)
    assert np.isfinite(want[8]).all() and moved(xy, want) > 0.9
    got, _, steps, rows, now, _ = run_engine(lbm, p, ob, cells, xy, [9], 4)
    assert_rows(steps, rows, want)
    assert steps.tolist() == [0, 4, 8] and same(got, ref) and tm.same_bits(now, rows[-1])


def test_two_runs_give_the_same_bits(lbm):
    p, ob, cells = random_case(lbm, 260, 40, 6, walls=False)
    xy = seeds(np.random.default_rng(7), 260, 40, 1000)
    a = run_engine(lbm, p, ob, cells, xy, [7, 6], 2)
    b = run_engine(lbm, p, ob, cells, xy, [7, 6], 2)
    assert a[2].tolist() == b[2].tolist() == [0, 2, 4, 6, 8, 10, 12] and a[3].tobytes() == b[3].tobytes()
    assert same(a[0], b[0]) and same(a[1], b[1])
    shuffled = np.random.default_rng(1).permutation(1000)             # the caller's order is the row's order, and nothing else
    c = run_engine(lbm, p, ob, cells, xy[shuffled], [7, 6], 2)
    assert c[3].tobytes() == np.ascontiguousarray(a[3][:, shuffled]).tobytes()


# ---- 14: the refusals, word for word --------------------------------------------------------------------------------------------------------
def c_arm(o, name, n, xy, every, capacity):
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    status = getattr(o.lib, name)(o.handle, n, xy.ctypes.data if xy.size else None, every, capacity)
    return status, o.lib.lbm_last_error().decode()


@pytest.mark.parametrize("owner", ["context", "batch"])
def test_the_kinds_own_refusals_word_for_word(lbm, owner):
    p, ob, cells = small(lbm, 30, 8, 2)
    batch = owner == "batch"
    name = "lbm_batch_set_tracers" if batch else "lbm_set_tracers"
    lattices = 3 if batch else 1
    xy = np.tile(seeds(np.random.default_rng(1), 30, 8, 4), (lattices, 1))
    with (lbm.Batch([p] * 3, [ob] * 3, [cells] * 3) if batch else lbm.Engine(p, ob, cells)) as o:
        assert c_arm(o, name, 4, xy, -1, 4) == (1, f"{name}: negative interval -1")
        assert c_arm(o, name, 4, xy, 2, -1) == (1, f"{name}: negative capacity -1 (0: no ring)")
        for n in (-1, (1 << 24) + 1):
            assert c_arm(o, name, n, xy, 2, 4) == (1, f"{name}: {n} tracers, between 0 (none: disarms) and LBM_MAX_TRACERS = 16777216 are possible")
        full = 3 if batch else 8                                      # 256 MiB per lattice and row
        assert c_arm(o, name, 1 << 24, xy, 2, full)[1].startswith(f"{name}: a ring of {full} rows ")
        assert "2 GiB or more" in o.lib.lbm_last_error().decode()
        assert c_arm(o, name, 4, xy[:0], 2, 4) == (1, f"{name}: NULL start positions")
        for at, bad in ((1, (np.nan, 1.0)), (2, (3.0, np.inf)), (0, (-1e-300, 1.0)), (3, (30.0, 1.0)), (1, (1.0, 8.0)), (4 * lattices - 1, (1.0, -1.0))):
            start = xy.copy()
            start[at:, :] = bad                                       # the first offending index is named
            of = f" of member {at // 4}" if batch else ""
            assert c_arm(o, name, 4, start, 2, 4) == (1, f"{name}: tracer {at % 4}{of} starts at ({bad[0]:g}, {bad[1]:g}), not a finite position "
                                                      "with 0 <= x < 30 and 0 <= y < 8")
        assert o.info()["steps_done"] == 0
        o.run(3)                                                      # nothing was armed by any of that
        o.set_tracers(xy.reshape(3, 4, 2) if batch else xy, 2, 4)
        prefix = "lbm_batch_" if batch else "lbm_"
        assert getattr(o.lib, prefix + "set_stats")(o.handle, 2, 4) == 1
        if batch:
            assert o.lib.lbm_last_error().decode() == ("lbm_batch_set_stats: this batch has tracer particles armed (lbm_batch_set_tracers); a batch "
                                                       "records one kind -- disarm them with lbm_batch_set_tracers(batch, 0, NULL, 0, 0) first")
        else:
            assert o.lib.lbm_last_error().decode() == ("lbm_set_stats: tracer particles are armed (lbm_set_tracers) and a context has one recorder -- "
                                                       "disarm them with lbm_set_tracers(ctx, 0, NULL, 0, 0) first")
        assert c_arm(o, name, 4, xy, 0, 0)[0] == 0                    # disarms
        assert getattr(o.lib, prefix + "set_stats")(o.handle, 2, 4) == 0


def test_two_slabs_are_refused(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = small(lbm, 32, 32, 3)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        assert eng.info()["n_slabs"] == 2
        assert c_arm(eng, "lbm_set_tracers", 2, np.ones((2, 2)), 4, 4) == (
            1, "lbm_set_tracers: the context has 2 slabs; a tracer's four cells can straddle two slabs, and a slab's lattice halo rows are not "
            "current after a pass: tracers need a context of one slab")
        eng.set_stats(1, 2)                                           # nothing was armed
