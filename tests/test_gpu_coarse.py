"""Coarse frames (lbm_set_coarse_frames / Engine.set_coarse_frames, lbm_read_coarse / Engine.coarse): after every global
timestep tt with tt % every == 0 one frame of per-box sums.  Every box of every frame is compared BIT FOR BIT with the
numpy model (tests/coarse_model.py) over the oracle's lattice of that step: the sums are exact and rounded once -- on the
device, except in the box rows two slabs share -- so every kernel path, call splitting, slab count and batch membership
gives the same bits; recording never changes the lattice, and av_vels equals that of the same run issued as calls split
at the sample steps."""
import ctypes

import numpy as np
import pytest

import coarse_model
import edge_lattice as el
from test_gpu_batch import random_members
from test_gpu_forces import FAMILIES, RESIDENT_SHAPES, Shared, bits, small
from test_gpu_parity import random_case
from test_gpu_stats import split_calls

pytestmark = pytest.mark.gpu

# coarse_gather: a lane owns a column of its box row.  bx <= WAVE: a wave owns a span of WAVE // bx whole boxes, a
# workgroup BLOCK // WAVE = 4 consecutive spans; bx > WAVE: a workgroup owns one box of at most BLOCK columns
WAVE, BLOCK, MAX_BOX = 64, 256, 256


def spans(nx, bx):
    """wave spans of one box row (bx <= WAVE)"""
    return -(-(-(-nx // bx)) // (WAVE // bx))


def run_engine(lbm, p, ob, cells, calls, every=0, box=(16, 16), capacity=0, n_gpus=1, unarmed_first=0, tiled=False, read_too=False):
    """`unarmed_first` steps, then coarse frames armed, then `calls`, drained after each:
    (lattice, av_vels, steps, frames [n][cy][cx], info, [Engine.coarse(box) after each call] if read_too)"""
    steps, frames, reads = [], [], []
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus, tiled=tiled) as eng:
        if unarmed_first:
            eng.run(unarmed_first)
        if every:
            eng.set_coarse_frames(every, capacity or 1 + sum(calls) // every, box)
        for n in calls:
            eng.run(n)
            if every:
                s, f = eng.coarse_frames()
                steps.append(s)
                frames.append(f)
            if read_too:
                reads.append(eng.coarse(box))
        total = unarmed_first + sum(calls)
        cy, cx = coarse_model.shape(p.nx, p.ny, box if isinstance(box, tuple) else (box, box))
        return (eng.cells(), eng.av_vels(total), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(frames) if frames else np.zeros((0, cy, cx), lbm.PROFILE_DTYPE), eng.info(), reads)


def assert_frames(steps, frames, want):
    """want: {tt: frame of coarse_model.frame}"""
    assert steps.tolist() == sorted(want) and frames.shape[0] == len(steps)
    for i, tt in enumerate(steps.tolist()):
        diff = coarse_model.same_bits(frames[i], want[tt])
        print("step", tt, "frame", frames[i].shape, "first", frames[i][0, 0], "differs:", diff[:4])
        assert not diff, (tt, diff[:8])


def check(lbm, oracle, p, ob, cells, calls, every, box, unarmed_first=0, n_gpus=1, want=None, ref=None, tiled_ob=None):
    """armed run against the model on the oracle's lattices; lattice and av_vels against the unarmed run split at the sample steps"""
    if want is None:
        start = cells.copy()
        oracle.run(p, start, ob, unarmed_first)
        ref, want = coarse_model.oracle_frames(oracle, p, ob, start, unarmed_first, sum(calls), every, box)
    engine_ob = ob if tiled_ob is None else tiled_ob
    got, av, steps, frames, info, _ = run_engine(lbm, p, engine_ob, cells, calls, every, box, n_gpus=n_gpus, unarmed_first=unarmed_first,
                                                 tiled=tiled_ob is not None)
    assert frames.shape[1:] == coarse_model.shape(p.nx, p.ny, box)
    assert_frames(steps, frames, want)
    assert np.array_equal(bits(ref), bits(got)), "recording changed the lattice"
    base, base_av, _, _, _, _ = run_engine(lbm, p, engine_ob, cells, split_calls(unarmed_first, calls, every), n_gpus=n_gpus,
                                           tiled=tiled_ob is not None)
    assert np.array_equal(bits(base), bits(got))
    assert np.array_equal(bits(base_av), bits(av)), "recording changed av_vels"
    return steps, frames, info


def one_lattice(lbm, oracle, key, nx, ny, steps, shape_ob):
    """(p, ob, cells, the oracle's lattice after `steps` steps), computed once per key and never changed"""
    def make():
        p, ob, cells = small(lbm, nx, ny, nx + ny)
        shape_ob(ob)
        ref = cells.copy()
        oracle.run(p, ref, ob, steps)
        return p, ob, cells, ref
    return Shared.get(("coarse", key), make)


def check_boxes(lbm, p, ob, cells, ref, steps, boxes, n_gpus=1):
    """one unarmed engine advanced `steps` steps: Engine.coarse of every box against the model on the oracle's lattice
    `ref` of that step; {box: frame}"""
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        eng.run(steps)
        assert np.array_equal(bits(eng.cells()), bits(ref))
        out = {}
        for box in boxes:
            want = coarse_model.frame(ref, ob, box)
            got = eng.coarse(box)
            diff = coarse_model.same_bits(got, want)
            print("box", box, "frame", got.shape, "last", got[-1, -1], "differs:", diff[:4])
            assert not diff, (box, diff[:8])
            out[box] = got
        return out


# ---- shapes: the smallest at which the kernel can go wrong --------------------------------------------------------------
def test_smallest_case(lbm, oracle):
    p, ob, cells = small(lbm, 16, 8)
    ob[3:5, 6:8] = 1
    steps, frames, _ = check(lbm, oracle, p, ob, cells, [5, 7], 1, (4, 2))
    assert len(steps) == 12 and frames.shape == (12, 4, 4)
    last = frames[-1]
    assert last["fluid"].tolist() == [[8] * 4, [8, 6, 8, 8], [8, 6, 8, 8], [8] * 4] and np.all(last["nonfinite"] == 0)
    assert last["sum_jx"][3, 0] > 0.0                                     # the driven row (ny - 2) lies in the last box row


NARROW = [(1, 7), (2, 1), (3, 2), (5, 3), (31, 1), (32, 7), (33, 2), (63, 3), (64, 1)]
WIDE = [(65, 1), (127, 5), (128, 1), (129, 5), (255, 1), (256, 5)]


@pytest.mark.parametrize("box", NARROW, ids=lambda b: "%dx%d" % b)
def test_wave_span_edges(lbm, oracle, box):
    """bx <= 64 on nx = 130 (no multiple of 4: pitch padding behind every row), ny = 7: a ragged last box for every bx but
    1, 2, 5, boxes per wave from 64 down to 1 with idle lanes at 3, 5, 31, 33, 63, span counts that are no multiple of
    the 4 waves of a workgroup; by of 1, 2, 3 (ragged) and the whole height.  An obstacle in row 1, the last cell
    blocked.  The recorder's frames through one armed run, and Engine.coarse of its last lattice."""
    nx, ny = 130, 7
    assert {b[0] for b in NARROW} == {1, 2, 3, 5, 31, 32, 33, 63, 64} and {b[1] for b in NARROW} == {1, 2, 3, 7}
    assert any(spans(nx, b[0]) % (BLOCK // WAVE) for b in NARROW) and nx % 4 != 0

    def shape_ob(ob):
        ob[1, 2:4] = 1
        ob[ny - 1, nx - 1] = 1
    p, ob, cells, ref3 = one_lattice(lbm, oracle, "narrow", nx, ny, 3, shape_ob)
    steps, frames, _ = check(lbm, oracle, p, ob, cells, [3], 2, box)
    assert steps.tolist() == [0, 2]
    got = check_boxes(lbm, p, ob, cells, ref3, 3, [box])[box]
    assert got.tobytes() == frames[-1].tobytes()
    assert got["fluid"][-1, -1] == (nx - (got.shape[1] - 1) * box[0]) * (ny - (got.shape[0] - 1) * box[1]) - 1


@pytest.mark.parametrize("box", WIDE, ids=lambda b: "%dx%d" % b)
def test_workgroup_box_edges(lbm, oracle, box):
    """bx > 64 on nx = 300, ny = 6: a workgroup per box with 1, 2, 3 or 4 working waves, the last box narrower (44 wide at
    256: one working wave that is not full); by of 1 and 5 (ragged: a last box row of one row)"""
    nx, ny = 300, 6
    assert nx - 256 == 44

    def shape_ob(ob):
        ob[1, 2:4] = ob[2:4, 140:150] = 1
        ob[ny - 1, nx - 1] = 1
    p, ob, cells, ref3 = one_lattice(lbm, oracle, "wide", nx, ny, 3, shape_ob)
    steps, frames, _ = check(lbm, oracle, p, ob, cells, [3], 2, box)
    got = check_boxes(lbm, p, ob, cells, ref3, 3, [box])[box]
    assert got.tobytes() == frames[-1].tobytes()
    assert got.shape == (-(-ny // box[1]), -(-nx // box[0]))
    assert got["fluid"][-1, -1] == (nx - (got.shape[1] - 1) * box[0]) - 1      # the last box row is one row for both by; its last cell is blocked


@pytest.mark.parametrize("nx,ny,box", [(20, 300, (4, 256)), (512, 300, (8, 256))])
def test_tall_boxes(lbm, oracle, nx, ny, box):
    """every lane walks 256 rows, then a ragged box row of 44; at 512 wide several workgroups do"""
    p, ob, cells = random_case(lbm, nx, ny, 11, walls=False)
    assert ny - MAX_BOX == 44 and (nx == 20 or spans(nx, box[0]) > BLOCK // WAVE)
    steps, frames, _ = check(lbm, oracle, p, ob, cells, [1], 1, box)
    assert frames.shape == (1, 2, nx // box[0])


@pytest.mark.parametrize("box", [(32, 8), (100, 40)], ids=lambda b: "%dx%d" % b)
def test_every_binade(lbm, oracle, box):
    """the lattice of tests/edge_lattice.py: populations over all the exponents the collision guards allow, so the limbs
    of every accumulator are used, and the device's rounding meets every binade"""
    def make():
        p, ob, cells, _ = el.build(lbm, 256, 40)
        return p, ob, cells
    p, ob, cells = Shared.get(("coarse", "binade"), make)
    steps, frames, _ = check(lbm, oracle, p, ob, cells, [el.STEPS], 1, box)
    assert np.all(frames["nonfinite"] == 0)


# ---- ties ---------------------------------------------------------------------------------------------------------------
def test_ties_to_profiles_stats_and_final_state(lbm, oracle):
    nx, ny = 72, 11
    p, ob, cells = small(lbm, nx, ny, 3)
    ob[4:6, 30:33] = ob[0, 0] = ob[10, 71] = 1
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_profiles(1, 8)
        eng.run(4)
        before = eng.cells()
        rows_frame, columns_frame, all_frame, cell_frame = eng.coarse((nx, 1)), eng.coarse((1, ny)), eng.coarse((nx, ny)), eng.coarse(1)
        boxes = eng.coarse((5, 3))                                        # ... with the line profiles armed
        assert np.array_equal(bits(before), bits(eng.cells()))            # nothing is disturbed
        steps, lines = eng.profiles()                                     # ... and the profiles' records are all there
        assert steps.tolist() == [0, 1, 2, 3]
        assert rows_frame.shape == (ny, 1) and rows_frame[:, 0].tobytes() == lines["rows"][-1].tobytes()
        assert columns_frame.shape == (1, nx) and columns_frame[0].tobytes() == lines["columns"][-1].tobytes()
        state = eng.final_state()
    with lbm.Engine(p, ob, cells) as eng:                                 # the statistics of the same lattice: a recorder of their own
        eng.run(3)
        eng.set_stats(1, 2)
        eng.run(1)
        stats = eng.stats()[1][-1]
        assert np.array_equal(bits(before), bits(eng.cells()))
        # the recorder's frame of a step against Engine.coarse of that lattice
        eng.set_stats(0)
        eng.set_coarse_frames(1, 2, (5, 3))
        eng.run(1)
        frame = eng.coarse_frames()[1][-1]
        assert frame.tobytes() == eng.coarse((5, 3)).tobytes() and frame.tobytes() != boxes.tobytes()
    assert all_frame.shape == (1, 1) and all_frame[0, 0]["nonfinite"] == 0
    assert bits(np.float64(all_frame[0, 0]["sum_jx"])) == bits(np.float64(stats["mom_x"]))
    assert bits(np.float64(all_frame[0, 0]["sum_jy"])) == bits(np.float64(stats["mom_y"]))
    assert cell_frame.shape == (ny, nx) and np.all(cell_frame["nonfinite"] == 0)
    fluid = ob == 0
    assert np.array_equal(cell_frame["fluid"], fluid.astype(np.int32))
    for key, field in (("u_x", "sum_ux"), ("u_y", "sum_uy")):
        wide = np.asarray(state[key], dtype=np.float32).astype(np.float64)
        assert np.array_equal(bits(cell_frame[field])[fluid], bits(wide)[fluid])
        assert np.all(bits(cell_frame[field])[~fluid] == 0)               # +0.0 on a blocked cell
    want = coarse_model.frame(before, ob, (5, 3))
    assert not coarse_model.same_bits(boxes, want)


# ---- blocked boxes and non-finite cells -------------------------------------------------------------------------------
def test_nonfinite_cells_are_counted_in_their_box_and_left_out(lbm, oracle):
    p, ob, cells = small(lbm, 32, 8, 5)
    ob[3:5, 6:8] = 1
    ob[6:8, 16:24] = 1                                    # the box (2, 3) of 8 x 2 boxes, fully blocked
    cells[1, 20, 3] = np.inf                              # a fluid cell
    cells[3, 7, 2] = np.nan                               # a blocked cell: counted nowhere
    box = (8, 2)
    ref, want = coarse_model.oracle_frames(oracle, p, ob, cells, 0, 3, 1, box)
    bad0 = [[b["nonfinite"] for b in row] for row in want[0]]
    assert sum(map(sum, bad0)) >= 1 and sum(b["nonfinite"] for row in want[2] for b in row) > sum(map(sum, bad0))
    for calls, every in (([1], 1), ([3], 2)):
        got, _, steps, frames, _, _ = run_engine(lbm, p, ob, cells, calls, every, box)
        assert_frames(steps, frames, {tt: want[tt] for tt in steps.tolist()})
        assert all(np.all(np.isfinite(frames[k])) for k in coarse_model.SUMS)
    assert steps.tolist() == [0, 2] and frames["nonfinite"][0].tolist() == bad0
    blocked = frames[:, 3, 2]
    assert np.all(blocked["fluid"] == 0) and np.all(blocked["nonfinite"] == 0)
    for k in coarse_model.SUMS:
        assert np.all(bits(blocked[k]) == 0)
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(got)) and np.array_equal(bits(ref)[~nan], bits(got)[~nan])


def test_all_nan_lattice(lbm):
    p, ob, cells = small(lbm, 20, 6)
    ob[2, 3] = 1
    cells[:] = np.nan
    _, _, steps, frames, _, reads = run_engine(lbm, p, ob, cells, [2], 1, (8, 4), read_too=True)
    assert frames.shape == (2, 2, 3) and frames["nonfinite"][0].tolist() == [[31, 32, 16], [16, 16, 8]]
    assert np.all(frames["fluid"] == 0) and reads[0].tobytes() == frames[-1].tobytes()
    for k in coarse_model.SUMS:
        assert np.all(bits(frames[k]) == 0)


# ---- paths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_steps", ["1", "3"])
@pytest.mark.parametrize("shape", list(RESIDENT_SHAPES))
def test_resident_shapes(lbm, oracle, monkeypatch, shape, min_steps):
    nx, ny, env = RESIDENT_SHAPES[shape]
    calls, every, box = [1, 2, 19, 5], 3, (16, 5)

    def make():
        p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
        ref, want = coarse_model.oracle_frames(oracle, p, ob, cells, 0, sum(calls), every, box)
        return p, ob, cells, ref, want
    p, ob, cells, ref, want = Shared.get(("coarse", shape), make)
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", min_steps)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    steps, frames, info = check(lbm, oracle, p, ob, cells, calls, every, box, want=want, ref=ref)
    assert info["resident_steps"] > 0 and len(steps) == 9


PER_PASS_BOX = (24, 10)


def per_pass_case(lbm, oracle):
    """128 x 96; armed after 5 steps; the oracle's frames of every step from there"""
    def make():
        p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
        start = cells.copy()
        oracle.run(p, start, ob, 5)
        ref, all_steps = coarse_model.oracle_frames(oracle, p, ob, start, 5, 63, 1, PER_PASS_BOX)
        return p, ob, cells, ref, all_steps
    return Shared.get(("coarse", "per-pass"), make)


@pytest.mark.parametrize("every", [1, 3, 4, 7])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_pass_families(lbm, oracle, monkeypatch, family, every):
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % every == 0}
    steps, frames, info = check(lbm, oracle, p, ob, cells, [23, 40], every, PER_PASS_BOX, unarmed_first=5, want=want, ref=ref)
    assert info["resident_steps"] == 0 and steps[0] == (5 + every - 1) // every * every


def test_one_call_against_ragged_split_calls(lbm, oracle):
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
    whole = run_engine(lbm, p, ob, cells, [63], 4, PER_PASS_BOX, unarmed_first=5)
    ragged = run_engine(lbm, p, ob, cells, [1, 2, 13, 4, 30, 1, 12], 4, PER_PASS_BOX, unarmed_first=5)
    assert whole[2].tolist() == ragged[2].tolist() == [tt for tt in range(5, 68) if tt % 4 == 0]
    assert whole[3].tobytes() == ragged[3].tobytes()
    assert np.array_equal(bits(whole[0]), bits(ragged[0])) and np.array_equal(bits(whole[0]), bits(ref))
    assert_frames(whole[2], whole[3], {tt: v for tt, v in all_steps.items() if tt % 4 == 0})


# ---- slabs --------------------------------------------------------------------------------------------------------------
def slab_case(lbm, oracle):
    def make():
        p, ob, cells = small(lbm, 72, 16, 16)
        ob[1, 2:4] = ob[15, 71] = ob[5:7, 40] = 1
        ref = cells.copy()
        lattices = {}
        for tt in range(7):
            oracle.run(p, ref, ob, 1)
            if tt % 2 == 0:
                lattices[tt] = ref.copy()
        return p, ob, cells, ref, lattices
    return Shared.get(("coarse", "slabs"), make)


@pytest.mark.parametrize("by", [1, 4, 5, 16])
def test_slabs(lbm, oracle, monkeypatch, by):
    """1, 2 and 3 slabs (of 6, 5 and 5 rows on ny = 16).  by = 1: every box row whole; 4: box rows straddle both seams; 5:
    also a ragged last box row; 16: one box row through all three slabs, the middle slab's only box row both its first
    and its last.  A box row's limbs are added over the slabs before the one rounding: the frames of one slab, bit for bit"""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells, ref, lattices = slab_case(lbm, oracle)
    box = (9, by)
    want = {tt: coarse_model.frame(lat, ob, box) for tt, lat in lattices.items()}
    assert [lbm.partition_rows(16, 3, s)[1] for s in range(3)] == [6, 5, 5]
    seen = []
    for n_gpus in (1, 2, 3):
        steps, frames, info = check(lbm, oracle, p, ob, cells, [4, 3], 2, box, n_gpus=n_gpus, want=want, ref=ref)
        assert info["n_slabs"] == n_gpus
        seen.append(frames)
        with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:            # the one-shot reader on the same slabs
            eng.run(7)
            assert eng.coarse(box).tobytes() == frames[-1].tobytes()
    for other in seen[1:]:
        assert other.tobytes() == seen[0].tobytes()


def test_eight_slabs(lbm, oracle, monkeypatch):
    """8 slabs of 2 rows with by = 3: every slab has a partial box row, most have two"""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells, ref, lattices = slab_case(lbm, oracle)
    box = (9, 3)
    want = {tt: coarse_model.frame(lat, ob, box) for tt, lat in lattices.items()}
    assert [lbm.partition_rows(16, 8, s)[1] for s in range(8)] == [2] * 8
    steps, frames, info = check(lbm, oracle, p, ob, cells, [4, 3], 2, box, n_gpus=8, want=want, ref=ref)
    assert info["n_slabs"] == 8
    one = run_engine(lbm, p, ob, cells, [4, 3], 2, box)[3]
    assert one.tobytes() == frames.tobytes()


def test_tiled_context(lbm, oracle):
    p, tile, _ = small(lbm, 32, 16)
    tile[0, 0] = tile[15, 31] = tile[5:8, 9:12] = 1
    p = lbm.Params(128, 48, 400, 10, 0.1, 0.005, 1.85)
    ob = np.tile(tile, (3, 4))
    cells = small(lbm, 128, 48, 8)[2]
    box = (20, 7)
    ref, want = coarse_model.oracle_frames(oracle, p, ob, cells, 0, 9, 2, box)
    expanded = check(lbm, oracle, p, ob, cells, [9], 2, box, want=want, ref=ref)[1]
    for n_gpus in (1, 2):
        _, frames, info = check(lbm, oracle, p, ob, cells, [9], 2, box, n_gpus=n_gpus, want=want, ref=ref, tiled_ob=tile)
        assert info["n_slabs"] == n_gpus
        assert frames.tobytes() == expanded.tobytes()


# ---- batches ------------------------------------------------------------------------------------------------------------
def run_batch(lbm, params, obstacles, cells, calls, every, box, capacity=0):
    steps, frames = [], []
    with lbm.Batch(params, obstacles, cells) as batch:
        batch.set_coarse_frames(every, capacity or 1 + sum(calls) // every, box)
        for n in calls:
            batch.run(n)
            s, f = batch.coarse_frames()
            steps.append(s)
            frames.append(f)
        info = batch.info()
        total = sum(calls)
        assert info["steps_done"] == total
        members = [(batch.member(i).cells(), batch.member(i).av_vels(total), batch.member(i).coarse(box)) for i in range(len(params))]
    return members, np.concatenate(steps), np.concatenate(frames), info


@pytest.mark.parametrize("nx,ny,resident,box", [(128, 128, True, (16, 16)), (100, 40, False, (33, 5)), (102, 12, False, (33, 5))])
def test_batch_members_equal_engines_and_model(lbm, oracle, monkeypatch, nx, ny, resident, box):
    """three members that differ in omega, acceleration and obstacle map, on a resident shape (the calls straddle
    resident_min_steps = 8) and on two that are not"""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "8")
    params, obstacles, cells = random_members(lbm, nx, ny, 3, nx + 3)
    assert len({(p.omega, p.accel) for p in params}) == 3
    calls, every = ([1, 23, 7], 10) if resident else ([12, 9], 4)
    members, steps, frames, info = run_batch(lbm, params, obstacles, cells, calls, every, box)
    assert (info["resident_steps"] > 0) == resident
    assert frames.shape == (len(steps), 3) + coarse_model.shape(nx, ny, box)
    for i, p in enumerate(params):
        lattice, av, e_steps, e_frames, _, reads = run_engine(lbm, p, obstacles[i], cells[i], calls, every, box, read_too=True)
        assert steps.tolist() == e_steps.tolist()
        assert np.ascontiguousarray(frames[:, i]).tobytes() == e_frames.tobytes(), f"member {i}: frames differ from Engine.set_coarse_frames'"
        assert np.array_equal(bits(members[i][0]), bits(lattice)) and np.array_equal(bits(members[i][1]), bits(av)), f"member {i}"
        assert members[i][2].tobytes() == reads[-1].tobytes()             # lbm_read_coarse on a member handle
    i = 1
    ref, want = coarse_model.oracle_frames(oracle, params[i], obstacles[i], cells[i], 0, sum(calls), every, box)
    assert_frames(steps, np.ascontiguousarray(frames[:, i]), want)
    assert np.array_equal(bits(members[i][0]), bits(ref))
    assert not coarse_model.same_bits(members[i][2], coarse_model.frame(ref, obstacles[i], box))


def test_batch_ring_and_refusals(lbm):
    params, obstacles, cells = random_members(lbm, 128, 16, 3, 23)
    with lbm.Batch(params, obstacles, cells) as batch:
        lib, h = batch.lib, batch.handle
        n = lib.lbm_batch_read_coarse_frames
        done = lambda: [batch.member(i).info()["steps_done"] for i in range(3)] + [batch.info()["steps_done"]]  # noqa: E731
        member_bytes = 128 * 16 * 48                                     # boxes of one cell: a line per cell
        too_many = -(-2 ** 31 // (3 * member_bytes))
        for every, cap, bx, by, msg in ((-1, 4, 8, 8, "negative interval -1"), (1, 0, 8, 8, "capacity 0, at least one frame"),
                                        (1, 4, 0, 8, "box 0 x 8, a box side is at least 1"), (1, 4, 8, -1, "box 8 x -1, a box side is at least 1"),
                                        (1, 4, 129, 8, "box side bx 129 is larger than the grid's nx 128"),
                                        (1, 4, 8, 17, "box side by 17 is larger than the grid's ny 16"),
                                        (1, too_many, 1, 1, "a ring of %d frames of 3 members is 2.00 GiB, 2 GiB or more (%d bytes per member and frame)"
                                         % (too_many, member_bytes))):
            assert lib.lbm_batch_set_coarse_frames(h, every, cap, bx, by) != 0
            assert lib.lbm_last_error().decode().startswith("lbm_batch_set_coarse_frames: ") and msg in lib.lbm_last_error().decode()
        batch.set_coarse_frames(10, 2, (16, 4))
        with pytest.raises(lbm.LbmError, match="lbm_batch_run: 25 steps would record 3 frames.*holds 2.*lbm_batch_read_coarse_frames"):
            batch.run(25)                    # frames at 0, 10, 20
        assert done() == [0, 0, 0, 0]        # a run without room moves no member
        batch.run(15)
        with pytest.raises(lbm.LbmError, match="2 frames are waiting"):
            batch.run(10)
        assert done() == [15, 15, 15, 15]
        waiting = ctypes.c_int(-1)
        assert n(h, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2       # the query form drains nothing
        steps, first = batch.coarse_frames(1)
        assert steps.tolist() == [0] and first.shape == (1, 3, 4, 8)
        batch.run(10)
        assert batch.coarse_frames()[0].tolist() == [10, 20]
        # the member-level setters and the six other batch kinds, while the batch's coarse frames are armed
        m = batch.member(2)
        for arm in (lambda: m.set_frames(10, 2), lambda: m.set_probes([(1, 1)], 1, 4), lambda: m.set_mean(10), lambda: m.set_field_frames(10, 2)):
            with pytest.raises(lbm.LbmError, match=r"this batch has coarse frames armed \(lbm_batch_set_coarse_frames\)"):
                arm()
        others = (("forces", lambda: batch.set_forces(10, 4), lambda: batch.set_forces(0), "obstacle forces"),
                  ("stats", lambda: batch.set_stats(10, 4), lambda: batch.set_stats(0), "lattice statistics"),
                  ("residual", lambda: batch.set_residual(10, 4), lambda: batch.set_residual(0), "velocity residuals"),
                  ("profiles", lambda: batch.set_profiles(10, 4), lambda: batch.set_profiles(0), "line profiles"),
                  ("enstrophy", lambda: batch.set_enstrophy(10, 4), lambda: batch.set_enstrophy(0), "enstrophy rows"),
                  ("psi", lambda: batch.set_psi(10, 4), lambda: batch.set_psi(0), "stream function rows"))
        for name, arm, off, _ in others:
            with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_%s: this batch has coarse frames armed \(lbm_batch_set_coarse_frames\)" % name):
                arm()
            off()                                                       # disarming another kind leaves the coarse frames alone
        with pytest.raises(lbm.LbmError, match="lbm_set_coarse_frames: not available on a member of a batch"):
            m.set_coarse_frames(10, 4)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_run_until: coarse frames are armed \(lbm_batch_set_coarse_frames\)"):
            batch.run_until(100, 10)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_run_until_residual: coarse frames are armed"):
            batch.run_until_residual(100, 10, 1e-3)
        batch.run(6)                         # 30
        batch.set_coarse_frames(10, 2, 8)    # re-arming, with another box, discards the unread frame
        assert batch.coarse_frames()[0].size == 0
        batch.run(10)                        # 40
        steps, frames = batch.coarse_frames()
        assert steps.tolist() == [40] and frames.shape == (1, 3, 2, 16)
        batch.set_coarse_frames(0)           # disarms and frees
        # the other way round
        m.set_mean(10)
        with pytest.raises(lbm.LbmError, match="lbm_batch_set_coarse_frames: member 2 has mean fields armed"):
            batch.set_coarse_frames(10, 4)
        m.set_mean(0)
        for name, arm, off, words in others:
            arm()
            with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_coarse_frames: this batch has %s armed \(lbm_batch_set_%s\)" % (words, name)):
                batch.set_coarse_frames(10, 4)
            batch.set_coarse_frames(0)       # ... and leaves the other kind alone
            off()
        assert done() == [41, 41, 41, 41]


def test_batch_refuses_a_box_side_above_the_limit(lbm):
    """members wide enough for bx to pass LBM_COARSE_MAX_BOX: the message names the side and the limit; the limit itself arms"""
    params, obstacles, cells = random_members(lbm, 300, 8, 2, 31)
    with lbm.Batch(params, obstacles, cells) as batch:
        assert batch.lib.lbm_batch_set_coarse_frames(batch.handle, 1, 4, 257, 4) != 0
        assert batch.lib.lbm_last_error().decode().startswith("lbm_batch_set_coarse_frames: box side bx 257 is larger than LBM_COARSE_MAX_BOX (256)")
        batch.set_coarse_frames(1, 2, (256, 4))
        batch.run(1)
        steps, frames = batch.coarse_frames()
        assert steps.tolist() == [0] and frames.shape == (1, 2, 2, 2)
        assert frames[0, 0].tobytes() == batch.member(0).coarse((256, 4)).tobytes()


# ---- the ring -----------------------------------------------------------------------------------------------------------
def test_ring_overflow_drain_order_query_rearm_disarm(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        n = eng.lib.lbm_read_coarse_frames
        eng.set_coarse_frames(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_run: 25 steps would record 3 frames.*holds 2.*lbm_read_coarse_frames"):
            eng.run(25)                      # frames at 0, 10, 20
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match="2 frames are waiting"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        waiting = ctypes.c_int(-1)
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # the query form
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # ... drains nothing
        steps, first = eng.coarse_frames(1)
        assert steps.tolist() == [0] and first.shape == (1, 8, 8)                                    # oldest first
        eng.run(10)                          # 20 goes into the slot that 0 left
        steps, frames = eng.coarse_frames()
        assert steps.tolist() == [10, 20] and frames[0]["sum_jx"][6, 5] != frames[1]["sum_jx"][6, 5] and first[0]["sum_jx"][6, 5] != frames[1]["sum_jx"][6, 5]
        eng.run(6)                           # 30
        eng.set_coarse_frames(10, 2, (100, 3))   # re-arming, with another box, discards the unread frame
        assert eng.coarse_frames()[0].size == 0
        eng.run(10)                          # 40
        steps, frames = eng.coarse_frames()
        assert steps.tolist() == [40] and frames.shape == (1, 43, 2)
        assert frames[0].tobytes() == eng.coarse((100, 3)).tobytes()
        eng.set_coarse_frames(0)             # disarms and frees
        eng.run(30)
        steps, frames = eng.coarse_frames()
        assert steps.size == 0 and frames.shape[0] == 0
        assert eng.info()["steps_done"] == 71
        with pytest.raises(lbm.LbmError, match="coarse_frames: max_frames must be"):
            eng.coarse_frames(-1)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(lbm):
    p, ob, cells = random_case(lbm, 300, 128, 4, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        frame_bytes = 300 * 128 * 48                                       # boxes of one cell
        too_many = -(-2 ** 31 // frame_bytes)                              # the first capacity of 2 GiB or more
        set_ = "lbm_set_coarse_frames: "
        for every, cap, bx, by, msg in ((-1, 4, 16, 16, set_ + "negative interval -1"), (1, 0, 16, 16, set_ + "capacity 0, at least one frame"),
                                        (1, -2, 16, 16, set_ + "capacity -2"), (1, 4, 0, 16, set_ + "box 0 x 16, a box side is at least 1"),
                                        (1, 4, 16, 0, set_ + "box 16 x 0, a box side is at least 1"), (1, 4, -3, 16, set_ + "box -3 x 16"),
                                        (1, 4, 301, 16, set_ + "box side bx 301 is larger than the grid's nx 300"),
                                        (1, 4, 16, 129, set_ + "box side by 129 is larger than the grid's ny 128"),
                                        (1, 4, 257, 16, set_ + "box side bx 257 is larger than LBM_COARSE_MAX_BOX (256)"),
                                        (1, too_many, 1, 1, set_ + "a ring of %d frames is 2 GiB or more (%d bytes per frame and slab)" % (too_many, frame_bytes))):
            assert eng.lib.lbm_set_coarse_frames(eng.handle, every, cap, bx, by) != 0
            assert msg in eng.lib.lbm_last_error().decode()
        eng.set_coarse_frames(1, too_many - 1, 1)                           # the last capacity below 2 GiB is taken (the ring is allocated)
        eng.set_coarse_frames(0)
        line = np.zeros(1, dtype=lbm.PROFILE_DTYPE)
        for bx, by, msg in ((0, 1, "box 0 x 1, a box side is at least 1"), (301, 1, "box side bx 301 is larger than the grid's nx 300"),
                            (257, 1, "box side bx 257 is larger than LBM_COARSE_MAX_BOX (256)")):
            assert eng.lib.lbm_read_coarse(eng.handle, bx, by, line.ctypes.data) != 0
            assert "lbm_read_coarse: " + msg in eng.lib.lbm_last_error().decode()
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
                                  (lambda: eng.set_enstrophy(10, 4), lambda: eng.set_enstrophy(0), "enstrophy rows"),
                                  (lambda: eng.set_psi(10, 4), lambda: eng.set_psi(0), "stream function rows")):
            arm()
            with pytest.raises(lbm.LbmError, match="lbm_set_coarse_frames: %s are armed" % name):
                eng.set_coarse_frames(10, 4)
            disarm()
            eng.set_coarse_frames(10, 4)
            with pytest.raises(lbm.LbmError, match=r"coarse frames are armed \(lbm_set_coarse_frames\)"):
                arm()
            eng.set_coarse_frames(0)
        eng.set_coarse_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_run_until: coarse frames are armed"):
            eng.run_until(100, 10)
        with pytest.raises(lbm.LbmError, match="lbm_run_until_residual: coarse frames are armed"):
            eng.run_until_residual(100, 10, 1e-3)
        assert eng.info()["steps_done"] == 0
    tall = small(lbm, 20, 300)                                              # a grid on which by can pass the limit
    with lbm.Engine(*tall) as eng:
        assert eng.lib.lbm_set_coarse_frames(eng.handle, 1, 4, 4, 257) != 0
        assert set_ + "box side by 257 is larger than LBM_COARSE_MAX_BOX (256)" in eng.lib.lbm_last_error().decode()
        eng.set_coarse_frames(1, 4, (4, 256))
    # a rank context (one rank, host message passing that is never called)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_set_coarse_frames: not available in a multi-process"):
            eng.set_coarse_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_read_coarse: not available in a multi-process"):
            eng.coarse(16)


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_coarse_frames: the context runs the %s halo mode" % mode):
                eng.set_coarse_frames(10, 4)
        eng.set_halo_mode("sync")
        eng.set_coarse_frames(10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match=r"lbm_set_halo_mode: coarse frames are armed \(lbm_set_coarse_frames\)"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0
