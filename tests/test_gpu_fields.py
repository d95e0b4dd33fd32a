"""Field frames (lbm_set_field_frames / Engine.set_field_frames): chosen ones of u_x, u_y, |u| and pressure over a window
after every global timestep tt with tt % every == 0, recorded by the running kernels.  Every value is bit-identical to the
oracle's final_state at that step; recording never changes the lattice, and av_vels stays bit-identical on the resident
path and equal to the run split at the sample steps on the per-pass paths."""
import numpy as np
import pytest

import test_frames_format as model
from fields_model import FIELDS, assert_field_frames, oracle_field_frames
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_engine(lbm, p, ob, cells, calls, every=0, fields=FIELDS, window=None, capacity=0, n_gpus=1):
    """Run `calls` from step 0, field frames armed before the first call; drain after each call."""
    steps, frames = [], []
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        if every:
            eng.set_field_frames(every, capacity or 1 + sum(calls) // every, fields, window)
        for n in calls:
            eng.run(n)
            if every:
                s, f = eng.field_frames()
                steps.append(s)
                frames.append(f)
        info = eng.info()
        got = {k: np.concatenate([f[k] for f in frames]) for k in frames[0]} if frames else {}
        return eng.cells(), eng.av_vels(sum(calls)), np.concatenate(steps) if steps else np.zeros(0, np.int32), got, info


class Shared:
    """The oracle's per-step states and the unarmed engine run of one resident case, computed once and shared by the
    windows (and field subsets) of that case; nothing changes them."""
    cache = {}

    @classmethod
    def get(cls, key, make):
        if key not in cls.cache:
            cls.cache[key] = make()
        return cls.cache[key]


def cut(want_full, fields, window, p):
    x0, y0, wnx, wny = window or (0, 0, p.nx, p.ny)
    return {tt: {k: f[k][y0:y0 + wny, x0:x0 + wnx] for k in FIELDS if k in fields} for tt, f in want_full.items()}


RESIDENT_SHAPES = {"128x16": (128, 16, {}), "128x64-rows4": (128, 64, {"LBM_RESIDENT_ROWS": "4"}),
                   "320x24-rows2": (320, 24, {"LBM_RESIDENT_JOINT": "1"}), "1024x64": (1024, 64, {}),   # (JOINT is four-row only)
                   "128x128-group4": (128, 128, {"LBM_RESIDENT_ONE_XCD": "0", "LBM_RESIDENT_GROUP": "4"})}


def resident_windows(nx, ny):
    return {"whole": None, "column": (37, 0, 1, ny), "lid-row": (0, ny - 2, nx, 1), "rows-1-2": (5, 1, nx - 9, 2),
            "rows-3-4": (0, 3, nx, 2), "to-last-cell": (nx - 21, ny - 7, 21, 7), "misses-lid-band": (3, 2, 50, ny - 10)}


def resident_case(lbm, oracle, monkeypatch, shape):
    """The random lattice of test_gpu_frames.test_resident_random_lattices at this shape, the oracle's full-grid field
    frames for calls [1, 2, 19, 5] at every = 3, and the unarmed engine run."""
    nx, ny, env = RESIDENT_SHAPES[shape]
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    calls, every = [1, 2, 19, 5], 3

    def make():
        p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
        ob[ny - 2, ::5] = 1                     # lid row
        ob[3::4, ::7] = 1                       # seam rows of four-row bands
        ob[0::4, 3::7] = 1
        ref, want = oracle_field_frames(oracle, p, ob, cells, 0, sum(calls), every, FIELDS, None)
        base, base_av, _, _, info = run_engine(lbm, p, ob, cells, calls)
        assert info["resident_steps"] > 0
        return p, ob, cells, ref, want, base, base_av
    return Shared.get(shape, make) + (calls, every)


def check_resident(lbm, case, fields, window):
    p, ob, cells, ref, want, base, base_av, calls, every = case
    got, av, steps, frames, info = run_engine(lbm, p, ob, cells, calls, every, fields, window)
    assert info["resident_steps"] > 0
    assert_field_frames(steps, frames, cut(want, fields, window, p), fields)
    assert np.array_equal(bits(ref), bits(got))
    assert np.array_equal(bits(base), bits(got))
    assert np.array_equal(bits(base_av), bits(av)), "field frames changed av_vels on the resident path"


@pytest.mark.parametrize("win", ["whole", "column", "lid-row", "rows-1-2", "rows-3-4", "to-last-cell", "misses-lid-band"])
@pytest.mark.parametrize("shape", list(RESIDENT_SHAPES))
def test_resident_random_lattices(lbm, oracle, monkeypatch, shape, win):
    """Shapes 1, 3, 1, 0 and 1 of the resident kernel (tests/resident_forms.py): two-row bands; four-row JOINT bands (the
    rows4 case, the only four-row one); two-row bands again at 320 x 24, where LBM_RESIDENT_JOINT=1 has no say; MAXT = 1024
    with two-row bands; grouped workgroups.  Windows that are the whole grid, one column at an odd x, the lid row, the
    interior pair of a four-row band, the top edge of one band and the bottom edge of the next, a rectangle that ends at
    the last column and row, and one that misses the lid row's band.  Shapes 2 and 4: tests/test_gpu_resident_forms.py."""
    case = resident_case(lbm, oracle, monkeypatch, shape)
    nx, ny, _ = RESIDENT_SHAPES[shape]
    check_resident(lbm, case, FIELDS, resident_windows(nx, ny)[win])


@pytest.mark.parametrize("fields", [("u_x",), ("u_y",), ("u",), ("pressure",), ("u_x", "u_y"), ("u_x", "pressure")])
@pytest.mark.parametrize("shape", ["128x16", "128x64-rows4"])
def test_field_subsets(lbm, oracle, monkeypatch, shape, fields):
    """Each subset plane by plane, in order, against the all-fields run (and so against the model)."""
    case = resident_case(lbm, oracle, monkeypatch, shape)
    p, ob, cells, calls, every = case[0], case[1], case[2], case[-2], case[-1]
    window = (11, 1, 70, p.ny - 3)
    all_steps, all_frames = Shared.get((shape, "all-fields"), lambda: run_engine(lbm, p, ob, cells, calls, every, FIELDS, window)[2:4])
    _, _, steps, frames, _ = run_engine(lbm, p, ob, cells, calls, every, fields, window)
    assert steps.tolist() == all_steps.tolist() and len(steps) == 9
    assert list(frames) == list(fields)
    for k in fields:
        assert np.array_equal(bits(frames[k]), bits(all_frames[k])), k
    check_resident(lbm, case, fields, window)


@pytest.mark.parametrize("every", [4095, 4096])
def test_resident_chunk_boundary(lbm, oracle, every):
    """A 4100-step call runs two launches (4096 + 4): a sample on the last step of the first (accel_last) and on the
    first step of the second."""
    def make():
        p, ob, cells = random_case(lbm, 128, 128, 5, walls=False)
        p.max_iters = 4100
        states = {}
        ref = cells.copy()
        done = 0
        for tt in (0, 4095, 4096):
            oracle.run(p, ref, ob, tt + 1 - done)
            done = tt + 1
            states[tt] = {k: v.copy() for k, v in oracle.final_state(p, ref, ob).items()}
        oracle.run(p, ref, ob, 4100 - done)
        base, base_av, _, _, _ = run_engine(lbm, p, ob, cells, [4100])
        return p, ob, cells, ref, states, base, base_av
    p, ob, cells, ref, states, base, base_av = Shared.get("chunk", make)
    window = (9, 100, 100, 28)
    want = {tt: states[tt] for tt in model.frame_steps(0, 4100, every)}
    check_resident(lbm, (p, ob, cells, ref, want, base, base_av, [4100], every), FIELDS, window)


def test_arming_mid_run_uses_global_steps(lbm, oracle):
    p, ob, cells = random_case(lbm, 128, 128, 9, walls=False)
    p.max_iters = 431
    window = (100, 90, 28, 38)
    ref = cells.copy()
    oracle.run(p, ref, ob, 130)
    _, want = oracle_field_frames(oracle, p, ob, ref, 130, 431, 100, FIELDS, window)
    with lbm.Engine(p, ob, cells) as eng:
        eng.run(130)
        eng.set_field_frames(100, 3, window=window)
        eng.run(301)
        steps, frames = eng.field_frames()
    assert steps.tolist() == [200, 300, 400]
    assert_field_frames(steps, frames, want)


PER_PASS = {"LBM_RESIDENT": "0", "LBM_TILE_STEPS": "0", "LBM_GRAPH": "0"}


@pytest.mark.parametrize("env,n_gpus,every,launch", [
    (dict(PER_PASS, LBM_FUSE2="1"), 1, 25, (2, 3)),                                   # stream kernel, K = 2 / 3
    (dict(PER_PASS, LBM_FUSE2="1", LBM_PASS_STEPS="4", LBM_LANE_CELLS="4"), 1, 25, (4,)),  # K = 4, packed
    (dict(PER_PASS, LBM_FUSE2="0"), 1, 25, (1,)),                                     # one-step kernel
    (dict(PER_PASS, LBM_TILE_STEPS="4"), 1, 25, (4,)),                                # LDS-tile kernel
    (dict(PER_PASS, LBM_GRAPH="1"), 1, 150, None),     # segments of 94 and 109 steps: hipGraph chunks are replayed
    ({"LBM_HALO": "memcpy"}, 2, 25, None), ({"LBM_HALO": "memcpy"}, 3, 25, None)])
def test_per_pass_families(lbm, oracle, monkeypatch, env, n_gpus, every, launch):
    """Calls the resident kernel does not serve end their passes at every sample step: frames match the model, the lattice
    and av_vels match the same run issued as calls split at the sample steps.  One window spans the slab seam(s) (rows 48
    of two slabs, 32 and 64 of three), one lies inside the first slab, so the other slabs record nothing."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    calls = [57, 203]

    def make():
        p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
        wants = {e: oracle_field_frames(oracle, p, ob, cells, 0, sum(calls), e, FIELDS, None) for e in (25, 150)}
        return p, ob, cells, wants
    p, ob, cells, wants = Shared.get("per-pass", make)
    ref, want = wants[every]
    split = model.split_calls(calls, every)
    base, base_av, _, _, _ = run_engine(lbm, p, ob, cells, split, n_gpus=n_gpus)
    for window in ((13, 20, 101, 60), (0, 5, 128, 20)):
        got, av, steps, frames, info = run_engine(lbm, p, ob, cells, calls, every, FIELDS, window, n_gpus=n_gpus)
        assert info["resident_steps"] == 0 and info["n_slabs"] == n_gpus
        if launch:
            assert info["steps_per_launch"] in launch, info
        if env.get("LBM_GRAPH") == "1":
            assert info["graph_steps"] > 0 and info["graph_steps"] < 94, info
        assert_field_frames(steps, frames, cut(want, FIELDS, window, p))
        assert np.array_equal(bits(ref), bits(got))
        assert np.array_equal(bits(base), bits(got))
        assert np.array_equal(bits(base_av), bits(av))


def batch_inputs(lbm, seed):
    p0, ob0, c0 = random_case(lbm, 128, 128, seed, walls=False)
    params = [lbm.Params(128, 128, 400, 10, 0.1, float(np.float32(0.004 + 0.001 * i)), float(np.float32(1.6 + 0.03 * i)))
              for i in range(8)]
    return params, [np.roll(ob0, i, axis=1) for i in range(8)], [np.roll(c0, i, axis=0) for i in range(8)]


def test_batch_members_armed_independently(lbm, oracle):
    params, obstacles, cells = batch_inputs(lbm, 31)
    armed = {0: (50, ("u_x", "u_y"), (64, 0, 1, 128)), 3: (7, ("u", "pressure"), (90, 101, 38, 27))}
    calls = [120, 180]
    with lbm.Batch(params, obstacles, cells) as plain, lbm.Batch(params, obstacles, cells) as batch:
        assert batch.info()["resident_steps"] > 0
        for i, (e, fields, window) in armed.items():
            batch.member(i).set_field_frames(e, 1 + sum(calls) // e, fields, window)
        for n in calls:
            plain.run(n)
            batch.run(n)
        for i in range(8):
            m, q = batch.member(i), plain.member(i)
            assert np.array_equal(bits(m.cells()), bits(q.cells())), i
            assert np.array_equal(bits(m.av_vels()), bits(q.av_vels())), i
            if i in armed:
                e, fields, window = armed[i]
                steps, frames = m.field_frames()
                _, want = oracle_field_frames(oracle, params[i], obstacles[i], cells[i], 0, sum(calls), e, fields, window)
                assert_field_frames(steps, frames, want, fields)
                s_steps, s_frames = run_engine(lbm, params[i], obstacles[i], cells[i], calls, e, fields, window)[2:4]
                assert s_steps.tolist() == steps.tolist()
                for k in fields:
                    assert np.array_equal(bits(s_frames[k]), bits(frames[k])), (i, k)
            else:
                assert m.field_frames()[0].size == 0


def test_batch_short_call_then_resident(lbm, oracle):
    """A call below resident_min_steps runs the members one by one on the per-pass kernels; an armed member's call is
    split at its sample steps.  The next batched resident call must still take every member's lattice where it lies."""
    params, obstacles, cells = batch_inputs(lbm, 41)
    calls = [2, 300, 3, 95]
    window = (17, 60, 64, 9)
    with lbm.Batch(params, obstacles, cells) as plain, lbm.Batch(params, obstacles, cells) as batch:
        assert batch.info()["resident_steps"] > 0 and batch.info()["resident_min_steps"] > 3
        batch.member(3).set_field_frames(100, 8, FIELDS, window)
        for n in calls:
            plain.run(n)
            batch.run(n)
        for i in range(8):
            ref = cells[i].copy()
            oracle.run(params[i], ref, obstacles[i], sum(calls))
            assert np.array_equal(bits(batch.member(i).cells()), bits(ref)), i
            assert np.array_equal(bits(batch.member(i).cells()), bits(plain.member(i).cells())), i
        steps, frames = batch.member(3).field_frames()
        _, want = oracle_field_frames(oracle, params[3], obstacles[3], cells[3], 0, sum(calls), 100, FIELDS, window)
        assert_field_frames(steps, frames, want)
        s_steps, s_frames = run_engine(lbm, params[3], obstacles[3], cells[3], calls, 100, FIELDS, window)[2:4]
        for k in FIELDS:
            assert np.array_equal(bits(s_frames[k]), bits(frames[k])), k


def test_capacity_overflow_fails_before_any_work(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_field_frames(10, 2, window=(1, 2, 30, 4))
        with pytest.raises(lbm.LbmError, match="lbm_run: 25 steps would record 3 field frames, but the field frame buffer holds 2"):
            eng.run(25)                      # frames at 0, 10, 20
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match=r"2 field frames are waiting \(lbm_read_field_frames drains them\)"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        steps, _ = eng.field_frames(1)
        assert steps.tolist() == [0]
        eng.run(10)                          # 20
        assert eng.field_frames()[0].tolist() == [10, 20]
        eng.set_field_frames(0)
        eng.run(30)
        assert eng.field_frames()[0].size == 0


def refuse_field_frames(lbm, eng):
    """One hipMalloc of about 512 TiB (2^31 - 1 slots of four 128 x 128 planes): the runtime refuses it at once with an
    out-of-memory return code, and nothing faults."""
    with pytest.raises(lbm.LbmError, match=r"lbm_set_field_frames: cannot allocate 2147483647 frame slots .* MiB per slab\); field frames stay off"):
        eng.set_field_frames(1, 2**31 - 1)


def test_failed_allocation_leaves_the_engine_whole(lbm, oracle, datasets):
    """lbm_set_field_frames whose ring cannot be allocated returns an error and leaves nothing behind: the same engine
    runs on, bit-identical to the oracle and to an engine that was never asked, and arms again."""
    p, ob = datasets("128x128")
    cells = oracle.init_cells(p)
    window = (0, 120, 128, 8)
    ref, _ = oracle_field_frames(oracle, p, ob, cells, 0, 40, 10, FIELDS, window)
    ref80, want80 = oracle_field_frames(oracle, p, ob, ref, 40, 80, 10, FIELDS, window)
    with lbm.Engine(p, ob, cells) as plain:
        plain.run(40)
        plain_av = plain.av_vels(40)
    with lbm.Engine(p, ob, cells) as eng:
        refuse_field_frames(lbm, eng)
        eng.run(40)
        assert np.array_equal(bits(eng.cells()), bits(ref))
        assert np.array_equal(bits(eng.av_vels(40)), bits(plain_av)), "the refusal changed av_vels"
        assert eng.field_frames()[0].size == 0
        eng.set_frames(10, 4)                # no recorder is armed: another kind may arm
        eng.set_frames(0)
        eng.set_field_frames(10, 4, window=window)
        eng.run(40)
        steps, frames = eng.field_frames()
        assert steps.tolist() == [40, 50, 60, 70]
        assert_field_frames(steps, frames, want80)
        assert np.array_equal(bits(eng.cells()), bits(ref80))


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_field_frames.*halo mode"):
                eng.set_field_frames(10, 4)
        eng.set_halo_mode("sync")
        eng.set_field_frames(10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match="lbm_set_halo_mode: field frames are armed"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0


def test_one_recorder_per_context_and_no_steady_runs(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_field_frames: animation frames are armed"):
            eng.set_field_frames(10, 4)
        eng.set_frames(0)
        eng.set_probes([(5, 5)], 1, 16)
        with pytest.raises(lbm.LbmError, match="lbm_set_field_frames: point probes are armed"):
            eng.set_field_frames(10, 4)
        eng.set_probes([], 0, 0)
        eng.set_mean(10)
        with pytest.raises(lbm.LbmError, match="lbm_set_field_frames: mean fields are armed"):
            eng.set_field_frames(10, 4)
        eng.set_mean(0)
        eng.set_field_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_frames: field frames are armed"):
            eng.set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_probes: field frames are armed"):
            eng.set_probes([(5, 5)], 1, 16)
        with pytest.raises(lbm.LbmError, match="lbm_set_mean: field frames are armed"):
            eng.set_mean(10)
        with pytest.raises(lbm.LbmError, match="lbm_run_until: field frames are armed"):
            eng.run_until(100, 10)
        assert eng.info()["steps_done"] == 0
        eng.run(11)
        assert eng.field_frames()[0].tolist() == [0, 10]      # still armed through all of it


def test_a_batch_records_one_kind(lbm):
    params, obstacles, cells = batch_inputs(lbm, 7)
    with lbm.Batch(params[:3], obstacles[:3], cells[:3]) as batch:
        batch.member(1).set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_field_frames: a member of this batch has animation frames armed"):
            batch.member(0).set_field_frames(10, 4)
        batch.member(1).set_frames(0)
        batch.member(0).set_field_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_mean: a member of this batch has field frames armed"):
            batch.member(2).set_mean(10)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run_until: field frames are armed"):
            batch.run_until(100, 10)
        assert batch.member(1).field_frames()[0].size == 0


def test_bad_arguments_and_rank_contexts_are_refused(lbm):
    """What the library itself refuses, each under the function's name, with the context left as it was."""
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    win = lbm._CWindow
    with lbm.Engine(p, ob, cells) as eng:
        lib, h = eng.lib, eng.handle
        eng.set_field_frames(10, 4, ("u",), (1, 2, 3, 4))
        for args, msg in (((-1, 4, 15, None), b"negative interval"), ((10, 0, 15, None), b"capacity 0"),
                          ((10, 4, 0, None), b"fields 0x0"), ((10, 4, 16, None), b"fields 0x10"), ((10, 4, -1, None), b"fields"),
                          ((10, 4, 15, win(0, 0, 0, 5)), b"window of 0 x 5"), ((10, 4, 15, win(0, 0, 5, -1)), b"window of 5 x -1"),
                          ((10, 4, 15, win(-1, 0, 5, 5)), b"leaves the 128 x 128 grid"),
                          ((10, 4, 15, win(124, 0, 5, 5)), b"leaves the 128 x 128 grid"),
                          ((10, 4, 15, win(0, 127, 5, 2)), b"leaves the 128 x 128 grid"),
                          ((10, 4, 15, win(1, 1, 2147483647, 1)), b"leaves the 128 x 128 grid")):
            every, capacity, fields, window = args
            assert lib.lbm_set_field_frames(h, every, capacity, fields, window) != 0, args
            err = lib.lbm_last_error()
            assert err.startswith(b"lbm_set_field_frames:") and msg in err, (args, err)
        eng.run(11)                          # the armed recorder is untouched by the refusals
        steps, frames = eng.field_frames()
        assert steps.tolist() == [0, 10] and list(frames) == ["u"] and frames["u"].shape == (2, 4, 3)
        with pytest.raises(lbm.LbmError, match="leaves the 128 x 128 grid"):
            eng.set_field_frames(10, 4, window=(0, 0, 129, 1))
    # a rank context (one rank, host message passing that is never called)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_set_field_frames: not available in a multi-process"):
            eng.set_field_frames(10, 4)
        eng.set_field_frames(0)              # disarming is not arming


def test_cli_writes_state_files(lbm, oracle, datasets, tmp_path):
    """d2q9-bgk with LBM_STATES=50 on 128^2 for 251 steps: state_data/final_state_%06d.dat for tt = 0, 50, ..., 250, each
    byte-identical to the Python twin fed with the model's frame, the last one to the run's own final_state.dat;
    final_state.dat and av_vels.dat as without it.  With a window: the window's lines only."""
    import hashlib
    import os
    import subprocess
    from conftest import GOLDEN
    p, ob = datasets("128x128")
    p.max_iters = 251
    of = os.path.join(GOLDEN, "inputs", "obstacles_128x128.dat")
    window = (100, 3, 20, 9)
    outs = {}
    for label, extra in (("plain", {}), ("states", {"LBM_STATES": "50"}), ("window", {"LBM_STATES": "50:%d,%d,%d,%d" % window})):
        d = tmp_path / label
        d.mkdir()
        pf = d / "input.params"
        pf.write_text("%d\n%d\n%d\n%d\n%.9g\n%.9g\n%.9g\n" % (p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel,
                                                           p.omega))
        env = {k: v for k, v in os.environ.items() if k != "LBM_STATES"}
        out = subprocess.run([lbm.CLI_PATH, str(pf), of], cwd=d, capture_output=True, text=True, env=dict(env, **extra), timeout=120)
        assert out.returncode == 0, out.stderr
        outs[label] = (d, out.stdout)
    tts = (0, 50, 100, 150, 200, 250)
    for label in ("states", "window"):
        d, stdout = outs[label]
        for name in ("final_state.dat", "av_vels.dat"):
            md5 = [hashlib.md5((outs[k][0] / name).read_bytes()).hexdigest() for k in ("plain", label)]
            assert md5[0] == md5[1], (label, name)
        assert [l for l in stdout.splitlines() if l.startswith("Written state")] == ["Written state data for timestep %d" % tt for tt in tts]
        assert sorted(os.listdir(d / "state_data")) == ["final_state_%06d.dat" % tt for tt in tts]
    assert not (outs["plain"][0] / "state_data").exists()
    d = outs["states"][0]
    assert (d / "state_data" / "final_state_000250.dat").read_bytes() == (d / "final_state.dat").read_bytes()
    _, want = oracle_field_frames(oracle, p, ob, oracle.init_cells(p), 0, 251, 50, FIELDS, None)
    for label, win in (("states", (0, 0, p.nx, p.ny)), ("window", window)):
        for tt in tts:
            twin = tmp_path / ("twin_%s_%d.dat" % (label, tt))
            lbm.write_state_frame(str(twin), cut({tt: want[tt]}, FIELDS, win, p)[tt], ob, win)
            got = (outs[label][0] / "state_data" / ("final_state_%06d.dat" % tt)).read_bytes()
            assert got == twin.read_bytes(), (label, tt)
            assert got.count(b"\n") == win[2] * win[3]
