"""Obstacle forces (lbm_set_forces / Engine.set_forces): the momentum the populations on the boundary links handed to
the solid, per body, after every global timestep tt with tt % every == 0.  Every row is compared with the numpy model
(tests/forces_model.py) over the oracle's lattice of that step, within n_links * 2^-52 * sum |term| per component -- the
distance any double sum of the terms may have from their exact sum -- and, since the engine takes the exact sum and rounds
once, it must also be the model's value itself.  All kernel paths, call splittings and slab counts give the same bits;
recording never changes the lattice, and av_vels equals that of the same run issued as calls split at the sample steps."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import forces_model
import test_frames_format as model
from cli_case import obstacles_text, params_text, run_cli
from conftest import GOLDEN
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def run_engine(lbm, p, ob, cells, calls, every=0, bodies=None, n_bodies=None, capacity=0, n_gpus=1, unarmed_first=0, tiled=False):
    """`unarmed_first` steps, then forces armed, then `calls`, drained after each: (lattice, av_vels, steps, rows, links, info)"""
    steps, rows, links = [], [], None
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus, tiled=tiled) as eng:
        if unarmed_first:
            eng.run(unarmed_first)
        if every:
            eng.set_forces(every, capacity or 1 + sum(calls) // every, bodies, n_bodies)
            links = eng.force_links()
        for n in calls:
            eng.run(n)
            if every:
                s, r = eng.forces()
                steps.append(s)
                rows.append(r)
        info = eng.info()
        total = unarmed_first + sum(calls)
        return (eng.cells(), eng.av_vels(total), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(rows) if rows else np.zeros((0, 0, 2)), links, info)


def assert_rows(steps, rows, want):
    """want: {tt: (force [n_bodies, 2], bound [n_bodies, 2])} of forces_model.oracle_forces"""
    assert steps.tolist() == sorted(want)
    for tt, row in zip(steps.tolist(), rows):
        f, limit = want[tt]
        assert row.shape == f.shape
        err = np.abs(row - f)
        print("step", tt, "max |F_gpu - F_model|", err.max(), "bound", limit.max())
        assert np.all(err <= limit), (tt, row, f, limit)
        assert np.array_equal(bits(row), bits(f)), (tt, row, f)      # the exact sum, rounded once


def check(lbm, oracle, p, ob, cells, calls, every, bodies=None, n_bodies=1, unarmed_first=0, n_gpus=1, want=None, ref=None):
    """armed run against the model and the oracle's lattice; av_vels against the unarmed run split at the sample steps"""
    if want is None:
        start = cells.copy()
        oracle.run(p, start, ob, unarmed_first)
        ref, want = forces_model.oracle_forces(oracle, p, ob, start, unarmed_first, sum(calls), every, bodies, n_bodies)
    got, av, steps, rows, links, info = run_engine(lbm, p, ob, cells, calls, every, bodies, n_bodies, n_gpus=n_gpus,
                                                   unarmed_first=unarmed_first)
    assert links.tolist() == forces_model.link_counts(ob, bodies, n_bodies)
    assert_rows(steps, rows, want)
    assert np.array_equal(bits(ref), bits(got)), "recording changed the lattice"
    # calls cut after every sample step, counted in global steps
    split, done = [], 0
    for n in [unarmed_first] + list(calls):
        end = done + n
        for c in [tt + 1 for tt in model.frame_steps(done, end, every) if tt >= unarmed_first] + [end]:
            if c > done:
                split.append(c - done)
                done = c
    base, base_av, _, _, _, _ = run_engine(lbm, p, ob, cells, split, n_gpus=n_gpus)
    assert np.array_equal(bits(base), bits(got))
    assert np.array_equal(bits(base_av), bits(av)), "recording changed av_vels"
    return steps, rows, info


def small(lbm, nx, ny, seed=1):
    rng = np.random.default_rng(seed)
    p = lbm.Params(nx, ny, 400, 10, 0.1, 0.005, 1.85)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32) * np.float32(p.density)
    cells = (w * (1.0 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    return p, np.zeros((ny, nx), dtype=np.int32), cells


# ---- shapes: the smallest at which the list builders and force_gather can go wrong ------------------------------------
def test_one_block_under_one_wave(lbm, oracle):
    p, ob, cells = small(lbm, 16, 8)
    ob[3:5, 6:8] = 1
    steps, rows, _ = check(lbm, oracle, p, ob, oracle.init_cells(p), [20], 1)
    assert forces_model.link_counts(ob) == [20] and len(steps) == 20
    assert rows[-1, 0, 0] > 0.0                                       # the accelerated flow pushes the block downstream
    check(lbm, oracle, p, ob, cells, [7], 2)


def test_blocked_cells_on_all_four_edges(lbm, oracle):
    """links over the x wrap, the y wrap (the mask's halo rows of a single slab) and both"""
    p, ob, cells = small(lbm, 16, 8, 2)
    ob[0, 0] = ob[7, 15] = ob[0, 9] = ob[7, 4] = ob[3, 0] = ob[5, 15] = 1
    check(lbm, oracle, p, ob, cells, [9], 2)


@pytest.mark.parametrize("segments,more_than", [([(2, 10, 21)], 64), ([(1, 3, 60), (4, 70, 129)], 256), ([(1, 0, 130), (3, 1, 93), (5, 7, 130)], 1024)])
def test_wave_and_workgroup_edges(lbm, oracle, segments, more_than):
    """130 x 6 (nx no multiple of 4) with blocked runs along x: more than one wave of links with a ragged last wave, more
    than one workgroup's lanes, and more than one workgroup per body"""
    p, ob, cells = small(lbm, 130, 6, 3)
    for y, x0, x1 in segments:
        ob[y, x0:x1] = 1
    n = forces_model.link_counts(ob)[0]
    assert n > more_than and n % 64 != 0
    check(lbm, oracle, p, ob, cells, [5], 2)


def test_several_workgroups_per_body_and_a_body_without_links(lbm, oracle):
    p, ob, cells = small(lbm, 128, 32, 4)
    ob[2:30:2, 4:124:2] = 1                  # body 0: 14 x 60 isolated cells, 8 links each
    ob[13:16, 61:64] = 1                     # a solid 3 x 3 block: body 1 its rim, body 2 its enclosed centre
    bodies = np.zeros_like(ob)
    bodies[13:16, 61:64] = 1
    bodies[14, 62] = 2
    counts = forces_model.link_counts(ob, bodies, 3)
    assert counts[0] > 4 * 1024 and counts[1] > 0 and counts[2] == 0
    steps, rows, _ = check(lbm, oracle, p, ob, cells, [6], 3, bodies, 3)
    assert np.all(rows[:, 2, :] == 0.0) and not np.signbit(rows[:, 2, :]).any()
    assert np.all(rows[:, 1, :] != 0.0)


def test_max_bodies(lbm, oracle, monkeypatch):
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "2")
    p, ob, cells = small(lbm, 128, 16, 5)
    bodies = np.full_like(ob, -1)            # fluid cells carry a label outside the range: ignored
    for b in range(lbm.LBM_MAX_BODIES):
        y, x = 1 + 2 * (b // 16), 3 + 8 * (b % 16)
        ob[y, x:x + 1 + b % 3] = 1
        bodies[y, x:x + 1 + b % 3] = b
    steps, rows, info = check(lbm, oracle, p, ob, cells, [4, 9], 3, bodies, lbm.LBM_MAX_BODIES)
    assert rows.shape == (5, 64, 2) and info["resident_steps"] > 0


# ---- paths ------------------------------------------------------------------------------------------------------------
class Shared:
    """One case's oracle forces of EVERY step and its lattices, computed once; nothing changes them."""
    cache = {}

    @classmethod
    def get(cls, key, make):
        if key not in cls.cache:
            cls.cache[key] = make()
        return cls.cache[key]


RESIDENT_SHAPES = {"128x16": (128, 16, {}), "128x64-rows4": (128, 64, {"LBM_RESIDENT_ROWS": "4"})}


@pytest.mark.parametrize("min_steps", ["1", "3"])
@pytest.mark.parametrize("shape", list(RESIDENT_SHAPES))
def test_resident_shapes(lbm, oracle, monkeypatch, shape, min_steps):
    """Sub-calls of at least resident_min_steps run the resident kernel (its plain form), shorter ones the per-pass
    kernels; the rows are those of the per-pass kernels alone, bit for bit."""
    nx, ny, env = RESIDENT_SHAPES[shape]
    calls, every = [1, 2, 19, 5], 3

    def make():
        p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
        ob[ny - 2, ::5] = 1                     # lid row
        ob[3::4, ::7] = 1                       # seam rows of four-row bands
        ref, want = forces_model.oracle_forces(oracle, p, ob, cells, 0, sum(calls), every)
        return p, ob, cells, ref, want
    p, ob, cells, ref, want = Shared.get(shape, make)
    monkeypatch.setenv("LBM_RESIDENT", "0")
    plain = Shared.get((shape, "per-pass"), lambda: run_engine(lbm, p, ob, cells, calls, every)[3])
    monkeypatch.delenv("LBM_RESIDENT")
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", min_steps)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    steps, rows, info = check(lbm, oracle, p, ob, cells, calls, every, want=want, ref=ref)
    assert info["resident_steps"] > 0 and len(steps) == 9
    assert np.array_equal(bits(rows), bits(plain))


PER_PASS = {"LBM_RESIDENT": "0", "LBM_TILE_STEPS": "0", "LBM_GRAPH": "0"}
FAMILIES = {"stream": dict(PER_PASS, LBM_FUSE2="1"), "stream4": dict(PER_PASS, LBM_FUSE2="1", LBM_PASS_STEPS="4", LBM_LANE_CELLS="4"),
            "one-step": dict(PER_PASS, LBM_FUSE2="0"), "tile": dict(PER_PASS, LBM_TILE_STEPS="4"), "graph": dict(PER_PASS, LBM_GRAPH="1")}


def per_pass_case(lbm, oracle):
    """128 x 96, blocked cells on every slab's first and last row for 2 and 3 slabs; armed after 5 steps; the oracle's
    forces of every step from there"""
    def make():
        p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
        for parts in (2, 3):
            for first, count in (lbm.partition_rows(96, parts, s) for s in range(parts)):
                ob[first, 11:14] = ob[first + count - 1, 64] = ob[first + count - 1, 127] = ob[first, 0] = 1
        start = cells.copy()
        oracle.run(p, start, ob, 5)
        ref, all_steps = forces_model.oracle_forces(oracle, p, ob, start, 5, 63, 1)
        return p, ob, cells, ref, all_steps
    return Shared.get("per-pass", make)


@pytest.mark.parametrize("every", [1, 3, 4, 7])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_pass_families(lbm, oracle, monkeypatch, family, every):
    """Armed at step 5, no multiple of any `every`; every kernel family gives the rows of the model"""
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % every == 0}
    steps, rows, info = check(lbm, oracle, p, ob, cells, [23, 40], every, unarmed_first=5, want=want, ref=ref)
    assert info["resident_steps"] == 0 and steps[0] == (5 + every - 1) // every * every


@pytest.mark.parametrize("n_gpus", [2, 3])
def test_slabs(lbm, oracle, monkeypatch, n_gpus):
    """A link belongs to the slab of its blocked cell; its neighbour across the slab edge is read from the mask's halo
    rows.  The rows are those of one slab, bit for bit."""
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
    want = {tt: v for tt, v in all_steps.items() if tt % 4 == 0}
    one = Shared.get("one-slab", lambda: run_engine(lbm, p, ob, cells, [23, 40], 4, unarmed_first=5)[3])
    monkeypatch.setenv("LBM_HALO", "memcpy")
    steps, rows, info = check(lbm, oracle, p, ob, cells, [23, 40], 4, unarmed_first=5, n_gpus=n_gpus, want=want, ref=ref)
    assert info["n_slabs"] == n_gpus
    assert np.array_equal(bits(rows), bits(one))


def test_one_call_against_ragged_split_calls(lbm, oracle):
    p, ob, cells, ref, all_steps = per_pass_case(lbm, oracle)
    whole = run_engine(lbm, p, ob, cells, [63], 4, unarmed_first=5)
    ragged = run_engine(lbm, p, ob, cells, [1, 2, 13, 4, 30, 1, 12], 4, unarmed_first=5)
    assert whole[2].tolist() == ragged[2].tolist() == [tt for tt in range(5, 68) if tt % 4 == 0]
    assert np.array_equal(bits(whole[3]), bits(ragged[3]))
    assert np.array_equal(bits(whole[0]), bits(ragged[0])) and np.array_equal(bits(whole[0]), bits(ref))
    assert_rows(whole[2], whole[3], {tt: v for tt, v in all_steps.items() if tt % 4 == 0})


def test_tiled_context(lbm, oracle):
    """lbm_create_tiled: the list is built from the device's mask, no host map; two slabs, labels given"""
    p, tile, _ = small(lbm, 32, 16)
    tile[0, 0] = tile[15, 31] = tile[5:8, 9:12] = 1
    p = lbm.Params(128, 48, 400, 10, 0.1, 0.005, 1.85)
    ob = np.tile(tile, (3, 4))
    cells = small(lbm, 128, 48, 8)[2]
    bodies = (np.arange(48)[:, None] // 16 + 0 * ob).astype(np.int32)        # one body per row of tiles
    ref, want = forces_model.oracle_forces(oracle, p, ob, cells, 0, 9, 2, bodies, 3)
    for n_gpus in (1, 2):
        got, _, steps, rows, links, info = run_engine(lbm, p, tile, cells, [9], 2, bodies, 3, n_gpus=n_gpus, tiled=True)
        assert info["n_slabs"] == n_gpus and links.tolist() == forces_model.link_counts(ob, bodies, 3)
        assert_rows(steps, rows, want)
        assert np.array_equal(bits(ref), bits(got))


# ---- the ring ---------------------------------------------------------------------------------------------------------
def test_ring_overflow_drain_order_query_rearm_disarm(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        n = eng.lib.lbm_read_forces
        eng.set_forces(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_run: 25 steps would record 3 rows.*holds 2"):
            eng.run(25)                      # rows at 0, 10, 20
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match="2 rows are waiting"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        import ctypes
        waiting = ctypes.c_int(-1)
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # the query form
        assert n(eng.handle, 0, None, None, ctypes.byref(waiting)) == 0 and waiting.value == 2      # ... drains nothing
        steps, first = eng.forces(1)
        assert steps.tolist() == [0] and first.shape == (1, 1, 2)                                 # oldest first
        eng.run(10)                          # 20 goes into the slot that 0 left
        steps, rows = eng.forces()
        assert steps.tolist() == [10, 20] and not np.array_equal(rows[0], rows[1])
        eng.run(6)                           # 30
        eng.set_forces(10, 2)                # re-arming discards the unread row
        assert eng.forces()[0].size == 0
        eng.run(10)                          # 40
        assert eng.forces()[0].tolist() == [40]
        eng.set_forces(0)                    # disarms and frees
        with pytest.raises(lbm.LbmError, match="not armed"):
            eng.force_links()
        eng.run(30)
        assert eng.forces()[0].size == 0
        assert eng.info()["steps_done"] == 71


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 4, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        lab = np.zeros((128, 128), dtype=np.int32)
        for n_bodies, labels, every, cap, msg in ((0, None, 1, 4, "0 bodies, between 1 and LBM_MAX_BODIES = 64"),
                                                  (65, None, 1, 4, "65 bodies, between 1 and LBM_MAX_BODIES = 64"),
                                                  (1, None, -1, 4, "negative interval -1"), (1, None, 1, 0, "capacity 0, at least one row"),
                                                  (1, None, 1, -2, "capacity -2"), (64, None, 1, 2 ** 18, "2 GiB or more")):
            assert eng.lib.lbm_set_forces(eng.handle, n_bodies, labels, every, cap) != 0
            assert msg in eng.lib.lbm_last_error().decode()
        y, x = [int(v[0]) for v in np.nonzero(ob)]
        for bad in (2, -1):
            lab[y, x] = bad
            with pytest.raises(lbm.LbmError, match=r"the blocked cell \(%d, %d\) has body %d, outside 0 .. 1" % (x, y, bad)):
                eng.set_forces(10, 4, lab, 2)
        lab[y, x] = 1
        lab[ob == 0] = 77                      # fluid cells: ignored
        eng.set_forces(10, 4, lab, 2)
        assert eng.force_links().sum() == len(forces_model.links(ob))
        eng.set_forces(0)
        assert eng.info()["steps_done"] == 0
        # one recorder per context, both directions
        eng.set_frames(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_set_forces: animation frames are armed|lbm_set_forces: .*frames are armed"):
            eng.set_forces(10, 4)
        eng.set_frames(0)
        eng.set_forces(10, 4)
        for arm, disarm in ((lambda: eng.set_frames(10, 2), None), (lambda: eng.set_probes([(1, 1)], 1, 4), None),
                            (lambda: eng.set_mean(10), None), (lambda: eng.set_field_frames(10, 2), None)):
            with pytest.raises(lbm.LbmError, match=r"obstacle forces are armed \(lbm_set_forces\)"):
                arm()
        with pytest.raises(lbm.LbmError, match="lbm_run_until: obstacle forces are armed|obstacle forces are armed"):
            eng.run_until(100, 10)
        assert eng.info()["steps_done"] == 0
    with lbm.Batch([p, p], [ob, ob], [cells, cells]) as batch:
        with pytest.raises(lbm.LbmError, match="lbm_set_forces: not available on a member of a batch"):
            batch.member(0).set_forces(10, 4)
    # a rank context (one rank, host message passing that is never called)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_set_forces: not available in a multi-process"):
            eng.set_forces(10, 4)


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_forces: the context runs the %s halo mode" % mode):
                eng.set_forces(10, 4)
        eng.set_halo_mode("sync")
        eng.set_forces(10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match=r"lbm_set_halo_mode: obstacle forces are armed \(lbm_set_forces\)"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0


# ---- the command line ---------------------------------------------------------------------------------------------------
def test_cli_writes_forces_dat(lbm, datasets, tmp_path):
    """d2q9-bgk with LBM_FORCES=50 on 128^2 for 1 000 steps: forces.dat parses to the rows Engine.forces gives (and is
    write_forces of them, byte for byte); final_state.dat as without the variable, which writes no forces.dat."""
    p, ob = datasets("128x128")
    p.max_iters = 1000
    of = os.path.join(GOLDEN, "inputs", "obstacles_128x128.dat")
    outs = {}
    for label, extra in (("plain", {}), ("forces", {"LBM_FORCES": "50"})):
        d = tmp_path / label
        d.mkdir()
        pf = d / "input.params"
        pf.write_text("%d\n%d\n%d\n%d\n%.9g\n%.9g\n%.9g\n" % (p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel, p.omega))
        out = subprocess.run([lbm.CLI_PATH, str(pf), of], cwd=d, capture_output=True, text=True, env=dict(os.environ, **extra), timeout=120)
        assert out.returncode == 0, out.stderr
        outs[label] = d
    md5 = [hashlib.md5((outs[k] / "final_state.dat").read_bytes()).hexdigest() for k in ("plain", "forces")]
    assert md5[0] == md5[1]
    assert not (outs["plain"] / "forces.dat").exists()
    with lbm.Engine(p, ob) as eng:
        eng.set_forces(50, 32)
        eng.run(1000)
        steps, rows = eng.forces()
    assert steps.tolist() == list(range(0, 1000, 50))
    lines = (outs["forces"] / "forces.dat").read_text().splitlines()
    assert [int(line.split(":")[0]) for line in lines] == steps.tolist()
    parsed = np.array([[float(v) for v in line.split(":")[1].split()] for line in lines])
    assert np.allclose(parsed, rows[:, 0, :], rtol=1e-12, atol=0.0) and np.all(rows[-1, 0, :] != 0.0)
    twin = tmp_path / "twin.dat"
    lbm.write_forces(str(twin), steps, rows)
    assert (outs["forces"] / "forces.dat").read_bytes() == twin.read_bytes()


def test_cli_forces_across_segments(lbm, tmp_path):
    """The segment loop of the command line over more than one segment: 64 x 16 with three blocked cells, 4 100 steps and
    LBM_FORCES=1, so the ring of 4 096 rows is drained after 4 096 steps and a second segment of 4 steps follows.  forces.dat
    holds the steps 0 .. 4 099 in order and is, as final_state.dat and av_vels.dat are, byte for byte what an Engine driven
    the same way gives: set_forces(1, 4096), run(4096), drain, run(4), drain."""
    p = lbm.Params(64, 16, 4100, 16, 0.1, 1e-5, 1.0)
    ob = np.zeros((16, 64), dtype=np.int32)
    ob[5, 20] = ob[6, 20] = ob[9, 41] = 1
    d = tmp_path / "cli"
    out = run_cli(lbm, d, params_text(p), obstacles_text(ob), LBM_FORCES="1")
    assert out.returncode == 0, out.stderr
    with lbm.Engine(p, ob) as eng:
        eng.set_forces(1, 4096)
        drained = []
        for n in (4096, 4):
            eng.run(n)
            drained.append(eng.forces())
        fields, av = eng.final_state(), eng.av_vels(4100)
    assert [len(steps) for steps, _ in drained] == [4096, 4]
    steps, rows = np.concatenate([s for s, _ in drained]), np.concatenate([r for _, r in drained])
    lines = (d / "forces.dat").read_text().splitlines()
    assert len(lines) == 4100
    assert [int(line.split(":")[0]) for line in lines] == list(range(4100)) == steps.tolist()
    assert rows[-1, 0, 0] != 0.0
    lbm.write_forces(str(tmp_path / "forces.dat"), steps, rows)
    lbm.write_final_state(str(tmp_path / "final_state.dat"), fields, ob)
    lbm.write_av_vels(str(tmp_path / "av_vels.dat"), av)
    for name in ("forces.dat", "final_state.dat", "av_vels.dat"):
        assert (d / name).read_bytes() == (tmp_path / name).read_bytes(), name
