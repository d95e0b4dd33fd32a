"""Point probes (lbm_set_probes / Engine.set_probes): u_x, u_y, |u| and pressure at chosen cells after every global
timestep tt with tt % every == 0, recorded by the running kernels.  A sample is by definition final_state at one cell,
so every comparison here is bitwise (uint32 views) against the oracle stepped to tt + 1; recording never changes the
lattice, and av_vels stays bit-identical to the unarmed run (resident path) or to the run split at the sample steps
(per-pass paths)."""
import numpy as np
import pytest

import test_frames_format as model
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu

FIELDS = ("u_x", "u_y", "u", "pressure")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_series(oracle, p, ob, cells, start, total, every, probes, only=None):
    """(lattice after `total` steps, {tt: float32[n_probes, 4]}) for the sample steps tt in [start, total) (those in
    `only`, if given); `cells` is the lattice after `start` steps."""
    ref = cells.copy()
    xs = np.array([c[0] for c in probes])
    ys = np.array([c[1] for c in probes])
    want, done = {}, start
    for tt in model.frame_steps(start, total, every):
        if only is not None and tt not in only:
            continue
        oracle.run(p, ref, ob, tt + 1 - done)
        done = tt + 1
        fs = oracle.final_state(p, ref, ob)
        want[tt] = np.stack([np.asarray(fs[k], dtype=np.float32)[ys, xs] for k in FIELDS], axis=1)
    oracle.run(p, ref, ob, total - done)
    return ref, want


def run_engine(lbm, p, ob, cells, calls, probes=None, every=0, capacity=0, n_gpus=1):
    """Run `calls` from step 0, probes armed before the first call; drain after each call."""
    steps, samples = [], []
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        if every:
            eng.set_probes(probes, every, capacity or 1 + sum(calls) // every)
        for n in calls:
            eng.run(n)
            if every:
                s, v = eng.probes()
                steps.append(s)
                samples.append(v)
        info = eng.info()
        return (eng.cells(), eng.av_vels(sum(calls)), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(samples) if samples else None, info)


def assert_series(steps, samples, want, only=None):
    got = steps.tolist()
    if only is None:
        assert got == sorted(want), (got, sorted(want))
    for i, tt in enumerate(got):
        if tt in want:
            assert np.array_equal(bits(samples[i]), bits(want[tt])), \
                f"sample tt={tt} differs at probes {np.nonzero((bits(samples[i]) != bits(want[tt])).any(axis=1))[0].tolist()}"


def probe_set(nx, ny, ob):
    """A cell on the lid row, the rows on both sides of band seams (two- and four-row bands), the wave-edge columns, a
    blocked cell, a duplicate, several probes in one band and none in most."""
    cols = sorted({0, 63 % nx, 64 % nx, nx - 1})
    cells = [(nx // 3, ny - 2), (cols[-1], ny - 2)]                      # lid row
    cells += [(x, y) for x in cols for y in (3, 4)]                      # seam of four-row bands (and of two-row ones)
    cells += [(cols[1], 5), (cols[2], 6)]                                # seam of two-row bands / interior rows
    cells += [(5 % nx, 0), (7 % nx, ny - 1)]                             # the periodic seam
    by, bx = np.nonzero(ob)
    if by.size:
        cells.append((int(bx[by.size // 2]), int(by[by.size // 2])))     # a blocked cell
        cells.append((int(bx[0]), int(by[0])))
    cells.append(cells[2])                                                # a duplicate
    return cells


def check_resident(lbm, oracle, p, ob, cells, calls, everys, probes, only=None):
    total = sum(calls)
    ref, all_want = oracle_series(oracle, p, ob, cells, 0, total, 1 if only is None else min(everys), probes,
                                  only=only)
    base, base_av, _, _, info = run_engine(lbm, p, ob, cells, calls)
    assert info["resident_steps"] > 0
    assert np.array_equal(bits(ref), bits(base))
    for every in everys:
        want = {tt: v for tt, v in all_want.items() if tt % every == 0}
        got, av, steps, samples, info = run_engine(lbm, p, ob, cells, calls, probes, every)
        assert info["resident_steps"] > 0
        assert steps.tolist() == list(model.frame_steps(0, total, every))
        assert_series(steps, samples, want, only=only)
        assert np.array_equal(bits(base), bits(got)), f"probes changed the lattice (every {every})"
        assert np.array_equal(bits(base_av), bits(av)), f"probes changed av_vels on the resident path (every {every})"


@pytest.mark.parametrize("calls", [[301], [50, 251]])
@pytest.mark.parametrize("name", ["128x128", "128x256", "256x256", "1024x1024"])
def test_resident_reference_datasets(lbm, oracle, datasets, monkeypatch, name, calls):
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "16")
    p, ob = datasets(name)
    check_resident(lbm, oracle, p, ob, oracle.init_cells(p), calls, (1, 7, 100), probe_set(p.nx, p.ny, ob))


@pytest.mark.parametrize("nx,ny,env", [(128, 16, {}), (128, 64, {"LBM_RESIDENT_ROWS": "4"}),
                                       (256, 64, {"LBM_RESIDENT_JOINT": "0"}), (320, 24, {"LBM_RESIDENT_JOINT": "1"}),
                                       (1024, 128, {"LBM_RESIDENT_XCD": "0"}), (1024, 64, {}),
                                       (512, 64, {"LBM_RESIDENT_ROWS": "2"}),
                                       (128, 128, {"LBM_RESIDENT_ONE_XCD": "0", "LBM_RESIDENT_GROUP": "4"}),
                                       (128, 64, {"LBM_RESIDENT_GROUP": "2", "LBM_RESIDENT_XCD": "0"})])
def test_resident_random_lattices(lbm, oracle, monkeypatch, nx, ny, env):
    """The shapes and variants of test_gpu_frames.py::test_resident_random_lattices, and the forms it says they launch:
    obstacles on the lid row and on the seam rows of the bands; two-row bands (<512, false, 2> and <1024, false, 2>) but for
    128 x 64 with LBM_RESIDENT_ROWS=4, the one four-row JOINT case; one XCD and grouped workgroups.  The other four-row
    forms: tests/test_gpu_resident_forms.py."""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
    ob[ny - 2, ::5] = 1                     # lid row
    ob[3::4, ::7] = 1                       # seam rows of four-row bands
    ob[0::4, 3::7] = 1
    probes = probe_set(nx, ny, ob) + [(0, ny - 2), (1, ny - 2)]   # a blocked and a free lid cell
    check_resident(lbm, oracle, p, ob, cells, [1, 2, 19, 5], (1, 3), probes)


def test_resident_chunk_boundary(lbm, oracle):
    """A 4100-step call runs two launches (4096 + 4): a sample on the last step of the first (accel_last) and on the
    first step of the second.  every = 1 is compared with the oracle on steps 4090 ... 4099 only."""
    p, ob, cells = random_case(lbm, 128, 128, 5, walls=False)
    p.max_iters = 4100
    probes = probe_set(128, 128, ob)
    check_resident(lbm, oracle, p, ob, cells, [4100], (4095,), probes, only={0, 4095})
    check_resident(lbm, oracle, p, ob, cells, [4100], (4096,), probes, only={0, 4096})
    check_resident(lbm, oracle, p, ob, cells, [4100], (1,), probes, only=set(range(4090, 4100)))


def test_arming_mid_run_uses_global_steps(lbm, oracle):
    p, ob, cells = random_case(lbm, 128, 128, 9, walls=False)
    p.max_iters = 431
    probes = probe_set(128, 128, ob)
    ref = cells.copy()
    oracle.run(p, ref, ob, 130)
    _, want = oracle_series(oracle, p, ob, ref, 130, 431, 100, probes)
    with lbm.Engine(p, ob, cells) as eng:
        eng.run(130)
        eng.set_probes(probes, 100, 3)
        eng.run(301)
        steps, samples = eng.probes()
    assert steps.tolist() == [200, 300, 400]
    assert_series(steps, samples, want)


def test_max_probes_at_once(lbm, oracle, datasets, monkeypatch):
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "16")
    p, ob = datasets("128x128")
    rng = np.random.default_rng(7)
    probes = [(int(x), int(y)) for x, y in zip(rng.integers(0, 128, lbm.LBM_MAX_PROBES), rng.integers(0, 128, lbm.LBM_MAX_PROBES))]
    probes[:4] = [(0, 126), (127, 126), (63, 126), (64, 126)]
    assert len(probes) == 256
    check_resident(lbm, oracle, p, ob, oracle.init_cells(p), [120], (1, 7), probes)


PER_PASS = {"LBM_RESIDENT": "0", "LBM_TILE_STEPS": "0", "LBM_GRAPH": "0"}


@pytest.mark.parametrize("every", [25, 1])
@pytest.mark.parametrize("env,n_gpus,launch", [
    (dict(PER_PASS, LBM_FUSE2="1"), 1, (2, 3)),                                   # stream kernel, K = 2 / 3
    (dict(PER_PASS, LBM_FUSE2="1", LBM_PASS_STEPS="4", LBM_LANE_CELLS="4"), 1, (4,)),  # K = 4, packed
    (dict(PER_PASS, LBM_FUSE2="0"), 1, (1,)),                                     # one-step kernel
    (dict(PER_PASS, LBM_TILE_STEPS="4"), 1, (4,)),                                # LDS-tile kernel
    (dict(PER_PASS, LBM_GRAPH="1"), 1, None),                                     # hipGraph chunks
    ({"LBM_HALO": "memcpy"}, 2, None), ({"LBM_HALO": "memcpy"}, 3, None)])
def test_per_pass_families(lbm, oracle, monkeypatch, env, n_gpus, launch, every):
    """Calls the resident kernel does not serve end their passes at every sample step, each followed by probe_gather:
    the series matches the oracle, lattice and av_vels match the same run issued as calls split at the sample steps."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    graph = env.get("LBM_GRAPH") == "1"
    if graph and every == 25:
        every = 150                                   # segments of 94 and 109 steps: hipGraph chunks are replayed
    p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
    probes = probe_set(128, 96, ob)
    for first, count in (lbm.partition_rows(96, n_gpus, s) for s in range(n_gpus)):
        probes += [(11, first), (64, first + count - 1), (127, first + count // 2)]   # every slab, both sides of its seams
    calls = [57, 203]
    ref, want = oracle_series(oracle, p, ob, cells, 0, sum(calls), every, probes)
    got, av, steps, samples, info = run_engine(lbm, p, ob, cells, calls, probes, every, n_gpus=n_gpus)
    assert info["resident_steps"] == 0
    assert info["n_slabs"] == n_gpus
    if launch:
        assert info["steps_per_launch"] in launch, info
    if graph and every == 150:
        assert info["graph_steps"] > 0 and info["graph_steps"] < 94, info
    assert_series(steps, samples, want)
    assert np.array_equal(bits(ref), bits(got))
    split = model.split_calls(calls, every)
    base, base_av, _, _, _ = run_engine(lbm, p, ob, cells, split, n_gpus=n_gpus)
    assert np.array_equal(bits(base), bits(got))
    assert np.array_equal(bits(base_av), bits(av))


def test_batch_members_armed_independently(lbm, oracle):
    """Eight members, two armed with their own cells and interval; long (batched resident) and short (per-pass, member
    by member) calls mixed."""
    p0, ob0, c0 = random_case(lbm, 128, 128, 41, walls=False)
    params = [lbm.Params(128, 128, 400, 10, 0.1, float(np.float32(0.004 + 0.001 * i)), float(np.float32(1.6 + 0.03 * i)))
              for i in range(8)]
    obstacles = [np.roll(ob0, i, axis=1) for i in range(8)]
    cells = [np.roll(c0, i, axis=0) for i in range(8)]
    armed = {2: (probe_set(128, 128, obstacles[2]), 1), 5: ([(64, 126), (3, 3), (3, 4), (100, 77)], 7)}
    calls = [2, 300, 3, 95]
    with lbm.Batch(params, obstacles, cells) as plain, lbm.Batch(params, obstacles, cells) as batch:
        assert batch.info()["resident_steps"] > 0 and batch.info()["resident_min_steps"] > 3
        for i, (pc, e) in armed.items():
            batch.member(i).set_probes(pc, e, 1 + sum(calls) // e)
        for n in calls:
            plain.run(n)
            batch.run(n)
        for i in range(8):
            m, q = batch.member(i), plain.member(i)
            ref = cells[i].copy()
            oracle.run(params[i], ref, obstacles[i], sum(calls))
            assert np.array_equal(bits(m.cells()), bits(ref)), i
            assert np.array_equal(bits(m.cells()), bits(q.cells())), i
            if i in armed:
                pc, e = armed[i]
                steps, samples = m.probes()
                _, want = oracle_series(oracle, params[i], obstacles[i], cells[i], 0, sum(calls), e, pc)
                assert_series(steps, samples, want)
                s_steps, s_samples = run_engine(lbm, params[i], obstacles[i], cells[i], calls, pc, e)[2:4]
                assert s_steps.tolist() == steps.tolist()
                assert np.array_equal(bits(s_samples), bits(samples))
            else:
                assert np.array_equal(bits(m.av_vels()), bits(q.av_vels())), i
                assert m.probes()[0].size == 0


def test_ring_overflow_fails_before_any_work(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_probes([(1, 2), (3, 4)], 10, 2)
        with pytest.raises(lbm.LbmError, match="holds 2"):
            eng.run(25)                      # samples at 0, 10, 20
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match="2 samples are waiting"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        steps, samples = eng.probes(1)
        assert steps.tolist() == [0] and samples.shape == (1, 2, 4)
        eng.run(10)                          # 20
        assert eng.probes()[0].tolist() == [10, 20]
        eng.set_probes([], 0)
        eng.run(30)
        assert eng.probes()[0].size == 0
        eng.set_probes([(1, 2)], 0)          # every == 0 disarms as well
        eng.run(5)
        assert eng.probes()[0].size == 0
    with lbm.Batch([p, p], [ob, ob], [cells, cells]) as batch:
        batch.member(1).set_probes([(1, 2)], 10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run.*holds 2"):
            batch.run(25)
        assert batch.info()["steps_done"] == 0
        assert batch.member(0).info()["steps_done"] == 0


def test_refusals(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 4, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        for bad in ((128, 0), (0, 128), (-1, 5), (5, -1)):
            with pytest.raises(lbm.LbmError, match="outside the 128 x 128 grid"):
                eng.set_probes([(1, 1), bad], 1, 4)
        with pytest.raises(lbm.LbmError, match="capacity 0"):
            eng.set_probes([(1, 1)], 1, 0)
        arr = (lbm._CProbe * 300)()
        for n, every, cap, msg in ((257, 1, 4, "LBM_MAX_PROBES"), (-1, 1, 4, "LBM_MAX_PROBES"), (1, -1, 4, "negative interval"),
                                   (1, 1, 0, "capacity 0")):
            assert eng.lib.lbm_set_probes(eng.handle, n, arr, every, cap) != 0
            assert msg in eng.lib.lbm_last_error().decode()
        assert eng.info()["steps_done"] == 0
        # one recorder per context, both directions
        eng.set_frames(10, 2)
        with pytest.raises(lbm.LbmError, match="frames are armed"):
            eng.set_probes([(1, 1)], 1, 4)
        eng.set_frames(0)
        eng.set_probes([(1, 1)], 1, 4)
        with pytest.raises(lbm.LbmError, match="probes are armed"):
            eng.set_frames(10, 2)
        with pytest.raises(lbm.LbmError, match="probes are armed"):
            eng.run_until(100, 10)
        assert eng.info()["steps_done"] == 0
    with lbm.Batch([p, p], [ob, ob], [cells, cells]) as batch:
        batch.member(0).set_probes([(1, 1)], 1, 4)
        with pytest.raises(lbm.LbmError, match="probes are armed"):
            batch.run_until(100, 10)
        with pytest.raises(lbm.LbmError, match="one kind"):
            batch.member(1).set_frames(10, 2)
        assert batch.info()["steps_done"] == 0
    # a rank context (one rank, host message passing that is never called)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="multi-process"):
            eng.set_probes([(1, 1)], 1, 4)


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="halo mode"):
                eng.set_probes([(1, 1)], 10, 4)
        eng.set_halo_mode("sync")
        eng.set_probes([(1, 1)], 10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match="probes are armed"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0


def test_cli_writes_probes_dat(lbm, oracle, datasets, tmp_path):
    """d2q9-bgk with LBM_PROBES="64,64;10,126:1" on 128^2 for 250 steps: probes.dat byte-identical to write_probes fed
    with the oracle's series; final_state.dat and av_vels.dat as without it; no probes.dat without the variable."""
    import hashlib
    import os
    import subprocess
    from conftest import GOLDEN
    p, ob = datasets("128x128")
    p.max_iters = 250
    of = os.path.join(GOLDEN, "inputs", "obstacles_128x128.dat")
    outs = {}
    for label, extra in (("plain", {}), ("probes", {"LBM_PROBES": "64,64;10,126:1"})):
        d = tmp_path / label
        d.mkdir()
        pf = d / "input.params"
        pf.write_text("%d\n%d\n%d\n%d\n%.9g\n%.9g\n%.9g\n" % (p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel,
                                                           p.omega))
        out = subprocess.run([lbm.CLI_PATH, str(pf), of], cwd=d, capture_output=True, text=True,
                             env=dict(os.environ, **extra), timeout=120)
        assert out.returncode == 0, out.stderr
        outs[label] = d
    for name in ("final_state.dat", "av_vels.dat"):
        md5 = [hashlib.md5((outs[k] / name).read_bytes()).hexdigest() for k in ("plain", "probes")]
        assert md5[0] == md5[1], name
    assert not (outs["plain"] / "probes.dat").exists()
    cells = [(64, 64), (10, 126)]
    _, want = oracle_series(oracle, p, ob, oracle.init_cells(p), 0, 250, 1, cells)
    twin = tmp_path / "twin.dat"
    lbm.write_probes(str(twin), cells, np.arange(250), np.stack([want[tt] for tt in range(250)]))
    assert (outs["probes"] / "probes.dat").read_bytes() == twin.read_bytes()


def test_switching_recorder_kind(lbm, oracle, monkeypatch):
    """One recorder per context, re-armed as the other kind mid-run: frames for 40 steps, then probes (one on the lid row)
    for 40 more, on an engine and across the members of a batch, whose count of armed members must go back to zero."""
    from test_gpu_frames import assert_frames, oracle_frames
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "16")
    nx, ny = 128, 16
    probes = [(5, 3), (77, ny - 2)]
    cases = [random_case(lbm, nx, ny, seed, walls=False) for seed in (61, 62)]
    refs = []   # per case: (frames of steps [0, 40), lattice after 80 steps, series of steps [40, 80))
    for p, ob, cells in cases:
        ref40, want_frames = oracle_frames(oracle, p, ob, cells, 0, 40, 7)
        ref80, want_series = oracle_series(oracle, p, ob, ref40, 40, 80, 3, probes)
        refs.append((want_frames, ref80, want_series))

    # (a) engine
    p, ob, cells = cases[0]
    want_frames, ref80, want_series = refs[0]
    with lbm.Engine(p, ob, cells) as eng:
        assert eng.info()["resident_steps"] > 0
        eng.set_frames(7, 16)
        eng.run(40)
        assert_frames(*eng.frames(), want_frames)
        eng.set_frames(0)
        eng.set_probes(probes, 3, 32)
        eng.run(40)
        steps, samples = eng.probes()
        assert steps.tolist() == list(range(42, 79, 3))
        assert_series(steps, samples, want_series)
        assert eng.frames()[0].size == 0
        assert np.array_equal(bits(eng.cells()), bits(ref80))

    # (b) batch of two members: frames on member 0, then probes on member 1
    with lbm.Batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]) as batch:
        assert batch.info()["resident_steps"] > 0
        m0, m1 = batch.member(0), batch.member(1)
        m0.set_frames(7, 16)
        batch.run(40)
        assert_frames(*m0.frames(), refs[0][0])
        m0.set_frames(0)
        m1.set_probes(probes, 3, 32)        # not "one kind": no member has frames armed any more
        batch.run(40)
        steps, samples = m1.probes()
        assert steps.tolist() == list(range(42, 79, 3))
        assert_series(steps, samples, refs[1][2])
        assert m0.frames()[0].size == 0
        for m, (_, ref80, _) in zip((m0, m1), refs):
            assert np.array_equal(bits(m.cells()), bits(ref80))
