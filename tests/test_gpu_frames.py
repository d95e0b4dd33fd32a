"""Animation frames (lbm_set_frames / Engine.set_frames): |u| after every global timestep tt with tt % every == 0,
recorded by the running kernels (the reference's write_animation_data hook, SerialCode/d2q9-bgk.c:171-173).  Every
frame is bit-identical to the oracle's final_state u at that step; recording never changes the lattice, and av_vels
stays bit-identical on the resident path and equal to the run split at the frame steps on the per-pass paths."""
import numpy as np
import pytest

import test_frames_format as model
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu


def oracle_frames(oracle, p, ob, cells, start, total, every):
    """(lattice after `total` steps, {tt: u}) for the frame steps tt in [start, total); `cells` is the lattice
    after `start` steps."""
    ref = cells.copy()
    frames, done = {}, start
    for tt in model.frame_steps(start, total, every):
        oracle.run(p, ref, ob, tt + 1 - done)
        done = tt + 1
        frames[tt] = oracle.final_state(p, ref, ob)["u"].copy()
    oracle.run(p, ref, ob, total - done)
    return ref, frames


def run_engine(lbm, p, ob, cells, calls, every=0, capacity=0, n_gpus=1):
    """Run `calls` from step 0, frames armed before the first call; drain after each call."""
    steps, frames = [], []
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        if every:
            eng.set_frames(every, capacity or 1 + sum(calls) // every)
        for n in calls:
            eng.run(n)
            s, f = eng.frames()
            steps.append(s)
            frames.append(f)
        info = eng.info()
        return (eng.cells(), eng.av_vels(sum(calls)), np.concatenate(steps) if steps else np.zeros(0, np.int32),
                np.concatenate(frames) if frames else None, info)


def assert_frames(steps, frames, want):
    assert steps.tolist() == sorted(want), (steps.tolist(), sorted(want))
    for i, tt in enumerate(steps.tolist()):
        assert np.array_equal(frames[i].view(np.uint32), want[tt].view(np.uint32)), f"frame tt={tt} differs"


def check_resident(lbm, oracle, p, ob, cells, calls, every):
    ref, want = oracle_frames(oracle, p, ob, cells, 0, sum(calls), every)
    got, av, steps, frames, info = run_engine(lbm, p, ob, cells, calls, every)
    assert info["resident_steps"] > 0
    assert_frames(steps, frames, want)
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    base, base_av, _, _, _ = run_engine(lbm, p, ob, cells, calls)
    assert np.array_equal(base.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(base_av.view(np.uint32), av.view(np.uint32)), "frames changed av_vels on the resident path"


@pytest.mark.parametrize("name,calls,everys", [("128x128", [301], (100, 7, 1)), ("128x128", [50, 251], (100, 7, 1)),
                                               ("128x256", [50, 251], (100, 7)), ("256x256", [301], (100, 7, 1)),
                                               ("1024x1024", [50, 251], (100, 7))])
def test_resident_reference_datasets(lbm, oracle, datasets, monkeypatch, name, calls, everys):
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "16")
    p, ob = datasets(name)
    cells = oracle.init_cells(p)
    for every in everys:
        check_resident(lbm, oracle, p, ob, cells, calls, every)


@pytest.mark.parametrize("nx,ny,env", [(128, 16, {}), (128, 64, {"LBM_RESIDENT_ROWS": "4"}),
                                       (256, 64, {"LBM_RESIDENT_JOINT": "0"}), (320, 24, {"LBM_RESIDENT_JOINT": "1"}),
                                       (1024, 128, {"LBM_RESIDENT_XCD": "0"}), (1024, 64, {}),
                                       (512, 64, {"LBM_RESIDENT_ROWS": "2"}),
                                       (128, 128, {"LBM_RESIDENT_ONE_XCD": "0", "LBM_RESIDENT_GROUP": "4"}),
                                       (128, 64, {"LBM_RESIDENT_GROUP": "2", "LBM_RESIDENT_XCD": "0"})])
def test_resident_random_lattices(lbm, oracle, monkeypatch, nx, ny, env):
    """Obstacles on the lid row and on the seam rows of the bands.  What the list launches at 256 CUs (pinned by
    tests/test_resident_forms.py, table in tests/resident_forms.py): two-row bands everywhere but 128 x 64 with
    LBM_RESIDENT_ROWS=4, which is the one four-row and the one JOINT case -- LBM_RESIDENT_JOINT has no say under two-row
    bands, so 256 x 64 and 320 x 24 run <512, false, 2> like 128 x 16; both 1024-wide cases run <1024, false, 2>; one
    XCD, grouped workgroups and seams written through are two-row cases.  The four-row forms without JOINT and at 1024
    threads are launched by tests/test_gpu_resident_forms.py."""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
    ob[ny - 2, ::5] = 1                     # lid row
    ob[3::4, ::7] = 1                       # seam rows of four-row bands
    ob[0::4, 3::7] = 1
    check_resident(lbm, oracle, p, ob, cells, [1, 2, 19, 5], 3)


@pytest.mark.parametrize("every", [4095, 4096])
def test_resident_chunk_boundary(lbm, oracle, every):
    """A 4100-step call runs two launches (4096 + 4): a frame on the last step of the first (accel_last) and on the
    first step of the second."""
    p, ob, cells = random_case(lbm, 128, 128, 5, walls=False)
    p.max_iters = 4100
    check_resident(lbm, oracle, p, ob, cells, [4100], every)


def test_arming_mid_run_uses_global_steps(lbm, oracle):
    p, ob, cells = random_case(lbm, 128, 128, 9, walls=False)
    p.max_iters = 431
    ref = cells.copy()
    oracle.run(p, ref, ob, 130)
    _, want = oracle_frames(oracle, p, ob, ref, 130, 431, 100)
    with lbm.Engine(p, ob, cells) as eng:
        eng.run(130)
        eng.set_frames(100, 3)
        eng.run(301)
        steps, frames = eng.frames()
    assert steps.tolist() == [200, 300, 400]
    assert_frames(steps, frames, want)


PER_PASS = {"LBM_RESIDENT": "0", "LBM_TILE_STEPS": "0", "LBM_GRAPH": "0"}


@pytest.mark.parametrize("env,n_gpus,every,launch", [
    (dict(PER_PASS, LBM_FUSE2="1"), 1, 25, (2, 3)),                                   # stream kernel, K = 2 / 3
    (dict(PER_PASS, LBM_FUSE2="1", LBM_PASS_STEPS="4", LBM_LANE_CELLS="4"), 1, 25, (4,)),  # K = 4, packed
    (dict(PER_PASS, LBM_FUSE2="0"), 1, 25, (1,)),                                     # one-step kernel
    (dict(PER_PASS, LBM_TILE_STEPS="4"), 1, 25, (4,)),                                # LDS-tile kernel
    (dict(PER_PASS, LBM_GRAPH="1"), 1, 150, None),     # segments of 94 and 109 steps: hipGraph chunks are replayed
    ({"LBM_HALO": "memcpy"}, 2, 25, None), ({"LBM_HALO": "memcpy"}, 3, 25, None)])
def test_per_pass_families(lbm, oracle, monkeypatch, env, n_gpus, every, launch):
    """Calls the resident kernel does not serve end their passes at every frame step: frames match the oracle, the
    lattice and av_vels match the same run issued as calls split at the frame steps."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
    calls = [57, 203]
    ref, want = oracle_frames(oracle, p, ob, cells, 0, sum(calls), every)
    got, av, steps, frames, info = run_engine(lbm, p, ob, cells, calls, every, n_gpus=n_gpus)
    assert info["resident_steps"] == 0
    if launch:
        assert info["steps_per_launch"] in launch, info
    if env.get("LBM_GRAPH") == "1":
        assert info["graph_steps"] > 0 and info["graph_steps"] < 94, info
    assert_frames(steps, frames, want)
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    split = model.split_calls(calls, every)
    base, base_av, _, _, _ = run_engine(lbm, p, ob, cells, split, n_gpus=n_gpus)
    assert np.array_equal(base.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(base_av.view(np.uint32), av.view(np.uint32))


def test_batch_members_armed_independently(lbm, oracle):
    p0, ob0, c0 = random_case(lbm, 128, 128, 31, walls=False)
    params, obstacles, cells = [], [], []
    for i in range(8):
        params.append(lbm.Params(128, 128, 400, 10, 0.1, float(np.float32(0.004 + 0.001 * i)), float(np.float32(1.6 + 0.03 * i))))
        obstacles.append(np.roll(ob0, i, axis=1))
        cells.append(np.roll(c0, i, axis=0))
    armed = {0: 50, 3: 7}
    calls = [120, 180]
    with lbm.Batch(params, obstacles, cells) as plain, lbm.Batch(params, obstacles, cells) as batch:
        assert batch.info()["resident_steps"] > 0
        for i, e in armed.items():
            batch.member(i).set_frames(e, 1 + sum(calls) // e)
        for n in calls:
            plain.run(n)
            batch.run(n)
        for i in range(8):
            m, q = batch.member(i), plain.member(i)
            assert np.array_equal(m.cells().view(np.uint32), q.cells().view(np.uint32)), i
            assert np.array_equal(m.av_vels().view(np.uint32), q.av_vels().view(np.uint32)), i
            if i in armed:
                steps, frames = m.frames()
                _, want = oracle_frames(oracle, params[i], obstacles[i], cells[i], 0, sum(calls), armed[i])
                assert_frames(steps, frames, want)
                s_steps, s_frames = run_engine(lbm, params[i], obstacles[i], cells[i], calls, armed[i])[2:4]
                assert np.array_equal(s_frames.view(np.uint32), frames.view(np.uint32))
            else:
                assert m.frames()[0].size == 0


def test_capacity_overflow_fails_before_any_work(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_frames(10, 2)
        with pytest.raises(lbm.LbmError, match="holds 2"):
            eng.run(25)                      # frames at 0, 10, 20
        assert eng.info()["steps_done"] == 0
        eng.run(15)                          # 0, 10
        with pytest.raises(lbm.LbmError, match="2 frames are waiting"):
            eng.run(10)
        assert eng.info()["steps_done"] == 15
        steps, _ = eng.frames(1)
        assert steps.tolist() == [0]
        eng.run(10)                          # 20
        assert eng.frames()[0].tolist() == [10, 20]
        eng.set_frames(0)
        eng.run(30)
        assert eng.frames()[0].size == 0


def refuse_frames(lbm, eng):
    """One hipMalloc of about 128 TiB (2^31 - 1 slots of 128 x 128 floats): the runtime refuses it at once with an
    out-of-memory return code, and nothing faults."""
    with pytest.raises(lbm.LbmError, match="frames stay off"):
        eng.set_frames(1, 2**31 - 1)


def test_failed_allocation_leaves_the_engine_whole(lbm, oracle, datasets):
    """lbm_set_frames whose buffer cannot be allocated returns an error and leaves nothing behind: the same engine runs
    on, bit-identical to the oracle, and arms again.  Arming right after the refusal records the frames of steps 0, 10,
    20 and 30 of a 40-step run; arming after 40 steps those of the next 40."""
    p, ob = datasets("128x128")
    cells = oracle.init_cells(p)
    ref, want = oracle_frames(oracle, p, ob, cells, 0, 40, 10)
    ref_av = oracle.run(p, cells.copy(), ob, 40)
    ref80, want80 = oracle_frames(oracle, p, ob, ref, 40, 80, 10)
    with lbm.Engine(p, ob, cells) as plain:
        plain.run(40)
        plain_av = plain.av_vels(40)
    with lbm.Engine(p, ob, cells) as eng:
        refuse_frames(lbm, eng)
        eng.run(40)
        assert np.array_equal(eng.cells().view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(eng.av_vels(40).view(np.uint32), plain_av.view(np.uint32)), "the refusal changed av_vels"
        np.testing.assert_allclose(eng.av_vels(40), ref_av, rtol=2e-4, atol=0)    # test_gpu_parity.AV_RTOL
        assert eng.frames()[0].size == 0
        eng.set_frames(10, 4)
        eng.run(40)
        steps, frames = eng.frames()
        assert steps.tolist() == [40, 50, 60, 70]
        assert_frames(steps, frames, want80)
        assert np.array_equal(eng.cells().view(np.uint32), ref80.view(np.uint32))
    with lbm.Engine(p, ob, cells) as eng:
        refuse_frames(lbm, eng)
        eng.set_frames(10, 4)
        eng.run(40)
        steps, frames = eng.frames()
        assert steps.tolist() == [0, 10, 20, 30]
        assert_frames(steps, frames, want)
        assert np.array_equal(eng.cells().view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(eng.av_vels(40).view(np.uint32), plain_av.view(np.uint32))


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="halo mode"):
                eng.set_frames(10, 4)
        eng.set_halo_mode("sync")
        eng.set_frames(10, 4)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match="frames are armed"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0


def test_cli_writes_the_reference_animation_files(lbm, oracle, datasets, tmp_path):
    """d2q9-bgk with LBM_ANIMATION=100 on 128^2 for 250 steps: animation_data/velocity_magnitude_%06d.dat for tt = 0, 100,
    200, byte-identical to the Python twin of the oracle's frames; final_state.dat and av_vels.dat as without it."""
    import hashlib
    import os
    import shutil
    import subprocess
    from conftest import GOLDEN
    p, ob = datasets("128x128")
    p.max_iters = 250
    of = os.path.join(GOLDEN, "inputs", "obstacles_128x128.dat")
    outs = {}
    for label, extra in (("plain", {}), ("anim", {"LBM_ANIMATION": "100"})):
        d = tmp_path / label
        d.mkdir()
        pf = d / "input.params"
        pf.write_text("%d\n%d\n%d\n%d\n%.9g\n%.9g\n%.9g\n" % (p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel,
                                                           p.omega))
        out = subprocess.run([lbm.CLI_PATH, str(pf), of], cwd=d, capture_output=True, text=True,
                             env=dict(os.environ, **extra), timeout=120)
        assert out.returncode == 0, out.stderr
        outs[label] = (d, out.stdout)
    d, stdout = outs["anim"]
    for name in ("final_state.dat", "av_vels.dat"):
        md5 = [hashlib.md5((outs[k][0] / name).read_bytes()).hexdigest() for k in ("plain", "anim")]
        assert md5[0] == md5[1], name
    assert [l for l in stdout.splitlines() if l.startswith("Written animation")] == \
        ["Written animation data for timestep %d" % tt for tt in (0, 100, 200)]
    assert not (outs["plain"][0] / "animation_data").exists()
    _, want = oracle_frames(oracle, p, ob, oracle.init_cells(p), 0, 250, 100)
    assert sorted(os.listdir(d / "animation_data")) == ["velocity_magnitude_%06d.dat" % tt for tt in (0, 100, 200)]
    for tt, u in want.items():
        twin = tmp_path / ("twin_%d.dat" % tt)
        lbm.write_animation_frame(str(twin), u, tt)
        assert (d / "animation_data" / ("velocity_magnitude_%06d.dat" % tt)).read_bytes() == twin.read_bytes(), tt


def test_batch_short_call_then_resident(lbm, oracle):
    """A call below resident_min_steps runs the members one by one on the per-pass kernels; an armed member's call is
    split at its frame steps (here: 1 + 1 passes against one 2-step pass of the others).  The next batched resident
    call must still take every member's lattice where it lies."""
    p0, ob0, c0 = random_case(lbm, 128, 128, 41, walls=False)
    params = [lbm.Params(128, 128, 400, 10, 0.1, float(np.float32(0.004 + 0.001 * i)), float(np.float32(1.6 + 0.03 * i)))
              for i in range(8)]
    obstacles = [np.roll(ob0, i, axis=1) for i in range(8)]
    cells = [np.roll(c0, i, axis=0) for i in range(8)]
    calls = [2, 300, 3, 95]
    with lbm.Batch(params, obstacles, cells) as plain, lbm.Batch(params, obstacles, cells) as batch:
        assert batch.info()["resident_steps"] > 0 and batch.info()["resident_min_steps"] > 3
        batch.member(3).set_frames(100, 8)
        for n in calls:
            plain.run(n)
            batch.run(n)
        for i in range(8):
            ref = cells[i].copy()
            oracle.run(params[i], ref, obstacles[i], sum(calls))
            assert np.array_equal(batch.member(i).cells().view(np.uint32), ref.view(np.uint32)), i
            assert np.array_equal(batch.member(i).cells().view(np.uint32), plain.member(i).cells().view(np.uint32)), i
        steps, frames = batch.member(3).frames()
        _, want = oracle_frames(oracle, params[3], obstacles[3], cells[3], 0, sum(calls), 100)
        assert_frames(steps, frames, want)
        s_steps, s_frames = run_engine(lbm, params[3], obstacles[3], cells[3], calls, 100)[2:4]
        assert np.array_equal(s_frames.view(np.uint32), frames.view(np.uint32))


def hosted_rank_main(rank, world, port, calls, every, out_dir):
    """One rank of a hosted world (lbm_create_rank_hosted, halo rows over gloo): the calls with frames armed, then
    the same run issued as calls split at the frame steps, without frames."""
    import os
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import conftest
        lbm = conftest.load_package()
        p, ob, cells = random_case(lbm, 128, 96, 23, walls=False)

        def exchange(plan, bufs):
            ops = [dist.P2POp(dist.isend if op["is_send"] else dist.irecv, torch.from_numpy(buf), op["peer"])
                   for op, buf in zip(plan, bufs)]
            for req in dist.batch_isend_irecv(ops):
                req.wait()

        def allreduce(values):
            dist.all_reduce(torch.from_numpy(values), op=dist.ReduceOp.SUM)

        out = {}
        for label, run_calls, e in (("armed", calls, every), ("split", model.split_calls(calls, every), 0)):
            with lbm.Engine(p, ob, cells, rank=rank, world_size=world, device=0, host_comm=(exchange, allreduce)) as eng:
                if e:
                    eng.set_frames(e, 1 + sum(calls) // e)
                got_steps, got_frames = [], []
                for n in run_calls:
                    eng.run(n)
                    s_, f_ = eng.frames()
                    got_steps.append(s_)
                    got_frames.append(f_)
                info = eng.info()
                out[label + "_cells"] = eng.cells()
                out[label + "_av"] = eng.av_vels(sum(calls))
                out[label + "_steps"] = np.concatenate(got_steps)
                out[label + "_frames"] = np.concatenate(got_frames)
        out["rows"] = np.array([info["row_first"], info["row_count"]])
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_hosted_two_rank_world(lbm, oracle, tmp_path):
    """Two ranks on one device, halo rows through the host over gloo: each rank's frames are its rows of the oracle's
    frames; the lattice is the oracle's and av_vels equals the run split at the frame steps."""
    import socket
    import torch
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.set_num_threads(1)
    calls, every = [57, 203], 25
    mp.spawn(hosted_rank_main, args=(2, port, calls, every, str(tmp_path)), nprocs=2, join=True)
    p, ob, cells = random_case(lbm, 128, 96, 23, walls=False)
    ref, want = oracle_frames(oracle, p, ob, cells, 0, sum(calls), every)
    for rank in range(2):
        d = np.load(tmp_path / f"rank{rank}.npz")
        first, count = (int(v) for v in d["rows"])
        assert (first, count) == lbm.partition_rows(p.ny, 2, rank)
        assert d["armed_steps"].tolist() == sorted(want)
        for i, tt in enumerate(d["armed_steps"].tolist()):
            assert np.array_equal(d["armed_frames"][i].view(np.uint32), want[tt][first:first + count].view(np.uint32)), (rank, tt)
        assert np.array_equal(d["armed_cells"].view(np.uint32), ref[first:first + count].view(np.uint32)), rank
        assert np.array_equal(d["armed_cells"].view(np.uint32), d["split_cells"].view(np.uint32)), rank
        assert np.array_equal(d["armed_av"].view(np.uint32), d["split_av"].view(np.uint32)), rank
        assert d["split_steps"].size == 0
