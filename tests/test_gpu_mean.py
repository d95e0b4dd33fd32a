"""Mean flow fields (lbm_set_mean / Engine.set_mean): per-cell float64 sums of u_x, u_y, |u| and pressure over the samples
taken after every global timestep tt with tt % every == 0, accumulated by the running kernels.  The sums are DEFINED
(acc = acc + (double)sample in step order), so every comparison is bit for bit, as uint64 views, against the CPU model
(tests/mean_model.py).  Recording never changes the lattice; av_vels stays bit-identical on the resident path and equal to
the run split at the sample steps on the per-pass paths."""
import numpy as np
import pytest

import mean_model
import test_frames_format as model
from mean_model import FIELDS
from test_gpu_frames import PER_PASS
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu


def assert_sums(got, n, want, want_n, what=""):
    assert n == want_n, (what, n, want_n)
    for k in FIELDS:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), f"{what}: sum of {k} differs"


def run_engine(lbm, p, ob, cells, calls, every=0, n_gpus=1):
    """Run `calls` from step 0, the mean fields armed before the first call; the sums are read once, at the end."""
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        if every:
            eng.set_mean(every)
        for n in calls:
            eng.run(n)
        sums, n = eng.mean_sums() if every else (None, 0)
        return eng.cells(), eng.av_vels(sum(calls)), sums, n, eng.info()


def check_resident(lbm, oracle, p, ob, cells, calls, every):
    ref, want, want_n = mean_model.oracle_sums(oracle, p, ob, cells, 0, sum(calls), every)
    got, av, sums, n, info = run_engine(lbm, p, ob, cells, calls, every)
    assert info["resident_steps"] > 0
    assert_sums(sums, n, want, want_n, f"every={every}")
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    base, base_av, _, _, _ = run_engine(lbm, p, ob, cells, calls)
    assert np.array_equal(base.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(base_av.view(np.uint32), av.view(np.uint32)), "the mean fields changed av_vels on the resident path"


@pytest.mark.parametrize("name,calls,everys", [("128x128", [301], (100, 7, 1)), ("128x128", [50, 251], (100, 7, 1)),
                                               ("128x256", [50, 251], (100, 7)), ("256x256", [301], (100, 1)),
                                               ("1024x1024", [50, 251], (100,))])
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
    """Obstacles on the lid row and on the seam rows of the bands; two-row bands at 512 and at 1024 threads, one XCD and
    grouped workgroups, and -- 128 x 64 with LBM_RESIDENT_ROWS=4 only -- four-row JOINT bands (LBM_RESIDENT_JOINT has no say
    under the two-row bands the planner prefers at these sizes; tests/resident_forms.py has the table): both lid
    placements accumulate across four launches.  The four-row forms without JOINT and at 1024 threads:
    tests/test_gpu_resident_forms.py."""
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
    """A 4100-step call runs two launches (4096 + 4): a sample on the last step of the first (accel_last) and one on the
    first step of the second."""
    p, ob, cells = random_case(lbm, 128, 128, 5, walls=False)
    p.max_iters = 4100
    check_resident(lbm, oracle, p, ob, cells, [4100], every)


def test_accumulation_across_paths(lbm, oracle):
    """Armed at step 130; a per-pass short call, a resident call and another short one add to the same sums: a resident
    launch that started from zero instead of from the buffer (or the reverse) would show."""
    p, ob, cells = random_case(lbm, 128, 128, 9, walls=False)
    p.max_iters = 400
    start = cells.copy()
    oracle.run(p, start, ob, 130)
    ref, want, want_n = mean_model.oracle_sums(oracle, p, ob, start, 130, 335, 10)
    assert want_n == 21
    with lbm.Engine(p, ob, cells) as eng:
        info = eng.info()
        assert info["resident_steps"] > 0 and 3 < info["resident_min_steps"] <= 200
        eng.run(130)
        eng.set_mean(10)
        for n in (3, 200, 2):
            eng.run(n)
        sums, n = eng.mean_sums()
        assert_sums(sums, n, want, 21)
        assert np.array_equal(eng.cells().view(np.uint32), ref.view(np.uint32))
        mean = eng.mean()
        assert mean["samples"] == 21
        for k in FIELDS:
            assert np.array_equal(mean[k].view(np.uint64), (want[k] / 21.0).view(np.uint64))


def test_read_does_not_reset_and_rearm_does(lbm, oracle, monkeypatch):
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "16")
    p, ob, cells = random_case(lbm, 128, 128, 13, walls=False)
    _, want60, n60 = mean_model.oracle_sums(oracle, p, ob, cells, 0, 60, 7)
    ref100, want100, n100 = mean_model.oracle_sums(oracle, p, ob, cells, 0, 100, 7)
    _, window, n_window = mean_model.oracle_sums(oracle, p, ob, ref100, 100, 160, 7)
    with lbm.Engine(p, ob, cells) as eng:
        eng.set_mean(7)
        sums, n = eng.mean_sums()
        assert n == 0 and all(not sums[k].any() for k in FIELDS)
        with pytest.raises(lbm.LbmError, match="no sample"):
            eng.mean()
        eng.run(60)
        first, n1 = eng.mean_sums()
        again, n2 = eng.mean_sums()
        assert_sums(first, n1, want60, n60, "first read")
        assert_sums(again, n2, want60, n60, "second read")
        eng.run(40)
        assert_sums(*eng.mean_sums(), want100, n100, "after running on")
        eng.set_mean(7)                      # re-arming: zero sums, zero count, and the window from here
        sums, n = eng.mean_sums()
        assert n == 0 and all(not sums[k].any() for k in FIELDS)
        eng.run(60)
        assert_sums(*eng.mean_sums(), window, n_window, "window after re-arming")
        eng.set_mean(3)
        sums, n = eng.mean_sums()
        assert n == 0 and all(not sums[k].any() for k in FIELDS)
        eng.set_mean(0)
        with pytest.raises(lbm.LbmError, match="not armed"):
            eng.mean_sums()
        eng.run(20)                          # disarmed: runs as ever


@pytest.mark.parametrize("env,n_gpus,every,launch", [
    (dict(PER_PASS, LBM_FUSE2="1"), 1, 25, (2, 3)),                                   # stream kernel, K = 2 / 3
    (dict(PER_PASS, LBM_FUSE2="1", LBM_PASS_STEPS="4", LBM_LANE_CELLS="4"), 1, 25, (4,)),  # K = 4, packed
    (dict(PER_PASS, LBM_FUSE2="0"), 1, 25, (1,)),                                     # one-step kernel
    (dict(PER_PASS, LBM_TILE_STEPS="4"), 1, 25, (4,)),                                # LDS-tile kernel
    (dict(PER_PASS, LBM_GRAPH="1"), 1, 150, None),     # segments of 94 and 109 steps: hipGraph chunks are replayed
    ({"LBM_HALO": "memcpy"}, 2, 25, None), ({"LBM_HALO": "memcpy"}, 3, 25, None)])
def test_per_pass_families(lbm, oracle, monkeypatch, env, n_gpus, every, launch):
    """Calls the resident kernel does not serve end their passes at every sample step, each followed by one accumulation
    pass over every slab: the sums match the model, the lattice and av_vels the same run issued as calls split there."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
    calls = [57, 203]
    ref, want, want_n = mean_model.oracle_sums(oracle, p, ob, cells, 0, sum(calls), every)
    got, av, sums, n, info = run_engine(lbm, p, ob, cells, calls, every, n_gpus=n_gpus)
    assert info["resident_steps"] == 0 and info["n_slabs"] == n_gpus
    if launch:
        assert info["steps_per_launch"] in launch, info
    if env.get("LBM_GRAPH") == "1":
        assert info["graph_steps"] > 0 and info["graph_steps"] < 94, info
    assert_sums(sums, n, want, want_n)
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    split = model.split_calls(calls, every)
    base, base_av, _, _, _ = run_engine(lbm, p, ob, cells, split, n_gpus=n_gpus)
    assert np.array_equal(base.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(base_av.view(np.uint32), av.view(np.uint32))


def batch_inputs(lbm, seed):
    p0, ob0, c0 = random_case(lbm, 128, 128, seed, walls=False)
    params = [lbm.Params(128, 128, 400, 10, 0.1, float(np.float32(0.004 + 0.001 * i)), float(np.float32(1.6 + 0.03 * i)))
              for i in range(8)]
    return params, [np.roll(ob0, i, axis=1) for i in range(8)], [np.roll(c0, i, axis=0) for i in range(8)]


def test_batch_members_armed_independently(lbm, oracle):
    params, obstacles, cells = batch_inputs(lbm, 31)
    armed = {0: 50, 3: 7}
    calls = [120, 180]
    with lbm.Batch(params, obstacles, cells) as plain, lbm.Batch(params, obstacles, cells) as batch:
        assert batch.info()["resident_steps"] > 0
        for i, e in armed.items():
            batch.member(i).set_mean(e)
        for n in calls:
            plain.run(n)
            batch.run(n)
        for i in range(8):
            m, q = batch.member(i), plain.member(i)
            assert np.array_equal(m.cells().view(np.uint32), q.cells().view(np.uint32)), i
            assert np.array_equal(m.av_vels().view(np.uint32), q.av_vels().view(np.uint32)), i
            if i in armed:
                sums, n = m.mean_sums()
                _, want, want_n = mean_model.oracle_sums(oracle, params[i], obstacles[i], cells[i], 0, sum(calls), armed[i])
                assert_sums(sums, n, want, want_n, f"member {i}")
                single, single_n = run_engine(lbm, params[i], obstacles[i], cells[i], calls, armed[i])[2:4]
                assert_sums(sums, n, single, single_n, f"member {i} against a single Engine")
            else:
                with pytest.raises(lbm.LbmError, match="not armed"):
                    m.mean_sums()


def test_batch_short_call_then_resident(lbm, oracle):
    """A call below resident_min_steps runs the members one by one on the per-pass kernels; the armed member's call is
    split at its sample steps, so its lattice may end in the other buffer and is copied to the batch's parity.  The
    batched resident calls that follow must take every lattice where it lies and add to the same sums."""
    params, obstacles, cells = batch_inputs(lbm, 41)
    calls = [2, 300, 3, 95]
    with lbm.Batch(params, obstacles, cells) as plain, lbm.Batch(params, obstacles, cells) as batch:
        assert batch.info()["resident_steps"] > 0 and batch.info()["resident_min_steps"] > 3
        batch.member(3).set_mean(100)
        for n in calls:
            plain.run(n)
            batch.run(n)
        for i in range(8):
            ref = cells[i].copy()
            oracle.run(params[i], ref, obstacles[i], sum(calls))
            assert np.array_equal(batch.member(i).cells().view(np.uint32), ref.view(np.uint32)), i
            assert np.array_equal(batch.member(i).cells().view(np.uint32), plain.member(i).cells().view(np.uint32)), i
        _, want, want_n = mean_model.oracle_sums(oracle, params[3], obstacles[3], cells[3], 0, sum(calls), 100)
        assert_sums(*batch.member(3).mean_sums(), want, want_n, "member 3")


def test_refused_in_stale_and_freshest_halo_modes(lbm, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_mean.*halo mode"):
                eng.set_mean(10)
        eng.set_halo_mode("sync")
        eng.set_mean(10)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match="mean fields are armed"):
                eng.set_halo_mode(mode)
        assert eng.info()["halo_mode"] == 0


def test_one_recorder_per_context_and_no_steady_runs(lbm):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_read_mean.*not armed"):
            eng.mean_sums()
        eng.set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_mean: animation frames are armed"):
            eng.set_mean(10)
        eng.set_frames(0)
        eng.set_probes([(5, 5)], 1, 16)
        with pytest.raises(lbm.LbmError, match="lbm_set_mean: point probes are armed"):
            eng.set_mean(10)
        eng.set_probes([], 0, 0)
        eng.set_mean(10)
        with pytest.raises(lbm.LbmError, match="lbm_set_frames: mean fields are armed"):
            eng.set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_probes: mean fields are armed"):
            eng.set_probes([(5, 5)], 1, 16)
        with pytest.raises(lbm.LbmError, match="lbm_run_until: mean fields are armed"):
            eng.run_until(100, 10)
        assert eng.info()["steps_done"] == 0
        assert eng.mean_sums()[1] == 0       # still armed, nothing sampled
        assert eng.lib.lbm_set_mean(eng.handle, -1) != 0     # (Engine.set_mean refuses it before the library sees it)
        assert b"lbm_set_mean: negative interval" in eng.lib.lbm_last_error()
        assert eng.mean_sums()[1] == 0


def test_a_batch_records_one_kind(lbm):
    params, obstacles, cells = batch_inputs(lbm, 7)
    with lbm.Batch(params[:3], obstacles[:3], cells[:3]) as batch:
        batch.member(1).set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_mean: a member of this batch has animation frames armed"):
            batch.member(0).set_mean(10)
        batch.member(1).set_frames(0)
        batch.member(0).set_mean(10)
        with pytest.raises(lbm.LbmError, match="lbm_set_probes: a member of this batch has mean fields armed"):
            batch.member(2).set_probes([(1, 1)], 1, 4)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run_until: mean fields are armed"):
            batch.run_until(100, 10)
        with pytest.raises(lbm.LbmError, match="not armed"):
            batch.member(1).mean_sums()


def test_cli_writes_mean_state(lbm, oracle, datasets, tmp_path):
    """d2q9-bgk with LBM_MEAN=10:100 on 128^2 for 250 steps: 15 samples (tt = 100, 110, ..., 240); mean_state.dat is
    byte-identical to the Python twin fed with the model's means; final_state.dat and av_vels.dat as without it."""
    import hashlib
    import os
    import subprocess
    from conftest import GOLDEN
    p, ob = datasets("128x128")
    p.max_iters = 250
    of = os.path.join(GOLDEN, "inputs", "obstacles_128x128.dat")
    outs = {}
    for label, extra in (("plain", {}), ("mean", {"LBM_MEAN": "10:100"})):
        d = tmp_path / label
        d.mkdir()
        pf = d / "input.params"
        pf.write_text("%d\n%d\n%d\n%d\n%.9g\n%.9g\n%.9g\n" % (p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel,
                                                           p.omega))
        out = subprocess.run([lbm.CLI_PATH, str(pf), of], cwd=d, capture_output=True, text=True,
                             env=dict(os.environ, **extra), timeout=120)
        assert out.returncode == 0, out.stderr
        outs[label] = (d, out.stdout)
    d, stdout = outs["mean"]
    for name in ("final_state.dat", "av_vels.dat"):
        md5 = [hashlib.md5((outs[k][0] / name).read_bytes()).hexdigest() for k in ("plain", "mean")]
        assert md5[0] == md5[1], name
    assert [l for l in stdout.splitlines() if l.startswith("Mean over")] == ["Mean over 15 samples"]
    assert stdout.index("Mean over") < stdout.index("==done==")
    assert "Mean over" not in outs["plain"][1] and not (outs["plain"][0] / "mean_state.dat").exists()
    start = oracle.init_cells(p)
    oracle.run(p, start, ob, 100)
    _, sums, n = mean_model.oracle_sums(oracle, p, ob, start, 100, 250, 10)
    assert n == 15
    twin = tmp_path / "twin.dat"
    lbm.write_mean_state(str(twin), mean_model.means_of(sums, n), ob)
    assert (d / "mean_state.dat").read_bytes() == twin.read_bytes()
