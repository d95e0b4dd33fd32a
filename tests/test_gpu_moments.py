"""Second moments of the mean fields (lbm_set_mean_order(ctx, every, 2) / Engine.set_mean_order): per-cell float64 sums of
u_x u_x, u_y u_y, u_x u_y and pressure pressure over the samples of the mean fields, accumulated by the running kernels.
The sums are DEFINED (acc = acc + (double)a * (double)b in step order, the product exact), so every comparison is bit for
bit, as uint64 views, against the CPU model (tests/moments_model.py).  Every test also holds planes 0-3 to the order-1
model (tests/mean_model.py) and the lattice and av_vels to an unarmed run."""
import numpy as np
import pytest

import mean_model
import moments_model
import test_frames_format as model
from mean_model import FIELDS
from moments_model import FIELDS2
from test_gpu_frames import PER_PASS
from test_gpu_mean import assert_sums, batch_inputs
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu

_models = {}


def model_sums(oracle, key, p, ob, cells, start, total, every):
    """moments_model.oracle_sums2, computed once per case and shared; the first-moment sums are checked against
    mean_model.oracle_sums (the order-1 model) where they are made."""
    if key not in _models:
        ref, sums, sums2, n = moments_model.oracle_sums2(oracle, p, ob, cells, start, total, every)
        ref1, sums1, n1 = mean_model.oracle_sums(oracle, p, ob, cells, start, total, every)
        assert n == n1 and np.array_equal(ref, ref1)
        for k in FIELDS:
            assert np.array_equal(sums[k].view(np.uint64), sums1[k].view(np.uint64))
        for v in (ref, *sums.values(), *sums2.values()):
            v.setflags(write=False)
        _models[key] = (ref, sums, sums2, n)
    return _models[key]


def assert_sums2(got, n, want, want_n, what=""):
    assert n == want_n, (what, n, want_n)
    assert tuple(got) == FIELDS2
    for k in FIELDS2:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), f"{what}: sum of {k} differs"


def run_engine(lbm, p, ob, cells, calls, every=0, order=2, n_gpus=1):
    """Run `calls` from step 0, armed before the first call; all sums are read once, at the end."""
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus) as eng:
        if every:
            eng.set_mean_order(every, order)
        for n in calls:
            eng.run(n)
        sums, n = eng.mean_sums() if every else (None, 0)
        sums2, n2 = eng.moment_sums() if every and order == 2 else (None, n)
        assert n2 == n
        return eng.cells(), eng.av_vels(sum(calls)), sums, sums2, n, eng.info()


def check_resident(lbm, oracle, key, p, ob, cells, calls, every):
    ref, want, want2, want_n = model_sums(oracle, key, p, ob, cells, 0, sum(calls), every)
    got, av, sums, sums2, n, info = run_engine(lbm, p, ob, cells, calls, every)
    assert info["resident_steps"] > 0
    assert_sums(sums, n, want, want_n, f"every={every}")
    assert_sums2(sums2, n, want2, want_n, f"every={every}")
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    base, base_av, _, _, _, _ = run_engine(lbm, p, ob, cells, calls)
    assert np.array_equal(base.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(base_av.view(np.uint32), av.view(np.uint32)), "the second moments changed av_vels on the resident path"


@pytest.mark.parametrize("nx,ny,env", [(128, 16, {}), (128, 64, {"LBM_RESIDENT_ROWS": "4"}),
                                       (320, 24, {"LBM_RESIDENT_JOINT": "1"}),
                                       (128, 128, {"LBM_RESIDENT_ONE_XCD": "0", "LBM_RESIDENT_GROUP": "4"}),
                                       (1024, 64, {})])
def test_resident_forms(lbm, oracle, monkeypatch, nx, ny, env):
    """Shapes 1, 3, 1, 1 and 0 of the resident kernel (tests/resident_forms.py): two-row bands, four-row JOINT bands
    (128 x 64 with LBM_RESIDENT_ROWS=4), two-row bands again at 320 x 24 -- LBM_RESIDENT_JOINT=1 has no say there --,
    grouped workgroups, and the 1024-thread form with two-row bands; obstacles on the lid row and on the seam rows of the
    bands; four launches accumulate into the same eight planes.  Shapes 2 and 4: tests/test_gpu_resident_forms.py."""
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, ob, cells = random_case(lbm, nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
    ob[ny - 2, ::5] = 1                     # lid row
    ob[3::4, ::7] = 1                       # seam rows of four-row bands
    ob[0::4, 3::7] = 1
    check_resident(lbm, oracle, ("forms", nx, ny), p, ob, cells, [1, 2, 19, 5], 3)


@pytest.mark.parametrize("every", [4095, 4096])
def test_resident_chunk_boundary(lbm, oracle, every):
    """A 4100-step call runs two launches (4096 + 4): a sample on the last step of the first and one on the first step of
    the second."""
    p, ob, cells = random_case(lbm, 128, 128, 5, walls=False)
    p.max_iters = 4100
    check_resident(lbm, oracle, ("chunk", every), p, ob, cells, [4100], every)


def test_accumulation_across_paths_and_not_vacuous(lbm, oracle):
    """Armed at step 130; a per-pass short call, a resident call and another short one add to the same eight planes.  The
    u_x u_y plane holds both signs, u_x u_x is non-zero on every fluid cell and +0.0 on every blocked one."""
    p, ob, cells = random_case(lbm, 128, 128, 9, walls=False)
    p.max_iters = 400
    start = cells.copy()
    oracle.run(p, start, ob, 130)
    ref, want, want2, want_n = model_sums(oracle, "across", p, ob, start, 130, 335, 10)
    assert want_n == 21
    # the model itself (on the CPU): the seed gives a plane worth comparing
    blocked = ob != 0
    assert (want2["u_x u_y"] > 0).any() and (want2["u_x u_y"] < 0).any()
    assert (want2["u_x u_x"][~blocked] != 0).all()
    assert not want2["u_x u_x"][blocked].view(np.uint64).any()
    base = cells.copy()
    base_av = oracle.run(p, base, ob, 335)
    with lbm.Engine(p, ob, cells) as plain:
        for n in (130, 3, 200, 2):
            plain.run(n)
        plain_cells, plain_av = plain.cells(), plain.av_vels(335)
    with lbm.Engine(p, ob, cells) as eng:
        info = eng.info()
        assert info["resident_steps"] > 0 and 3 < info["resident_min_steps"] <= 200
        eng.run(130)
        eng.set_mean_order(10, 2)
        for n in (3, 200, 2):
            eng.run(n)
        sums, n = eng.mean_sums()
        sums2, n2 = eng.moment_sums()
        assert_sums(sums, n, want, 21)
        assert_sums2(sums2, n2, want2, 21)
        assert (sums2["u_x u_y"] > 0).any() and (sums2["u_x u_y"] < 0).any()
        assert (sums2["u_x u_x"][~blocked] != 0).all()
        assert not sums2["u_x u_x"][blocked].view(np.uint64).any()       # exactly +0.0
        assert np.array_equal(eng.cells().view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(eng.cells().view(np.uint32), plain_cells.view(np.uint32))
        assert np.array_equal(base.view(np.uint32), plain_cells.view(np.uint32))
        # the armed run splits its per-pass calls after their sample steps (tt = 130, in the call of 3); the resident call
        # holds the samples 140 .. 330 and is not split: av_vels of the plain run with the first short call split
        with lbm.Engine(p, ob, cells) as split:
            for n in (130, 1, 2, 200, 2):
                split.run(n)
            assert np.array_equal(eng.av_vels(335).view(np.uint32), split.av_vels(335).view(np.uint32))
        assert np.allclose(plain_av, base_av, rtol=2e-4, atol=0)
        f = eng.fluctuations()
        twin = lbm.fluctuations_of(want, want2, 21)
        assert f["samples"] == 21
        for k in twin:
            if k != "samples":
                assert np.array_equal(f[k].view(np.uint64), twin[k].view(np.uint64)), k
        assert (f["rms_u_x"][~blocked] > 0).any() and not f["rms_u_x"][blocked].any()


def test_order_1_then_order_2_rearm(lbm, oracle, monkeypatch):
    monkeypatch.setenv("LBM_RESIDENT_MIN_STEPS", "16")
    p, ob, cells = random_case(lbm, 128, 128, 13, walls=False)
    ref40, want40, n40 = mean_model.oracle_sums(oracle, p, ob, cells, 0, 40, 7)
    ref100, w1, w2, n_w = model_sums(oracle, "rearm-window", p, ob, ref40, 40, 100, 7)
    ref130, last, n_last = mean_model.oracle_sums(oracle, p, ob, ref100, 100, 130, 7)
    with lbm.Engine(p, ob, cells) as plain:
        for n in (40, 60, 30):
            plain.run(n)
        plain_cells, plain_av = plain.cells(), plain.av_vels(130)
    with lbm.Engine(p, ob, cells) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_read_mean2.*not armed"):
            eng.moment_sums()
        eng.set_mean_order(7, 1)
        eng.run(40)
        with pytest.raises(lbm.LbmError, match=r"lbm_read_mean2: the second moments are not armed \(lbm_set_mean_order\(ctx, every, 2\)\)"):
            eng.moment_sums()
        assert_sums(*eng.mean_sums(), want40, n40, "order 1")
        eng.set_mean_order(7, 2)
        sums, n = eng.mean_sums()
        sums2, n2 = eng.moment_sums()
        assert n == 0 and n2 == 0
        assert all(not sums[k].view(np.uint64).any() for k in FIELDS) and all(not sums2[k].view(np.uint64).any() for k in FIELDS2)
        with pytest.raises(lbm.LbmError, match="no sample"):
            eng.fluctuations()
        eng.run(60)
        assert_sums(*eng.mean_sums(), w1, n_w, "order 2 window")
        assert_sums2(*eng.moment_sums(), w2, n_w, "order 2 window")
        assert_sums2(*eng.moment_sums(), w2, n_w, "second read")
        eng.set_mean(7)                      # order 1 again
        with pytest.raises(lbm.LbmError, match="lbm_read_mean2.*not armed"):
            eng.moment_sums()
        eng.run(30)
        assert_sums(*eng.mean_sums(), last, n_last, "order 1 again")
        assert np.array_equal(eng.cells().view(np.uint32), ref130.view(np.uint32))
        assert np.array_equal(eng.cells().view(np.uint32), plain_cells.view(np.uint32))
        assert np.array_equal(eng.av_vels(130).view(np.uint32), plain_av.view(np.uint32))
        eng.set_mean_order(0, 2)             # disarms at either order
        with pytest.raises(lbm.LbmError, match="not armed"):
            eng.mean_sums()


def test_batch_mixes_orders(lbm, oracle):
    params, obstacles, cells = batch_inputs(lbm, 31)
    armed = {0: (5, 2), 1: (7, 2), 2: (5, 2), 3: (7, 2), 4: (5, 1), 5: (7, 1)}
    with lbm.Batch(params, obstacles, cells) as plain, lbm.Batch(params, obstacles, cells) as batch:
        assert batch.info()["resident_steps"] > 0
        for i, (e, order) in armed.items():
            batch.member(i).set_mean_order(e, order)
        plain.run(120)
        batch.run(120)
        for i in range(8):
            m, q = batch.member(i), plain.member(i)
            assert np.array_equal(m.cells().view(np.uint32), q.cells().view(np.uint32)), i
            assert np.array_equal(m.av_vels().view(np.uint32), q.av_vels().view(np.uint32)), i
            if i not in armed:
                with pytest.raises(lbm.LbmError, match="not armed"):
                    m.mean_sums()
                with pytest.raises(lbm.LbmError, match="lbm_read_mean2.*not armed"):
                    m.moment_sums()
                continue
            every, order = armed[i]
            ref, want, want2, want_n = model_sums(oracle, ("batch", i), params[i], obstacles[i], cells[i], 0, 120, every)
            assert np.array_equal(m.cells().view(np.uint32), ref.view(np.uint32)), i
            assert_sums(*m.mean_sums(), want, want_n, f"member {i}")
            if order == 2:
                assert_sums2(*m.moment_sums(), want2, want_n, f"member {i}")
            else:
                with pytest.raises(lbm.LbmError, match="lbm_read_mean2: the second moments are not armed"):
                    m.moment_sums()


@pytest.mark.parametrize("env,n_gpus,every,launch", [
    (dict(PER_PASS, LBM_FUSE2="1"), 1, 25, (2, 3)),                                   # stream kernel, K = 2 / 3
    (dict(PER_PASS, LBM_FUSE2="1", LBM_PASS_STEPS="4", LBM_LANE_CELLS="4"), 1, 25, (4,)),  # K = 4, packed
    (dict(PER_PASS, LBM_FUSE2="0"), 1, 25, (1,)),                                     # one-step kernel
    (dict(PER_PASS, LBM_TILE_STEPS="4"), 1, 25, (4,)),                                # LDS-tile kernel
    (dict(PER_PASS, LBM_GRAPH="1"), 1, 150, None),     # segments of 94 and 109 steps: hipGraph chunks are replayed
    ({"LBM_HALO": "memcpy"}, 2, 25, None), ({"LBM_HALO": "memcpy"}, 3, 25, None)])
def test_per_pass_families(lbm, oracle, monkeypatch, env, n_gpus, every, launch):
    """Calls the resident kernel does not serve end their passes at every sample step, each followed by one accumulation
    pass over every slab (mean_accumulate at order 2): the sums match the model, the lattice and av_vels the same run
    issued as calls split there; several slabs are stitched by their rows."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, ob, cells = random_case(lbm, 128, 96, 21, walls=False)
    calls = [57, 203]
    ref, want, want2, want_n = model_sums(oracle, ("per-pass", every), p, ob, cells, 0, sum(calls), every)
    got, av, sums, sums2, n, info = run_engine(lbm, p, ob, cells, calls, every, n_gpus=n_gpus)
    assert info["resident_steps"] == 0 and info["n_slabs"] == n_gpus
    if launch:
        assert info["steps_per_launch"] in launch, info
    if env.get("LBM_GRAPH") == "1":
        assert info["graph_steps"] > 0 and info["graph_steps"] < 94, info
    assert_sums(sums, n, want, want_n)
    assert_sums2(sums2, n, want2, want_n)
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    split = model.split_calls(calls, every)
    base, base_av, _, _, _, _ = run_engine(lbm, p, ob, cells, split, n_gpus=n_gpus)
    assert np.array_equal(base.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(base_av.view(np.uint32), av.view(np.uint32))


def test_refusals_name_the_function(lbm, monkeypatch):
    p, ob, cells = random_case(lbm, 128, 128, 3, walls=False)
    with lbm.Engine(p, ob, cells) as eng:
        for order in (0, 3):
            with pytest.raises(lbm.LbmError, match="set_mean_order: order must be 1"):
                eng.set_mean_order(10, order)                # the binding's check
            assert eng.lib.lbm_set_mean_order(eng.handle, 10, order) != 0
            assert b"lbm_set_mean_order: order %d" % order in eng.lib.lbm_last_error()
        with pytest.raises(lbm.LbmError, match="lbm_read_mean.*not armed"):
            eng.mean_sums()                                  # the refused calls armed nothing
        assert eng.lib.lbm_set_mean_order(eng.handle, -1, 2) != 0
        assert b"lbm_set_mean_order: negative interval" in eng.lib.lbm_last_error()
        eng.set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_mean_order: animation frames are armed"):
            eng.set_mean_order(10, 2)
        eng.set_frames(0)
        eng.set_probes([(5, 5)], 1, 16)
        with pytest.raises(lbm.LbmError, match="lbm_set_mean_order: point probes are armed"):
            eng.set_mean_order(10, 2)
        eng.set_probes([], 0, 0)
        eng.set_mean_order(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_set_frames: mean fields are armed"):
            eng.set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_run_until: mean fields are armed"):
            eng.run_until(100, 10)
        assert eng.info()["steps_done"] == 0
        assert eng.moment_sums()[1] == 0 and eng.mean_sums()[1] == 0      # still armed, nothing sampled
        n = lbm.ctypes.c_longlong(-1)
        assert eng.lib.lbm_read_mean2(eng.handle, None, None, None, None, lbm.ctypes.byref(n)) == 0 and n.value == 0
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, n_gpus=2) as eng:
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="lbm_set_mean_order.*halo mode"):
                eng.set_mean_order(10, 2)
        eng.set_halo_mode("sync")
        eng.set_mean_order(10, 2)
        for mode in ("stale", "freshest"):
            with pytest.raises(lbm.LbmError, match="mean fields are armed"):
                eng.set_halo_mode(mode)


def test_refused_on_a_rank_context(lbm):
    """A rank context (one rank, host message passing that is never called) refuses order 2 as it refuses order 1."""
    p, ob, cells = random_case(lbm, 128, 64, 4, walls=False)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        with pytest.raises(lbm.LbmError, match="lbm_set_mean_order: not available in a multi-process"):
            eng.set_mean_order(10, 2)


def test_batch_records_one_kind_at_order_2(lbm):
    params, obstacles, cells = batch_inputs(lbm, 7)
    with lbm.Batch(params[:3], obstacles[:3], cells[:3]) as batch:
        batch.member(1).set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="lbm_set_mean_order: a member of this batch has animation frames armed"):
            batch.member(0).set_mean_order(10, 2)
        batch.member(1).set_frames(0)
        batch.member(0).set_mean_order(10, 2)
        with pytest.raises(lbm.LbmError, match="lbm_set_probes: a member of this batch has mean fields armed"):
            batch.member(2).set_probes([(1, 1)], 1, 4)
        with pytest.raises(lbm.LbmError, match="lbm_batch_run_until: mean fields are armed"):
            batch.run_until(100, 10)


def test_cli_writes_rms_state(lbm, oracle, datasets, tmp_path):
    """d2q9-bgk with LBM_MEAN=10:100 LBM_MEAN_ORDER=2 on 128^2 for 250 steps: rms_state.dat is byte-identical to the
    Python twin fed with the model's sums; the other three files as with LBM_MEAN alone."""
    import os
    import subprocess
    from conftest import GOLDEN
    p, ob = datasets("128x128")
    p.max_iters = 250
    of = os.path.join(GOLDEN, "inputs", "obstacles_128x128.dat")
    outs = {}
    for label, extra in (("mean", {"LBM_MEAN": "10:100"}), ("rms", {"LBM_MEAN": "10:100", "LBM_MEAN_ORDER": "2"}),
                         ("one", {"LBM_MEAN": "10:100", "LBM_MEAN_ORDER": "1"})):
        d = tmp_path / label
        d.mkdir()
        pf = d / "input.params"
        pf.write_text("%d\n%d\n%d\n%d\n%.9g\n%.9g\n%.9g\n" % (p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel,
                                                           p.omega))
        out = subprocess.run([lbm.CLI_PATH, str(pf), of], cwd=d, capture_output=True, text=True,
                             env=dict(os.environ, **extra), timeout=120)
        assert out.returncode == 0, out.stderr
        assert [l for l in out.stdout.splitlines() if l.startswith("Mean over")] == ["Mean over 15 samples"]
        outs[label] = d
    for name in ("final_state.dat", "av_vels.dat", "mean_state.dat"):
        for label in ("rms", "one"):
            assert (outs[label] / name).read_bytes() == (outs["mean"] / name).read_bytes(), (label, name)
    assert not (outs["mean"] / "rms_state.dat").exists() and not (outs["one"] / "rms_state.dat").exists()
    start = oracle.init_cells(p)
    oracle.run(p, start, ob, 100)
    _, sums, sums2, n = model_sums(oracle, "cli", p, ob, start, 100, 250, 10)
    assert n == 15
    twin = tmp_path / "twin.dat"
    lbm.write_rms_state(str(twin), lbm.fluctuations_of(sums, sums2, n), ob)
    assert (outs["rms"] / "rms_state.dat").read_bytes() == twin.read_bytes()
