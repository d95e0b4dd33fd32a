"""GPU parity: the HIP engine (through the C ABI) against the CPU oracle on the same inputs.

Bar: EXACT mode is BIT-IDENTICAL to the oracle's lattice and per-cell outputs (and therefore to
the reference's SerialCode binary, which the oracle is pinned to).  av_vels differ only by
summation order: the reference adds 10^4..10^8 fp32 terms left to right (rounding noise of order
sqrt(n)*2^-24, 4e-5 observed on 128x256; its own OpenMP variant moves them by 5e-5, SURVEY.md
section 8c), the GPU adds per-wave fp32 partials in double.  So av_vels are compared (a) with the
oracle's sequential fp32 value at 2e-4 relative and (b) with a float64 re-summation of the per-cell |u| the
kernel adds, at the bound derived in tests/av_model.py (test_av_vels_against_float64_resummation here;
every kernel family in tests/test_gpu_av_vels.py).  FAST mode (reciprocal multiplies + FMA) is held to the north-star
tolerance, the check.py rule: max |100*(ref-sim)/sim| <= 1 % on av_vels and on pressure
(/root/reference/check/check.py:83-99,136-148).
"""
import os

import functools

import numpy as np
import pytest

import moments_model
import test_frames_format as frames_model

pytestmark = pytest.mark.gpu

AV_RTOL = 2e-4          # vs the reference's sequential fp32 sum (see module docstring)
CHECK_TOL_PCT = 1.0     # check.py default tolerance (check/check.py:19-24)


def random_case(lbm, nx, ny, seed, blocked_frac=0.05, walls=True):
    """Seeded lattice with positive populations near equilibrium and a random obstacle map."""
    rng = np.random.default_rng(seed)
    p = lbm.Params(nx, ny, 400, 10, 0.1, 0.005, 1.85)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32) * np.float32(p.density)
    cells = (w * (1.0 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    ob = (rng.random((ny, nx)) < blocked_frac).astype(np.int32)
    if walls:
        ob[0, :] = 1
        ob[:, 0] = 1
    ob[ny - 2, nx // 2] = 1          # a blocked cell on the accelerated row
    return p, ob, cells


def run_both(lbm, oracle, p, ob, cells, steps, math="exact", n_gpus=1):
    ref_cells = cells.copy()
    ref_av = oracle.run(p, ref_cells, ob, steps)
    with lbm.Engine(p, ob, cells, n_gpus=n_gpus, math=math) as eng:
        eng.run(steps)
        got_cells = eng.cells()
        got_av = eng.av_vels(steps)
        fields = eng.final_state()
    return ref_cells, ref_av, got_cells, got_av, fields


@pytest.mark.parametrize("name,steps", [("128x128", 1), ("128x128", 2), ("128x128", 37),
                                        ("128x256", 300), ("256x256", 50)])
def test_exact_bitwise_reference_datasets(lbm, oracle, datasets, name, steps):
    p, ob = datasets(name)
    cells = oracle.init_cells(p)
    ref_cells, ref_av, got_cells, got_av, fields = run_both(lbm, oracle, p, ob, cells, steps)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32)), \
        f"{name}: lattice differs after {steps} steps"
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL, atol=0)
    ref_f = oracle.final_state(p, ref_cells, ob)
    for k in ("u_x", "u_y", "u", "pressure"):
        assert np.array_equal(ref_f[k].view(np.uint32), fields[k].view(np.uint32)), k


@pytest.mark.parametrize("nx,ny,seed", [(64, 32, 1), (256, 16, 2), (1024, 8, 3), (2048, 5, 4)])
def test_exact_bitwise_random_lattice(lbm, oracle, nx, ny, seed):
    """Random populations + random obstacles, no side walls: both periodic wraps are live."""
    p, ob, cells = random_case(lbm, nx, ny, seed, walls=False)
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 25)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL, atol=0)


@pytest.mark.parametrize("nx,ny", [(7, 6), (130, 9), (33, 4), (1, 5), (3, 2)])
def test_exact_bitwise_ragged_widths(lbm, oracle, nx, ny):
    """Widths that are not a multiple of 4 take the one-cell-per-lane kernel."""
    p, ob, cells = random_case(lbm, nx, ny, 7 + nx, blocked_frac=0.1, walls=False)
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 12)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL, atol=1e-12)


@pytest.mark.parametrize("resident,speed", [("0", "relaxed"), ("1", "moment")])
def test_av_vels_against_float64_resummation(lbm, oracle, datasets, monkeypatch, resident, speed):
    """Tight av_vels check: every step within av_model.bound(info) of a float64 sum of the per-cell values the kernel
    adds (tests/av_model.py; every kernel family is held to it in test_gpu_av_vels.py).  The LDS-tile and one-step
    kernels take |u| from the relaxed populations exactly as av_velocity() does (SerialCode/d2q9-bgk.c:426-450): per-cell
    |u| is bit-identical, only the summation differs.  The resident and the multi-step stream kernels take it from the
    pre-collision moments with the native v_sqrt_f32 (BGK conserves density and momentum): their sum lies up to 4.3e-5
    from the relaxed one in the first steps of this run, where |u| ~ 1e-5, but within a few 2^-24 of the float64 sum of
    those moments' |u|."""
    import av_model
    monkeypatch.setenv("LBM_RESIDENT", resident)
    p, ob = datasets("128x256")
    steps = 40
    model = av_model.model(p.nx, p.ny, steps, reference=True)
    maps = model.moment if speed == "moment" else model.relaxed
    want = np.array([av_model.want_av(m, ob) for m in maps])
    with lbm.Engine(p, ob, oracle.init_cells(p)) as eng:
        info = eng.info()
        assert (info["resident_steps"] > 0) == (resident == "1") and info["steps_per_launch"] == 4
        eng.run(steps)
        got = eng.av_vels(steps).astype(np.float64)
        assert np.array_equal(eng.cells().view(np.uint32), model.cells.view(np.uint32))
    bound = av_model.bound(info, tile=0)         # 16x8 tiles (shape 0) on this grid, also for calls too short to run resident
    assert bound <= (1e-6 if resident == "0" else 1e-4)   # (13 + 2) 2^-24, + 2^-23 resident: stricter than what it replaces
    err = np.abs(got - want)
    print(f"av_ratio resummation LBM_RESIDENT={resident}: largest error / bound {np.max(err / (bound * want)):.3f}")
    assert np.all(err <= bound * want + av_model.FLUSH_ALLOWANCE), (err / want).tolist()


def test_all_blocked_and_no_blocked(lbm, oracle):
    p = lbm.Params(64, 16, 10, 10, 0.1, 0.005, 1.85)
    cells = oracle.init_cells(p)
    # no obstacles at all
    ob = np.zeros((16, 64), dtype=np.int32)
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 10)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)
    # everything but one cell blocked
    ob = np.ones((16, 64), dtype=np.int32)
    ob[14, 5] = 0
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 10)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    # ONE fluid cell whose momentum cancels to rounding noise every other step (|u| ~ 2e-8 next to populations of
    # 1e-2): the resident / stream kernels take |u| from the pre-collision moments, which differ from the relaxed
    # cell's by that noise -- an absolute 2e-8, meaningless as a ratio
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL, atol=1e-7)


def test_run_in_pieces_equals_one_run(lbm, oracle, datasets):
    """lbm_run(a) then lbm_run(b) must equal lbm_run(a+b): the fused next-step acceleration is
    dropped on the last step of a call and re-applied at the start of the next."""
    p, ob = datasets("128x128")
    cells = oracle.init_cells(p)
    with lbm.Engine(p, ob, cells) as one, lbm.Engine(p, ob, cells) as two:
        one.run(90)
        for n in (1, 2, 64, 23):
            two.run(n)
        assert np.array_equal(one.cells().view(np.uint32), two.cells().view(np.uint32))
        # av_vels: same cells, but the short calls run the LDS-tile kernel (|u| of the relaxed cell, av_velocity()'s own
        # arithmetic) and the long ones the resident kernel (|u| from the pre-collision moments, native sqrt): up to
        # 2.6e-5 apart in the first steps, where |u| ~ 1e-5 -- av_vels is tolerance-only
        np.testing.assert_allclose(one.av_vels(90), two.av_vels(90), rtol=5e-5, atol=0)


@pytest.mark.parametrize("slabs", [2, 3, 4, 8])
def test_exact_bitwise_multi_slab_one_device(lbm, oracle, datasets, slabs, monkeypatch):
    """Row slabs with packed halo rows exchanged between them (several slabs on one device):
    the decomposition, halo indices, boundary/interior split and lid-row placement."""
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob = datasets("128x256")
    cells = oracle.init_cells(p)
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 150, n_gpus=slabs)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)


def test_exact_bitwise_multi_slab_random(lbm, oracle, monkeypatch):
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells = random_case(lbm, 96, 23, 11, walls=False)   # uneven slabs: 23 rows over 4
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 40, n_gpus=4)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)


def test_rccl_self_exchange(lbm, oracle, datasets, monkeypatch):
    """One slab whose halo rows travel through RCCL send/recv to itself (periodic ring of 1):
    exercises the RCCL plumbing, streams and events on a 1-GPU box."""
    monkeypatch.setenv("LBM_FORCE_HALO", "1")
    monkeypatch.setenv("LBM_HALO", "rccl")
    p, ob = datasets("128x256")
    cells = oracle.init_cells(p)
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 60)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)


@pytest.mark.parametrize("band,lane_cells", [(2, 4), (5, 2), (8, 4), (8, 2), (64, 4), (3, 2)])
@pytest.mark.parametrize("slabs,halo", [(1, None), (1, "rccl"), (2, "memcpy"), (3, "memcpy"), (8, "memcpy")])
def test_two_steps_per_pass_kernel_bitwise(lbm, oracle, datasets, monkeypatch, band, lane_cells, slabs, halo):
    """The two-timesteps-per-pass kernel (step2_stream: register sliding window, DPP neighbours,
    2-row halos across slabs) is forced on at test sizes; odd step counts end with a one-step launch.
    Same per-cell arithmetic, so the lattice stays bit-identical to the oracle."""
    monkeypatch.setenv("LBM_FUSE2", "1")
    monkeypatch.setenv("LBM_BAND_ROWS", str(band))
    monkeypatch.setenv("LBM_LANE_CELLS", str(lane_cells))      # 4 or 2 cells per lane
    if halo:
        monkeypatch.setenv("LBM_HALO", halo)
        if slabs == 1:
            monkeypatch.setenv("LBM_FORCE_HALO", "1")
    p, ob = datasets("128x256")
    cells = oracle.init_cells(p)
    steps = 75                                        # odd: 37 two-step passes + 1 single step
    ref_cells, ref_av, got_cells, got_av, fields = run_both(lbm, oracle, p, ob, cells, steps, n_gpus=slabs)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)
    ref_f = oracle.final_state(p, ref_cells, ob)
    assert np.array_equal(ref_f["pressure"].view(np.uint32), fields["pressure"].view(np.uint32))


def test_two_step_runs_in_pieces_across_slabs(lbm, oracle, datasets, monkeypatch):
    """lbm_run in pieces of odd and even length with the two-step kernel on and three slabs
    (default halo transport for slabs that share a device): every piece starts with its own
    accelerate pass and halo exchange and may end with a one-step launch."""
    monkeypatch.setenv("LBM_FUSE2", "1")
    monkeypatch.delenv("LBM_HALO", raising=False)
    p, ob = datasets("128x256")
    cells = oracle.init_cells(p)
    ref = cells.copy()
    ref_av = oracle.run(p, ref, ob, 64)
    with lbm.Engine(p, ob, cells, n_gpus=3) as eng:
        for n in (1, 2, 3, 8, 5, 1, 44):
            eng.run(n)
        assert eng.info()["steps_done"] == 64
        assert np.array_equal(eng.cells().view(np.uint32), ref.view(np.uint32))
        np.testing.assert_allclose(eng.av_vels(64), ref_av, rtol=AV_RTOL)


def test_two_steps_per_pass_random_lattice(lbm, oracle, monkeypatch):
    """Random populations / obstacles, both periodic wraps live, lid row next to a slab edge."""
    monkeypatch.setenv("LBM_FUSE2", "1")
    monkeypatch.setenv("LBM_BAND_ROWS", "3")
    monkeypatch.setenv("LBM_HALO", "memcpy")
    for nx, ny, slabs in ((256, 24, 1), (512, 23, 4), (64, 40, 5), (1024, 9, 2)):
        monkeypatch.setenv("LBM_LANE_CELLS", "4" if ny % 2 else "2")
        p, ob, cells = random_case(lbm, nx, ny, 100 + ny, walls=False)
        ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 20, n_gpus=slabs)
        assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32)), (nx, ny, slabs)
        np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)


def test_randomised_configurations_bitwise(lbm, oracle, monkeypatch):
    """Seeded sweep over grid shapes, slab counts, band heights, kernels and step counts (random
    populations and obstacles, both wraps live): every configuration must reproduce the oracle's
    lattice bit for bit."""
    rng = np.random.default_rng(20260101)
    monkeypatch.setenv("LBM_HALO", "memcpy")
    checked = 0
    for case in range(60):
        nx = int(rng.choice([4, 8, 12, 64, 100, 128, 252, 256, 260, 512, 1000]))
        ny = int(rng.integers(8, 70))
        slabs = int(rng.choice([1, 1, 2, 3, 4, 5]))
        if ny // slabs < 4:
            slabs = 1
        fuse = int(rng.integers(0, 2))
        band = int(rng.choice([2, 3, 4, 7, 8, 16]))
        steps = int(rng.integers(1, 14))
        lane_cells = int(rng.choice([2, 4]))
        monkeypatch.setenv("LBM_FUSE2", str(fuse))
        monkeypatch.setenv("LBM_BAND_ROWS", str(band))
        monkeypatch.setenv("LBM_LANE_CELLS", str(lane_cells))
        p, ob, cells = random_case(lbm, nx, ny, 1000 + case, blocked_frac=float(rng.choice([0.0, 0.03, 0.3])),
                                   walls=bool(rng.integers(0, 2)))
        ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, steps, n_gpus=slabs)
        tag = dict(nx=nx, ny=ny, slabs=slabs, fuse=fuse, band=band, lane_cells=lane_cells, steps=steps)
        assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32)), tag
        np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL, atol=1e-12, err_msg=str(tag))
        checked += 1
    assert checked == 60
    # a few wider / taller ones: several strips per row, many bands per slab, uneven slabs
    for nx, ny, slabs, band, steps, lane_cells in ((4096, 131, 3, 8, 9, 4), (8192, 40, 2, 5, 6, 2),
                                                   (2048, 517, 4, 12, 5, 2), (1536, 260, 1, 23, 7, 4)):
        monkeypatch.setenv("LBM_FUSE2", "1")
        monkeypatch.setenv("LBM_BAND_ROWS", str(band))
        monkeypatch.setenv("LBM_LANE_CELLS", str(lane_cells))
        p, ob, cells = random_case(lbm, nx, ny, nx + ny, blocked_frac=0.02, walls=False)
        ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, steps, n_gpus=slabs)
        assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32)), (nx, ny, slabs, band)
        np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)


def test_rank_api_single_rank_rccl(lbm, oracle, datasets, monkeypatch):
    """lbm_create_rank with a world of one: ncclCommInitRank, halo send/recv to itself and the
    av_vels all-reduce all run through RCCL -- the code path every rank of a torchrun job takes."""
    monkeypatch.setenv("LBM_FORCE_HALO", "1")
    p, ob = datasets("128x256")
    cells = oracle.init_cells(p)
    ref = cells.copy()
    ref_av = oracle.run(p, ref, ob, 45)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, unique_id=lbm.rccl_unique_id(), device=0) as eng:
        info = eng.info()
        assert (info["world_rank"], info["world_size"], info["row_first"], info["row_count"]) == (0, 1, 0, p.ny)
        eng.run(45)
        assert np.array_equal(eng.cells().view(np.uint32), ref.view(np.uint32))
        np.testing.assert_allclose(eng.av_vels(45), ref_av, rtol=AV_RTOL)
        assert eng.av_velocity() == pytest.approx(float(ref_av[-1]), rel=AV_RTOL)


def test_fast_mode_within_check_tolerance(lbm, oracle, datasets):
    p, ob = datasets("128x128")
    cells = oracle.init_cells(p)
    steps = 2000
    ref_cells, ref_av, got_cells, got_av, fields = run_both(lbm, oracle, p, ob, cells, steps, math="fast")
    ref_f = oracle.final_state(p, ref_cells, ob)
    assert lbm.check_passes(ref_av, got_av, CHECK_TOL_PCT)
    assert lbm.check_passes(ref_f["pressure"], fields["pressure"], CHECK_TOL_PCT)
    # and it is close, not merely within 1 %
    np.testing.assert_allclose(got_av, ref_av, rtol=2e-4)


def test_diagnostics_match_oracle(lbm, oracle, datasets):
    """av_velocity / calc_reynolds / total_density (SerialCode/d2q9-bgk.c:409-458,637-660)."""
    p, ob = datasets("128x128")
    cells = oracle.init_cells(p)
    ref_cells = cells.copy()
    oracle.run(p, ref_cells, ob, 500)
    with lbm.Engine(p, ob, cells) as eng:
        mass0 = eng.total_density()
        eng.run(500)
        assert eng.av_velocity() == pytest.approx(oracle.av_velocity(p, ref_cells, ob), rel=AV_RTOL)
        assert eng.reynolds() == pytest.approx(oracle.calc_reynolds(p, ref_cells, ob), rel=AV_RTOL)
        # the device sums in double: compare with a float64 sum of the (bit-identical) lattice;
        # the oracle's sequential fp32 sum (total_density(), :644-660) carries ~1e-4 of rounding
        assert eng.total_density() == pytest.approx(float(ref_cells.astype(np.float64).sum()), rel=1e-9)
        assert eng.total_density() == pytest.approx(oracle.total_density(p, ref_cells), rel=1e-3)
        # mass conservation (the reference's DEBUG invariant, :175-179)
        assert eng.total_density() == pytest.approx(mass0, rel=1e-5)


def test_slab_thread_team(lbm, oracle, datasets, monkeypatch):
    """LBM_THREADS=1: one issuing host thread per slab (fork-join per phase).  Same results."""
    monkeypatch.setenv("LBM_THREADS", "1")
    monkeypatch.setenv("LBM_HALO", "memcpy")
    monkeypatch.setenv("LBM_FUSE2", "1")
    p, ob = datasets("128x256")
    cells = oracle.init_cells(p)
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 101, n_gpus=4)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)
    monkeypatch.setenv("LBM_FUSE2", "0")
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 50, n_gpus=3)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))


def test_run_to_run_determinism(lbm, datasets, monkeypatch):
    """No atomics anywhere: per-workgroup partials reduced in a fixed order, so two runs of the same
    configuration give bit-identical av_vels (and lattices) -- with one slab, several slabs, and
    the two-step kernel."""
    p, ob = datasets("256x256")
    for fuse, slabs in (("0", 1), ("1", 1), ("1", 3)):
        monkeypatch.setenv("LBM_FUSE2", fuse)
        monkeypatch.setenv("LBM_HALO", "memcpy")
        outs = []
        for _ in range(2):
            with lbm.Engine(p, ob, None, n_gpus=slabs) as eng:
                eng.run(301)
                outs.append((eng.av_vels(301).copy(), eng.cells().copy()))
        assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)), (fuse, slabs)
        assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32)), (fuse, slabs)


def test_api_misuse_returns_errors(lbm, datasets):
    """Error behaviour of the C ABI in return-code mode (the Python host's mode): every misuse is
    reported with a message, nothing crashes, and the context stays usable."""
    import ctypes
    p, ob = datasets("128x128")
    small = lbm.Params(p.nx, p.ny, 10, p.reynolds_dim, p.density, p.accel, p.omega)
    with lbm.Engine(small, ob) as eng:
        eng.run(4)
        with pytest.raises(lbm.LbmError, match="steps requested"):
            eng.av_vels(5)                      # only 4 recorded
        with pytest.raises(lbm.LbmError, match="negative"):
            eng.run(-1)
        eng.run(0)                              # no-op
        lib = eng.lib
        assert lib.lbm_read_av_vels(eng.handle, None, 1) != 0 and b"NULL" in lib.lbm_last_error()
        assert lib.lbm_read_cells(eng.handle, None) != 0
        assert lib.lbm_run(None, 1) != 0 and b"null context" in lib.lbm_last_error()
        assert lib.lbm_get_info(eng.handle, None) != 0
        eng.run(6)                              # still works, fills the record exactly
        assert eng.info()["steps_done"] == 10 and np.isfinite(eng.av_vels(10)).all()
    bad_math = 7
    with pytest.raises(lbm.LbmError, match="math mode"):
        h = lbm.load_library().lbm_create(ctypes.byref(small._c()), ob.ctypes.data, None, 1, bad_math)
        if not h:
            raise lbm.LbmError(lbm.load_library().lbm_last_error().decode())


def test_run_beyond_record_fails(lbm, datasets):
    p, ob = datasets("128x128")
    small = lbm.Params(p.nx, p.ny, 5, p.reynolds_dim, p.density, p.accel, p.omega)
    with lbm.Engine(small, ob) as eng:
        eng.run(5)
        with pytest.raises(lbm.LbmError):
            eng.run(1)


@pytest.mark.parametrize("knob,value", [("LBM_NEIGH", "1"), ("LBM_NEIGH", "2"), ("LBM_SNAKE", "1"),
                                        ("LBM_PLANE_PAD_FLOATS", "16"), ("LBM_NTS", "1"), ("LBM_NTS", "0"),
                                        ("LBM_VEC4", "0"), ("LBM_VEC4", "1")])
@pytest.mark.parametrize("fuse", ["0", "1"])
def test_tuning_knobs_do_not_change_results(lbm, oracle, monkeypatch, knob, value, fuse):
    """Every environment knob of DESIGN.md section 6a selects a different kernel flavour or layout, never a
    different result: each one bit-exact against the oracle, single slab and across 3 slabs."""
    monkeypatch.setenv("LBM_FUSE2", fuse)
    monkeypatch.setenv("LBM_HALO", "memcpy")
    monkeypatch.setenv(knob, value)
    p, ob, cells = random_case(lbm, 320, 29, 41)
    for slabs in (1, 3):
        ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 13, n_gpus=slabs)
        assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32)), (knob, value, slabs)
        np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_graph_replay_is_bit_exact(lbm, oracle, monkeypatch, fuse):
    """LBM_GRAPH=1: chunks of 64 timesteps + their reduce replayed as one hipGraph each (single slab);
    several lbm_run calls with lengths around the chunk size, odd totals, both lattice parities."""
    monkeypatch.setenv("LBM_GRAPH", "1")
    monkeypatch.setenv("LBM_FUSE2", fuse)
    p, ob, cells = random_case(lbm, 192, 40, 77)
    calls = [130, 1, 64, 65, 7, 129, 4]           # 400 steps
    ref = cells.copy()
    ref_av = oracle.run(p, ref, ob, sum(calls))
    with lbm.Engine(p, ob, cells) as eng:
        for n in calls:
            eng.run(n)
        got = eng.cells()
        got_av = eng.av_vels(sum(calls))
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)


@pytest.mark.parametrize("nx,ny", [(128, 128), (96, 40), (33, 19), (257, 9), (20, 6), (64, 8)])
@pytest.mark.parametrize("tile_steps", ["4", "3", "1", "8", "6"])
def test_lds_tile_kernel_bitwise(lbm, oracle, monkeypatch, nx, ny, tile_steps):
    """step_tile: several timesteps per launch from LDS tiles (16x8 own cells + a halo of 4 or 8 cells,
    periodic images staged where the halo leaves the grid -- also when the grid is smaller than one staged
    tile).
    Ragged tile edges, step counts that are not multiples of the launch depth, run in pieces, graph
    replay on and off: lattice bit-identical to the oracle."""
    monkeypatch.setenv("LBM_TILE_STEPS", tile_steps)
    if tile_steps == "3":
        monkeypatch.setenv("LBM_TILE_SHAPE", "3")              # 32x16 own cells, halo of 3 (mid-size default)
    p, ob, cells = random_case(lbm, nx, ny, nx + ny)
    for graph in ("0", "1"):
        monkeypatch.setenv("LBM_GRAPH", graph)
        calls = [1, 70, 6, 133]
        ref = cells.copy()
        ref_av = oracle.run(p, ref, ob, sum(calls))
        with lbm.Engine(p, ob, cells) as eng:
            assert eng.info()["steps_per_launch"] == int(tile_steps)
            for n in calls:
                eng.run(n)
            got = eng.cells()
            got_av = eng.av_vels(sum(calls))
            fields = eng.final_state()
        assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
        np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)
        want = oracle.final_state(p, ref, ob)
        assert np.array_equal(fields["pressure"].view(np.uint32), want["pressure"].view(np.uint32))


@pytest.mark.parametrize("shape,steps", [("2", "2"), ("4", "4"), ("5", "2"), ("6", "1")])
def test_lds_tile_shapes_bitwise(lbm, oracle, monkeypatch, shape, steps):
    """The other step_tile instantiations (LBM_TILE_SHAPE) on a grid whose edges cut through tiles."""
    monkeypatch.setenv("LBM_TILE_SHAPE", shape)
    monkeypatch.setenv("LBM_TILE_STEPS", steps)
    p, ob, cells = random_case(lbm, 200, 51, 9)
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 37)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)


def test_default_kernel_by_grid_size(lbm, datasets):
    """The policy of DESIGN.md section 6: LDS tiles below 300 Ki cells, three steps per pass on one pair of cells per
    lane from there, four steps per pass on two pairs per lane from 3.5 Mi cells."""
    for n, want in ((128, 4), (448, 4), (512, 3), (576, 3), (768, 3), (1024, 3), (1792, 3), (1920, 4), (2048, 4)):
        p = lbm.Params(n, n, 4, 10, 0.1, 0.005, 1.85)
        ob = np.zeros((n, n), dtype=np.int32)
        with lbm.Engine(p, ob, None) as eng:
            assert eng.info()["steps_per_launch"] == want, n


@pytest.mark.parametrize("nx,ny", [(1, 2), (2, 2), (3, 3), (5, 2), (4, 2), (8, 3), (4, 5), (12, 4)])
@pytest.mark.parametrize("kernel", ["default", "one-step", "two-step"])
def test_degenerate_grid_sizes_bitwise(lbm, oracle, monkeypatch, nx, ny, kernel):
    """The smallest grids the parameter check admits (ny >= 2, nx >= 1): every neighbour is a periodic
    image of the cell itself or of the one other row; each kernel family must still follow the oracle."""
    if kernel != "default":
        monkeypatch.setenv("LBM_FUSE2", "1" if kernel == "two-step" else "0")
    p, ob, cells = random_case(lbm, nx, ny, 100 + nx * ny, blocked_frac=0.0, walls=False)
    ob[:] = 0
    if nx * ny > 4:
        ob[0, 0] = 1
    ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, 9)
    assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)


PADDED_STEPS, PADDED_EVERY = 7, 2
PADDED_PROBES = ((45, 4), (129, 8), (0, 0), (64, 7))   # inside the obstacle block; last column of the top row; ...


@functools.lru_cache(maxsize=None)
def padded_reference(lbm, oracle):
    """The 130 x 9 case of test_readers_and_recorders_with_padded_planes and what the oracle makes of it, computed once:
    the final_state after each of the first PADDED_STEPS steps, and the mean sums of both orders."""
    p, ob, cells = random_case(lbm, 130, 9, 130, walls=False)
    ob[3:6, 40:50] = 1
    ref, states = cells.copy(), {}
    for t in range(1, PADDED_STEPS + 1):
        oracle.run(p, ref, ob, 1)
        states[t] = oracle.final_state(p, ref, ob)
    _, sums, sums2, n = moments_model.oracle_sums2(oracle, p, ob, cells, 0, PADDED_STEPS, PADDED_EVERY)
    return p, ob, cells, ref, states, sums, sums2, n


@pytest.mark.parametrize("slabs", [1, 3])
def test_readers_and_recorders_with_padded_planes(lbm, oracle, monkeypatch, slabs):
    """plane_stride (208) != mask pitch (192) != nx (130), the one layout in which a stride taken for another reads the
    wrong plane or row: every reader of a stored lattice and every per-pass record kernel, bit for bit against the
    oracle, on one slab and across three."""
    monkeypatch.setenv("LBM_PLANE_PAD_FLOATS", "16")
    monkeypatch.setenv("LBM_HALO", "memcpy")
    p, ob, cells, ref, states, sums, sums2, n_samples = padded_reference(lbm, oracle)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)
    sample_steps = frames_model.frame_steps(0, PADDED_STEPS, PADDED_EVERY)
    assert ob[PADDED_PROBES[0][1], PADDED_PROBES[0][0]] == 1 and n_samples == len(sample_steps) == 4

    with lbm.Engine(p, ob, cells, n_gpus=slabs) as eng:                      # the readers
        assert eng.info()["resident_steps"] == 0                               # 130 columns: the per-pass path
        eng.run(PADDED_STEPS)
        assert np.array_equal(bits(eng.cells()), bits(ref))
        fields = eng.final_state()
        for k in ("u_x", "u_y", "u", "pressure"):
            assert np.array_equal(bits(fields[k]), bits(states[PADDED_STEPS][k])), k
        assert eng.av_velocity() == pytest.approx(oracle.av_velocity(p, ref, ob), rel=AV_RTOL)
        # the device adds the cells' fp32 densities (the nine populations summed in index order, as total_density()
        # and av_velocity() form them) in double.  On 1170 random cells the fp32 rounding of each density does not
        # average out of the total the way it does on a reference data set (1.1e-9 relative against a float64 sum of
        # the populations), so the float64 sum is taken over those same fp32 densities
        rho = ref[..., 0].copy()
        for k in range(1, 9):
            rho = rho + ref[..., k]
        assert rho.dtype == np.float32
        assert eng.total_density() == pytest.approx(float(rho.astype(np.float64).sum()), rel=1e-9)
        assert eng.total_density() == pytest.approx(oracle.total_density(p, ref), rel=1e-3)

    with lbm.Engine(p, ob, cells, n_gpus=slabs) as eng:                      # frames
        eng.set_frames(PADDED_EVERY, 8)
        eng.run(PADDED_STEPS)
        steps, frames = eng.frames()
        assert steps.tolist() == sample_steps
        for i, tt in enumerate(sample_steps):
            assert np.array_equal(bits(frames[i]), bits(states[tt + 1]["u"])), tt

    xs, ys = np.array([c[0] for c in PADDED_PROBES]), np.array([c[1] for c in PADDED_PROBES])
    with lbm.Engine(p, ob, cells, n_gpus=slabs) as eng:                      # probes
        eng.set_probes(PADDED_PROBES, PADDED_EVERY, 8)
        eng.run(PADDED_STEPS)
        steps, samples = eng.probes()
        assert steps.tolist() == sample_steps
        for i, tt in enumerate(sample_steps):
            want = np.stack([states[tt + 1][k][ys, xs] for k in ("u_x", "u_y", "u", "pressure")], axis=1)
            assert np.array_equal(bits(samples[i]), bits(want)), tt

    with lbm.Engine(p, ob, cells, n_gpus=slabs) as eng:                      # mean fields, both orders
        eng.set_mean_order(PADDED_EVERY, 2)
        eng.run(PADDED_STEPS)
        got, n = eng.mean_sums()
        got2, n2 = eng.moment_sums()
        assert n == n2 == n_samples
        for k in sums:
            assert np.array_equal(bits(got[k]), bits(sums[k])), k
        for k in sums2:
            assert np.array_equal(bits(got2[k]), bits(sums2[k])), k
