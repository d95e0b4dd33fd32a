"""Batches (lbm_create_batch / lbm.Batch): B independent lattices of one shape advanced together, on resident shapes as
launches of the batched resident kernel (8 one-XCD members per launch, else as many as have a CU per workgroup).  Every
member is bit-identical to the oracle and to a single Engine run on the same inputs and call sequence."""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_parity import AV_RTOL, random_case

pytestmark = pytest.mark.gpu


def sweep_128(lbm, datasets):
    """Eight 128^2 members: omega 1.5-1.9, accel 0.005-0.02, two densities; the reference map, its mirror, 10 %
    random blocked cells and no obstacles."""
    p0, ob0 = datasets("128x128")
    rng = np.random.default_rng(11)
    maps = [ob0, np.ascontiguousarray(ob0[:, ::-1]), (rng.random(ob0.shape) < 0.1).astype(np.int32),
            np.zeros_like(ob0)]
    params, obstacles = [], []
    for i in range(8):
        params.append(lbm.Params(p0.nx, p0.ny, p0.max_iters, p0.reynolds_dim, (0.1, 0.12)[i % 2],
                                 float(np.float32(0.005 + 0.015 * i / 7)), float(np.float32(1.5 + 0.4 * i / 7))))
        obstacles.append(maps[i % 4])
    return params, obstacles


def random_members(lbm, nx, ny, n, seed, max_iters=400):
    params, obstacles, cells = [], [], []
    for i in range(n):
        p, ob, c = random_case(lbm, nx, ny, seed + i)
        p = lbm.Params(nx, ny, max_iters, p.reynolds_dim, p.density, float(np.float32(0.004 + 0.001 * (i % 5))),
                       float(np.float32(1.6 + 0.02 * (i % 13))))
        params.append(p)
        obstacles.append(ob)
        cells.append(c)
    return params, obstacles, cells


def assert_members_match_oracle(lbm, oracle, batch, params, obstacles, cells, steps):
    for i, (p, ob) in enumerate(zip(params, obstacles)):
        ref = oracle.init_cells(p) if cells is None else cells[i].copy()
        ref_av = oracle.run(p, ref, ob, steps)
        m = batch.member(i)
        got = m.cells()
        assert np.array_equal(ref.view(np.uint32), got.view(np.uint32)), f"member {i}: lattice differs from the oracle"
        np.testing.assert_allclose(m.av_vels(steps), ref_av, rtol=AV_RTOL, err_msg=f"member {i}")
        want = oracle.final_state(p, ref, ob)
        assert np.array_equal(m.final_state()["pressure"].view(np.uint32), want["pressure"].view(np.uint32)), i
        yield i, p, ob, ref, m


def test_eight_member_sweep_128_bitwise(lbm, oracle, datasets):
    params, obstacles = sweep_128(lbm, datasets)
    calls = [37, 5, 300]       # 5 < resident_min_steps: that call takes the per-pass path member by member
    with lbm.Batch(params, obstacles) as batch:
        info = batch.info()
        assert info["members"] == 8 and info["members_per_launch"] == 8 and info["launches_per_chunk"] == 1, info
        assert info["resident_steps"] > 0 and 5 < info["resident_min_steps"] <= 37, info
        for n in calls:
            batch.run(n)
        batch.sync()
        assert batch.info()["steps_done"] == sum(calls)
        for i, p, ob, ref, m in assert_members_match_oracle(lbm, oracle, batch, params, obstacles, None, sum(calls)):
            assert m.reynolds() == pytest.approx(oracle.calc_reynolds(p, ref, ob), rel=AV_RTOL)
            assert m.av_velocity() == pytest.approx(oracle.av_velocity(p, ref, ob), rel=AV_RTOL)
            # the device sums each cell's fp32 density in double, the oracle in sequential fp32
            assert m.total_density() == pytest.approx(float(ref.astype(np.float64).sum()), rel=1e-7)
            assert m.info()["steps_done"] == sum(calls)


@pytest.mark.parametrize("nx,ny", [(64, 64), (128, 128)])
@pytest.mark.parametrize("n_members", [1, 3, 9, 17])
def test_members_equal_single_engines(lbm, nx, ny, n_members):
    """No cross-talk between members, no sub-batch mistakes: every member equals its own Engine, bit for bit."""
    params, obstacles, cells = random_members(lbm, nx, ny, n_members, seed=100 * n_members + nx)
    calls = [40, 3, 25]
    with lbm.Batch(params, np.stack(obstacles), np.stack(cells)) as batch:
        info = batch.info()
        assert info["members_per_launch"] == 8, info
        assert info["launches_per_chunk"] == -(-n_members // 8), info
        for n in calls:
            batch.run(n)
        for i in range(n_members):
            with lbm.Engine(params[i], obstacles[i], cells[i]) as eng:
                for n in calls:
                    eng.run(n)
                want, want_av = eng.cells(), eng.av_vels()
            m = batch.member(i)
            assert np.array_equal(m.cells().view(np.uint32), want.view(np.uint32)), f"member {i} of {n_members}"
            assert np.array_equal(m.av_vels().view(np.uint32), want_av.view(np.uint32)), f"member {i} of {n_members}"


@pytest.mark.parametrize("n_members,nx,ny,steps,per_launch", [(2, 256, 256, 50, 2), (3, 128, 256, 50, 2),
                                                              (8, 1024, 64, 50, 8), (2, 1024, 1024, 24, 1)])
def test_multi_xcd_shapes_bitwise(lbm, oracle, n_members, nx, ny, steps, per_launch):
    params, obstacles, cells = random_members(lbm, nx, ny, n_members, seed=7 * nx + ny)
    with lbm.Batch(params, obstacles, cells) as batch:
        info = batch.info()
        assert info["members_per_launch"] == per_launch, info
        assert info["launches_per_chunk"] == -(-n_members // per_launch), info
        batch.run(steps)
        for _ in assert_members_match_oracle(lbm, oracle, batch, params, obstacles, cells, steps):
            pass


def test_long_call_crosses_chunks(lbm):
    """9 000 steps in one call: three chunks of the resident kernel, the tags of each member run on across them."""
    params, obstacles, cells = random_members(lbm, 64, 64, 8, seed=900, max_iters=9000)
    with lbm.Batch(params, obstacles, cells) as batch:
        assert batch.info()["resident_steps"] < 9000
        batch.run(9000)
        for i in range(8):
            with lbm.Engine(params[i], obstacles[i], cells[i]) as eng:
                eng.run(9000)
                want, want_av = eng.cells(), eng.av_vels()
            m = batch.member(i)
            assert np.array_equal(m.cells().view(np.uint32), want.view(np.uint32)), f"member {i}"
            assert np.array_equal(m.av_vels().view(np.uint32), want_av.view(np.uint32)), f"member {i}"


@pytest.mark.parametrize("nx,ny", [(100, 40), (2048, 64)])
def test_fallback_shapes_bitwise(lbm, oracle, nx, ny):
    params, obstacles, cells = random_members(lbm, nx, ny, 3, seed=nx + ny)
    with lbm.Batch(params, obstacles, cells) as batch:
        info = batch.info()
        assert info["resident_steps"] == 0, info
        batch.run(12)
        batch.run(9)
        for _ in assert_members_match_oracle(lbm, oracle, batch, params, obstacles, cells, 21):
            pass


def test_eight_reference_runs_match_serialcode(lbm, datasets, tmp_path):
    """8 copies of the reference's 128x128 data set, all 40 000 steps in one call: every member's final_state.dat has
    the bytes the reference's SerialCode wrote."""
    p, ob = datasets("128x128")
    ref = np.load(os.path.join(GOLDEN, "serialcode_128x128.npz"))
    with lbm.Batch([p] * 8, [ob] * 8) as batch:
        batch.run(p.max_iters)
        batch.sync()
        for i in range(8):
            m = batch.member(i)
            path = tmp_path / f"final_state_{i}.dat"
            lbm.write_final_state(str(path), m.final_state(), ob)
            assert hashlib.md5(path.read_bytes()).hexdigest() == str(ref["md5_final_state"]), f"member {i}"
            np.testing.assert_allclose(m.av_vels(), ref["av_vels"], rtol=AV_RTOL, err_msg=f"member {i}")


def test_member_handles_are_read_only_views(lbm, datasets):
    p, ob = datasets("128x128")
    batch = lbm.Batch([p, p], [ob, ob])
    m = batch.member(1)
    with pytest.raises(lbm.LbmError, match="member of a batch"):
        m.run(10)
    with pytest.raises(lbm.LbmError, match="member of a batch"):
        m.run_timed(10)
    m.close()                  # does nothing: the batch owns its members
    batch.run(20)
    assert m.info()["steps_done"] == 20
    assert m.av_vels().shape == (20,)
    with pytest.raises(lbm.LbmError):
        batch.member(2)
    batch.close()
    with pytest.raises(lbm.LbmError, match="closed"):
        m.cells()


def test_give_up_is_reported_by_every_member(lbm, datasets, monkeypatch):
    """A batched launch whose workgroups are not all running gives up after the bound; the next sync of each member
    reports it (the tests' absent-band knob: one band of every member never starts)."""
    monkeypatch.setenv("LBM_RESIDENT_ABSENT_BAND", "5")
    monkeypatch.setenv("LBM_RESIDENT_TIMEOUT_MS", "200")
    p, ob = datasets("128x128")
    with lbm.Batch([p] * 3, [ob] * 3) as batch:
        batch.run(100)
        for i in range(3):
            with pytest.raises(lbm.LbmError, match="resident kernel gave up"):
                batch.member(i).sync()
