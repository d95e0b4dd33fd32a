"""The double engine (lbm_double_*) where tests/test_gpu_double.py never takes it: the refused lid acceleration in every
kernel that accelerates, cells far from equilibrium (denormals, 2^1000, negative and zero density, infinite and NaN
results, a stored cell of -0.0), more than 256 workgroups and more than 65 536 cells (the second trips of reduce_partials_d and
lattice_sums_d), the ring of per-step partials across calls, and lattices that are staged in several chunks.  The
inputs are tests/double_edge_lattice.py; tests/test_double_edge_lattice.py shows, by the model alone, that they reach
what they aim at.

The rule of every comparison.  Fields are compared with tests/double_model.py as uint64 bit patterns: every finite value,
every infinity and the sign of every zero must match bit for bit; a NaN in the model must be a NaN in the engine, with any
sign and payload, and the other way round (`assert_same`).  av_vels[t] is a sum of n = fluid cells non-negative terms that the
kernels add in another order than the model: wherever the model's value is finite it must be within 2 (n - 1) 2^-53
relative (the bound of test_gpu_double.py); where it is not, the engine's value is non-finite of the same class
(`assert_av`).  No tolerance here is measured."""
import numpy as np
import pytest

import double_edge_lattice as dl
import double_model

pytestmark = pytest.mark.gpu

DENSITY, ACCEL, OMEGA = dl.DENSITY, dl.ACCEL, dl.OMEGA
FIELDS = ("u_x", "u_y", "pressure", "u")
K_BLOCK = 256                                 # lanes of a workgroup (lbm::kBlock), partials one reduce lane adds per trip


def sum_order_bound(n_fluid):
    return 2.0 * (n_fluid - 1) * 2.0 ** -53


def assert_same(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        bad = np.argwhere(~ok)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} values differ from the float64 model, the first at {first}: "
                             f"{got[first]!r} ({got.view(np.uint64)[first]:#018x}), model {want[first]!r} "
                             f"({want.view(np.uint64)[first]:#018x})")


def assert_av(got, want, n_fluid, what):
    """Returns the largest relative difference among the finite values (0.0 if there is none)."""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN where the model has none, or none where it has"
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), f"{what}: infinities differ"
    assert np.isfinite(got[fin]).all(), what
    worst = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0
    assert worst <= sum_order_bound(n_fluid), f"{what}: av_vels differ by {worst:.3e} relative, bound {sum_order_bound(n_fluid):.3e}"
    return worst


def nts_cases(shapes):
    """(nx, ny, nts): both store flavours where a row is made of pairs; the one-cell kernel has one."""
    return [(nx, ny, nts) for nx, ny in shapes for nts in ((0, 1) if nx % 2 == 0 else (0,))]


def engine(lbm, monkeypatch, nx, ny, nts, max_iters, ob, start):
    monkeypatch.setenv("LBM_DOUBLE_NTS", str(nts))
    eng = lbm.DoubleEngine(lbm.ParamsDouble(nx, ny, max_iters, 10, DENSITY, ACCEL, OMEGA), ob, start)
    info = eng.info()
    assert info["lane_cells"] == (2 if nx % 2 == 0 else 1) and info["nontemporal"] == (nts if nx % 2 == 0 else 0), info
    assert info["fluid_cells"] == int((np.asarray(ob) == 0).sum())
    return eng


def workgroups(nx, ny, lane_cells):
    """Workgroups of one step launch, as lbm_double_create sizes it."""
    return -(-(nx * ny // lane_cells) // K_BLOCK)


# ---- the refused acceleration ------------------------------------------------------------------------------------
# 130 x 12: step_double, the wave edge at pair 64, the ramp's period inside the row; 131 x 12: step_double_scalar.
# [13]: step 0 through accelerate_row_d, steps 1 .. 12 through the epilogue of relax_cell_d; [1] * 13: every step
# through accelerate_row_d; [1, 5, 7]: both, with the pre-pass meeting a lattice that has run.
@pytest.mark.parametrize("calls", [[13], [1] * 13, [1, 5, 7]], ids=["one call", "13 calls", "1+5+7"])
@pytest.mark.parametrize("nx,ny,nts", nts_cases(dl.REFUSAL_SHAPES))
def test_refusal_in_every_kernel_that_accelerates(lbm, monkeypatch, nx, ny, nts, calls):
    run = dl.refusal_run(nx, ny)
    if calls == [13]:
        for t, c in enumerate(run["counts"]):
            print(f"{nx}x{ny} lid row before step {t}, by the model: {c}")
    n = int((run["ob"] == 0).sum())
    with engine(lbm, monkeypatch, nx, ny, nts, dl.STEPS, run["ob"], run["start"]) as eng:
        done = 0
        for k in calls:
            eng.run(k)
            done += k
            assert eng.info()["steps_done"] == done
            assert_same(eng.cells(), run["states"][done - 1], f"{nx}x{ny} nts={nts} calls {calls}, after step {done}")
        worst = assert_av(eng.av_vels(), run["av"], n, f"{nx}x{ny} nts={nts} calls {calls}")
        final = eng.final_state()
    want = double_model.final_state(run["states"][-1], run["ob"], DENSITY)
    for name in FIELDS:
        assert_same(final[name], want[name], name)
    print(f"{nx}x{ny} nts={nts} calls {calls}: av_vels max relative difference {worst:.3e} (bound {sum_order_bound(n):.3e})")


# ---- cells far from equilibrium ----------------------------------------------------------------------------------
# 130 x 6: step_double; 7 x 5: step_double_scalar.  1 step: the placed cells' own collision; 2 and 4: what they relax to
# meets arithmetic again (after 4 steps the 7 x 5 lattice holds nothing but NaN, after 2 it still holds numbers).
@pytest.mark.parametrize("steps", [1, 2, 4])
@pytest.mark.parametrize("nx,ny,nts", nts_cases(dl.EXTREME_SHAPES))
def test_extreme_cells(lbm, monkeypatch, nx, ny, nts, steps):
    run = dl.extreme_run(nx, ny)
    want = run["after"][steps]
    n = int((run["ob"] == 0).sum())
    with engine(lbm, monkeypatch, nx, ny, nts, steps, run["ob"], run["start"]) as eng:
        assert_same(eng.cells(), run["start"], "upload and read back")     # denormals, 2^1000 and zeros through the staging
        eng.run(steps)
        got, final, av = eng.cells(), eng.final_state(), eng.av_vels()
    assert_same(got, want["cells"], f"{nx}x{ny} nts={nts}, lattice after {steps} steps")
    for name in FIELDS:
        assert_same(final[name], want["final"][name], f"{nx}x{ny} nts={nts}, {name} after {steps} steps")
    assert_av(av, run["av"][:steps], n, f"{nx}x{ny} nts={nts}, {steps} steps")
    nans = int(np.isnan(got).any(axis=2).sum())
    print(f"{nx}x{ny} nts={nts}, {steps} steps: {nans} of {nx * ny} cells hold a NaN, as in the model; av_vels {av}")


@pytest.mark.parametrize("nx,ny", [(8, 3), (7, 5)])
def test_stored_cell_of_negative_zeros(lbm, monkeypatch, nx, ny):
    """A stored fluid cell whose nine populations are -0.0, and one of +0.0, read without a step: the reference's density
    starts from 0.f (SerialCode/d2q9-bgk.c:692 as :325), so it is +0.0 for both and so is the pressure; u is 0/0."""
    ob, start = dl.build_signed_zeros(nx, ny)
    want = double_model.final_state(start, ob, DENSITY)
    with engine(lbm, monkeypatch, nx, ny, 0, 1, ob, start) as eng:
        assert_same(eng.cells(), start, "upload and read back")
        final, mass = eng.final_state(), eng.total_density()
    for name in FIELDS:
        assert_same(final[name], want[name], name)
    total = float(start.sum())
    assert abs(mass - total) / total <= sum_order_bound(9 * nx * ny)


# ---- random lattices, the model's run kept at chosen steps ---------------------------------------------------------
def random_case(nx, ny, keep, seed=None):
    """The lattice of test_gpu_double.case (0.5 .. 1.5 x equilibrium, 15 % obstacles, blocked cells on the lid row) and
    the model's lattice after each step count in `keep`, with av_vels up to the last of them."""
    rng = np.random.default_rng(1000 * nx + ny if seed is None else seed)
    ob = (rng.random((ny, nx)) < 0.15).astype(np.int32)
    lid = ny - 2
    ob[lid, :] = 0
    ob[lid, rng.choice(nx, size=max(1, nx // 8), replace=False)] = 1
    ob[lid, 0], ob[lid, nx - 1] = 0, 1
    start = double_model.init_cells(nx, ny, DENSITY) * (0.5 + rng.random((ny, nx, 9)))
    cells, states, av = start.copy(), {}, []
    for t in range(1, max(keep) + 1 if keep else 1):
        double_model.timestep(cells, ob, DENSITY, ACCEL, OMEGA)
        av.append(double_model.av_velocity(cells, ob))
        if t in keep:
            states[t] = cells.copy()
    av = np.array(av)
    for a in (ob, start, av, *states.values()):
        a.setflags(write=False)
    return {"ob": ob, "start": start, "states": states, "av": av, "n": int((ob == 0).sum())}


# ---- more than 256 workgroups, more than 65 536 cells --------------------------------------------------------------
# reduce_partials_d: lane i adds partials i, i + 256, ...: at 260 (259) workgroups the loop's second trip takes the last
# 4 (3).  A reducer that stopped after the first trip would lose 4 of 260 workgroups' |u|, about 1.5 % of av_vels -- the
# bound is 1.4e-11.  lattice_sums_d strides 256 x 256 lanes over the cells: a third trip here.
_big = {}


@pytest.mark.parametrize("nx,ny,nts", nts_cases([(1024, 130), (513, 129)]))
def test_more_than_256_workgroups(lbm, monkeypatch, nx, ny, nts):
    steps = 3
    if (nx, ny) not in _big:                  # once per shape, never changed
        _big[(nx, ny)] = random_case(nx, ny, {steps})
    case = _big[(nx, ny)]
    n = case["n"]
    with engine(lbm, monkeypatch, nx, ny, nts, steps, case["ob"], case["start"]) as eng:
        groups = workgroups(nx, ny, eng.info()["lane_cells"])
        assert groups == (260 if nx % 2 == 0 else 259) and groups > K_BLOCK
        assert nx * ny > 256 * K_BLOCK                                     # lattice_sums_d: 256 workgroups of 256 lanes
        eng.run(steps)
        got, av = eng.cells(), eng.av_vels()
        av_now, mass, reynolds = eng.av_velocity(), eng.total_density(), eng.reynolds()
    want = case["states"][steps]
    assert_same(got, want, f"{nx}x{ny} nts={nts}, lattice after {steps} steps")
    worst = assert_av(av, case["av"], n, f"{nx}x{ny} nts={nts}")
    print(f"{nx}x{ny} nts={nts}: {groups} workgroups, av_vels max relative difference {worst:.3e} (bound {sum_order_bound(n):.3e})")
    assert abs(av_now - case["av"][-1]) / case["av"][-1] <= sum_order_bound(n)
    total = float(want.sum())
    assert abs(mass - total) / total <= sum_order_bound(9 * nx * ny)
    assert reynolds == av_now * 10 / (1.0 / 6.0 * (2.0 / OMEGA - 1.0))


# ---- the ring of partials across calls ---------------------------------------------------------------------------
# 64 slots.  run(5): no wrap; run(70) from step 5: a full ring reduced into tot_u[5 .. 69), then 6 more; run(64) from
# step 75: exactly one ring, reduced at its last slot; run(1).  tot_u's index is steps_done + t - slot.
@pytest.mark.parametrize("nts", [0, 1])
def test_partial_ring_across_calls(lbm, monkeypatch, nts):
    nx, ny, calls = 130, 6, (5, 70, 64, 1)
    total = sum(calls)
    case = ring_case()
    with engine(lbm, monkeypatch, nx, ny, nts, total, case["ob"], case["start"]) as eng:
        done = 0
        for k in calls:
            eng.run(k)
            done += k
            assert_same(eng.cells(), case["states"][done], f"nts={nts}, lattice after {done} steps")
        av = eng.av_vels()
        with pytest.raises(lbm.LbmError, match=f"av_vels record holds {total}"):
            eng.run(1)
    worst = assert_av(av, case["av"], case["n"], f"nts={nts}, calls {calls}")
    print(f"130x6 nts={nts} calls {calls}: av_vels max relative difference {worst:.3e} (bound {sum_order_bound(case['n']):.3e})")
    with engine(lbm, monkeypatch, nx, ny, nts, total, case["ob"], case["start"]) as eng:
        eng.run(total)
        whole = eng.av_vels()
    assert np.array_equal(av.view(np.uint64), whole.view(np.uint64)), "av_vels of the calls differ from one call's"


_ring = {}


def ring_case():
    if not _ring:
        _ring.update(random_case(130, 6, {5, 75, 139, 140}))
        assert np.isfinite(_ring["av"]).all() and (_ring["av"] > 0).all() and len(_ring["av"]) == 140
    return _ring


# ---- staging seams ---------------------------------------------------------------------------------------------------
# Upload and lbm_double_read_cells move 64 MiB / (72 nx) rows at a time, lbm_double_read_final_state 16 MiB / (8 nx):
# the chunk sizes fix the cell count at which both loops iterate, and 16384 x 130 is the smallest such shape with ragged
# last chunks (56 + 56 + 18 rows, 128 + 2 rows).  Zero steps: what is checked is the staging, the host cost is array
# comparisons.  (No step kernel runs, so the store flavour cannot show; both are run as everywhere.)
@pytest.mark.parametrize("nts", [0, 1])
def test_staging_seams(lbm, monkeypatch, nts):
    nx, ny = 16384, 130
    lattice_rows = (64 << 20) // (nx * 9 * 8)
    final_rows = (16 << 20) // (nx * 8)
    for rows in (lattice_rows, final_rows):      # at least two chunks and a ragged last one
        assert 1 <= rows < ny and ny % rows != 0, rows
    case = random_case(nx, ny, set())
    ob, start, n = case["ob"], case["start"], case["n"]
    with engine(lbm, monkeypatch, nx, ny, nts, 1, ob, start) as eng:
        got = eng.cells()
        assert_same(got, start, "cells() after the upload")
        del got
        final = eng.final_state()
        av_now, mass = eng.av_velocity(), eng.total_density()
    want = double_model.final_state(start, ob, DENSITY)
    for name in FIELDS:
        assert_same(final[name], want[name], name)
    del final, want
    tot_u, cells_in = double_model.tot_u(start, ob)
    assert cells_in == n
    assert abs(av_now - tot_u / n) / (tot_u / n) <= sum_order_bound(n)
    total = float(start.sum())
    assert abs(mass - total) / total <= sum_order_bound(9 * nx * ny)
    del case, start, ob
