"""av_vels of the fp32 engine on every kernel family, held to a derived bound.

The lattice and the per-cell fields are compared bit for bit elsewhere; av_vels is the one output whose correctness does
not follow from a correct lattice: every multi-step kernel decides per sub-step which of its redundantly relaxed rows
and lanes are its own, and the sums go into per-step partial slots.  A cell counted twice at a strip seam, a cell missed
at a ragged edge or a partial in the neighbouring sub-step's slot leaves the lattice bit-exact and moves av_vels by one
cell's weight -- which the 2e-4 against the reference's sequential fp32 sum cannot see on a grid of 5 000 cells or more.

Here every step of every case meets

    |av_vels[t] - want_av(map_t)| <= bound(info) * want_av(map_t) + 2^-63

in float64, where map_t is the per-cell |u| the kernel adds (tests/av_model.py: `relaxed` for the SPEED = 0 kernels,
`moment` for the SPEED = 1 ones, both from the oracle's four sweeps) and bound = (depth + 2) 2^-24 + s 2^-23 with depth
read from the kernel source.  tests/test_av_model.py shows on the CPU that one cell's weight is at least 8 x bound on
every lattice used here.  Each case prints its largest error / bound; the figure never feeds back into the bound.
"""
import numpy as np
import pytest

import av_model
from av_model import CASES, FLUSH_ALLOWANCE, U

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_selected(case, info):
    """The knobs selected the kernel the case is about (Engine.info())."""
    for key, want in case.expect.items():
        if key == "resident_steps":
            assert (info[key] > 0) == (want > 0), (key, info)
        else:
            assert info[key] == want, (key, info)
    assert info["n_slabs"] == case.slabs


def run_case(lbm, case, calls):
    p, ob, cells = av_model.case_inputs(case)
    kwargs = {"n_gpus": case.slabs}
    if case.rank:
        kwargs = {"rank": 0, "world_size": 1, "unique_id": lbm.rccl_unique_id(), "device": 0}
    with lbm.Engine(p, ob, cells.copy(), **kwargs) as eng:
        info = eng.info()
        assert_selected(case, info)
        for n in calls:
            eng.run(n)
        return info, eng.cells(), eng.av_vels(sum(calls)).astype(np.float64)


def check_av(case, info, got_av, what):
    _, ob, _ = av_model.case_inputs(case)
    want = av_model.case_model(case)
    maps = want.moment if case.speed == "moment" else want.relaxed
    assert av_model.speed_mode(info) == (1 if case.speed == "moment" else 0)
    bound = case.bound(info)
    assert bound == case.bound()                       # the bound the CPU coverage check was made with
    want_av = np.array([av_model.want_av(m, ob) for m in maps])
    err = np.abs(got_av - want_av)
    ratio = float(np.max(err / (bound * want_av + FLUSH_ALLOWANCE)))
    print(f"av_ratio {case.family} {case.id} {what}: bound {bound / U:.0f} u, largest error / bound {ratio:.3f} "
          f"at step {int(np.argmax(err / want_av))}")
    bad = np.nonzero(err > bound * want_av + FLUSH_ALLOWANCE)[0]
    assert len(bad) == 0, (f"{case.id} {what}: av_vels off the float64 sum of the per-cell values by more than "
                           f"{bound:.3e} relative at steps {bad[:16].tolist()}: {(err / want_av)[bad[:16]].tolist()}")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_av_vels_within_the_derived_bound(lbm, monkeypatch, case):
    for key, value in case.env.items():
        monkeypatch.setenv(key, value)
    want = av_model.case_model(case)
    for calls in case.calls:
        info, got_cells, got_av = run_case(lbm, case, calls)
        assert np.array_equal(bits(got_cells), bits(want.cells)), f"{case.id} {list(calls)}: lattice differs"
        check_av(case, info, got_av, list(calls))


# ---- the readers: av_velocity() and reynolds() of the stored lattice --------------------------------------------------------
@pytest.mark.parametrize("nx,ny,env", [(130, 9, {"LBM_FUSE2": "0"}), (320, 24, {"LBM_RESIDENT": "0"})])
def test_readers_against_the_float64_sum(lbm, monkeypatch, nx, ny, env):
    """lbm_av_velocity: lattice_sums adds the cells' IEEE |u| (moments_exact, sqrtf: the relaxed map's bits) in double
    (lbm_kernels.hip.h:2716-2737; the host adds the 1024 workgroup sums in double, lbm_hip.hip:3165), n additions of
    2^-53 at the most; then (float)speed / (float)fluid_cells (lbm_hip.hip:3188): two fp32 roundings.
    lbm_calc_reynolds (lbm_hip.hip:3204-3205): av * reynolds_dim / viscosity, two more, with the viscosity
    1.f / 6.f * (2.f / omega - 1.f) in fp32, restated here operation by operation."""
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    steps = 13
    p, ob, cells = av_model.lattice(nx, ny)
    want = av_model.model(nx, ny, steps)
    n = int((ob == 0).sum())
    want_av = av_model.want_av(want.relaxed[-1], ob)
    with lbm.Engine(p, ob, cells.copy()) as eng:
        eng.run(steps)
        got_av, got_re = eng.av_velocity(), eng.reynolds()
        assert np.array_equal(bits(eng.cells()), bits(want.cells))
    bound_av = n * 2.0 ** -53 + 2 * U
    print(f"av_ratio readers {nx}x{ny}: av_velocity error / bound {abs(got_av - want_av) / (bound_av * want_av):.3f}")
    assert abs(got_av - want_av) <= bound_av * want_av
    f32 = np.float32
    viscosity = f32(f32(1) / f32(6)) * f32(f32(f32(2) / f32(p.omega)) - f32(1))
    assert viscosity.dtype == np.float32
    want_re = want_av * p.reynolds_dim / float(viscosity)
    bound_re = n * 2.0 ** -53 + 4 * U
    print(f"av_ratio readers {nx}x{ny}: reynolds error / bound {abs(got_re - want_re) / (bound_re * want_re):.3f}")
    assert abs(got_re - want_re) <= bound_re * want_re
