"""The inputs of tests/edge_lattice.py do what they claim, by the CPU oracle alone: every guard cell arrives at the first
collision as placed, on the intended side of every guard; the lid row offers accelerate_flow accepting, refusing and
disagreeing cells in both cells of a pair before each of the 13 steps; and the lattice stays finite.  Conditions on the
inputs, not measurements of any kernel: the GPU comparison (test_gpu_edge_arithmetic.py) means nothing without them."""
import ctypes

import numpy as np
import pytest

import double_model
import edge_lattice as el

SHAPES = [(256, 40), (130, 12)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_guard_cells_arrive_as_placed(lbm, oracle, nx, ny):
    """accelerate_flow and propagate of step 0, by the oracle: the cell each placement sees at its first collision is T,
    bit for bit -- on the lid row too -- and the mask around it is what the placement says."""
    p, ob, cells, placed = el.build(lbm, nx, ny)
    cp = oracle.cparams(p)
    oracle.lib.lbm_oracle_accelerate_flow(ctypes.byref(cp), cells.ctypes.data, ob.ctypes.data)
    tmp = np.empty_like(cells)
    oracle.lib.lbm_oracle_propagate(ctypes.byref(cp), cells.ctypes.data, tmp.ctypes.data)
    assert len(placed) == 7 * len(el.GUARD_KINDS)
    for q in placed:
        assert np.array_equal(bits(tmp[q["y"], q["x"]]), bits(q["T"])), (q["kind"], q["x"], q["y"])
        assert ob[q["y"], q["x"]] == 0
        assert (q["y"] == ny - 2) == (q["where"] == "lid")
        assert (ob[q["y"], q["x"] ^ 1] != 0) == (q["where"] == "pair blocked"), (q["kind"], q["x"], q["y"])
    for kind in el.GUARD_KINDS:
        mine = [q for q in placed if q["kind"] == kind]
        assert sorted(q["x"] % 4 for q in mine if q["where"] == "plain") == [0, 1, 2, 3], kind
        assert sorted(q["x"] % 2 for q in mine if q["where"] == "pair blocked") == [0, 1], kind
        assert sum(q["where"] == "lid" for q in mine) == 1, kind


def test_guard_kinds_sit_where_they_claim():
    """Density (the sequential fp32 sum of moments_exact), numerators and |u|^2 of every kind, in fp32, against the
    bounds of the guards: 2^-60 <= rho < 2^60, |u|^2 < 5e28, |numerator| >= 2^-103."""
    m = {kind: el.moments_fp32(t) for kind, t in el.GUARD_KINDS.items()}
    tiny = np.finfo(np.float32).tiny
    in_range = lambda rho: el.RHO_LO <= rho < el.RHO_HI
    zero = np.float32(0)
    assert m["rho=2^-60"]["rho"] == np.float32(2.0 ** -60)
    assert m["rho=pred(2^-60)"]["rho"] == np.nextafter(np.float32(2.0 ** -60), zero)
    assert m["rho=2^60"]["rho"] == np.float32(2.0 ** 60)
    assert m["rho=pred(2^60)"]["rho"] == np.nextafter(np.float32(2.0 ** 60), zero)
    assert in_range(m["rho=2^-60"]["rho"]) and not in_range(m["rho=pred(2^-60)"]["rho"])
    assert in_range(m["rho=pred(2^60)"]["rho"]) and not in_range(m["rho=2^60"]["rho"])
    assert m["rho<0"]["rho"] < 0 and abs(m["rho<0"]["rho"]) > el.RHO_LO and m["rho<0"]["u_sq"] < 1
    for kind in ("u_sq>=5e28", "u_sq<5e28"):
        assert m[kind]["rho"] == np.float32(2.0 ** -40) and in_range(m[kind]["rho"]) and np.isfinite(m[kind]["u_sq"])
    assert m["u_sq>=5e28"]["u_sq"] >= el.U_SQ_GUARD
    # below the guard, with (u_x + u_y)^2 and 2 |u|^2 in the last decade below the fast divides' 1e29
    assert np.float32(2.5e28) < m["u_sq<5e28"]["u_sq"] < el.U_SQ_GUARD
    assert in_range(m["numerator<2^-103"]["rho"]) and tiny <= m["numerator<2^-103"]["num_x"] < el.NUMERATOR_LO
    assert in_range(m["numerator denormal"]["rho"]) and 0 < m["numerator denormal"]["num_x"] < tiny
    faint = el.GUARD_KINDS["all denormal"]
    assert ((faint > 0) & (faint < tiny)).all() and 0 < m["all denormal"]["rho"] < el.RHO_LO
    assert np.float32(2.0 ** 59) <= m["rho=2^59"]["rho"] < el.RHO_HI
    # far below the range with ordinary numbers: no denormal anywhere, a numerator below 2^-103 and a velocity that counts
    small = el.GUARD_KINDS["rho=2^-100"]
    assert (small >= tiny).all() and tiny < m["rho=2^-100"]["rho"] < el.RHO_LO
    assert tiny <= m["rho=2^-100"]["num_x"] < el.NUMERATOR_LO and m["rho=2^-100"]["u_x"] > np.float32(2.0 ** -25)
    for kind, mk in m.items():                       # everywhere else: the plain range and small velocities
        if kind not in ("u_sq>=5e28", "u_sq<5e28"):
            assert mk["u_sq"] < 1, kind


@pytest.mark.parametrize("when", [1, 2])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_overflowing_cell_gives_inf_and_no_nan(lbm, oracle, nx, ny, when):
    """The one cell that tells the |u|^2 guard's IEEE path from the fast divides: it reaches the collision of step `when`
    as placed, the oracle relaxes it to +Inf in six populations, and after `when` steps there is no NaN and no other Inf in
    the lattice (so bits can be compared); among fluid neighbours there is one step later."""
    m = el.moments_fp32(el.OVERFLOW_T)
    assert m["rho"] == np.float32(2.0 ** -40) and el.U_SQ_GUARD <= m["u_sq"] < np.float32(2.26e38)
    assert np.float32(m["u_x"] * m["u_x"]) >= el.QUOTIENT_OVERFLOWS_FROM
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(m["u_x"] * m["u_x"]) / np.float32(2.0 / 9.0)) and np.isfinite(m["u_sq"] / np.float32(2.0 / 3.0))
    p, ob, cells, placed = el.build_overflow(lbm, nx, ny, when)
    cp = oracle.cparams(p)
    before = cells.copy()
    oracle.run(p, before, ob, when - 1)
    oracle.lib.lbm_oracle_accelerate_flow(ctypes.byref(cp), before.ctypes.data, ob.ctypes.data)
    tmp = np.empty_like(before)
    oracle.lib.lbm_oracle_propagate(ctypes.byref(cp), before.ctypes.data, tmp.ctypes.data)
    assert sorted(q["x"] % 4 for q in placed if q["where"] == "plain") == [0, 0, 1, 1, 2, 2, 3, 3]
    assert sorted(q["x"] % 2 for q in placed if q["where"] == "lid") == [0, 1]
    for q in placed:
        # (in its box the cell keeps the rest population step 1 left it, which the sum f0 + f1 absorbs: same moments)
        assert np.array_equal(bits(tmp[q["y"], q["x"], when - 1:]), bits(q["T"][when - 1:])), (q["x"], q["y"])
        assert el.moments_fp32(tmp[q["y"], q["x"]]) == m, (q["x"], q["y"])
        assert ob[q["y"], q["x"]] == 0 and (ob[q["y"], q["x"] ^ 1] != 0) == (when == 2)
    oracle.run(p, cells, ob, when)
    assert not np.isnan(cells).any()
    want_inf = np.zeros(cells.shape, dtype=bool)
    for q in placed:
        want_inf[q["y"], q["x"], list(el.OVERFLOWS)] = True
    assert np.array_equal(np.isposinf(cells), want_inf) and not np.isneginf(cells).any()
    if when == 1:                               # (in the box the Inf comes back to arithmetic two steps later)
        oracle.run(p, cells, ob, 1)
        assert np.isnan(cells).any()


def test_lid_specials_hang_on_one_comparison():
    for dtype in (np.float32, np.float64):
        cells = np.ones((4, 128, 9), dtype=dtype)
        ob = np.ones((4, 128), dtype=np.int32)
        a1, a2 = el.accel_terms(el.DENSITY, el.ACCEL, dtype)
        specials = el.place_lid_specials(cells, ob, el.DENSITY, el.ACCEL)
        c3, c6, c7 = el.verdicts(cells[2], a1, a2)
        for x, name, accepts in specials:
            assert ob[2, x] == 0 and bool(c3[x] & c6[x] & c7[x]) == accepts, (name, x)
        by_name = {}
        for x, name, _ in specials:
            by_name.setdefault(name, []).append(x)
        assert all(sorted(x % 2 for x in xs) == [0, 1] for xs in by_name.values()), by_name
        x = by_name["f3==a1"][0]
        assert cells[2, x, 3] - a1 == 0 and cells[2, x, 6] - a2 > 0 and cells[2, x, 7] - a2 > 0
        x = by_name["f3==next(a1)"][0]
        assert cells[2, x, 3] - a1 > 0 and cells[2, x, 3] - a1 <= np.spacing(a1)
        x = by_name["f6==a2"][0]
        assert cells[2, x, 6] - a2 == 0 and cells[2, x, 3] - a1 > 0 and cells[2, x, 7] - a2 > 0
        x = by_name["f7<0"][0]
        assert cells[2, x, 7] < 0 and cells[2, x, 3] - a1 > 0 and cells[2, x, 6] - a2 > 0
        # the exact zero and its accepting neighbour share an aligned pair, both ways round
        pairs = {(x // 2, accepts) for x, name, accepts in specials if name.startswith("f3==")}
        assert len({i for i, _ in pairs}) == 2 and len(pairs) == 4


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_lid_row_is_covered_before_every_step(lbm, oracle, nx, ny):
    """The oracle one step at a time: before each of the 13 steps the lid row holds, in each x-parity, at least 4 fluid
    cells that accept, 4 that refuse and 4 whose sub-conditions disagree, and at least 4 aligned pairs with two
    verdicts; after them the lattice is finite."""
    p, ob, cells, _ = el.build(lbm, nx, ny)
    a1, a2 = el.accel_terms(p.density, p.accel)
    for t in range(el.STEPS):
        el.assert_covered(el.coverage(cells[ny - 2], ob[ny - 2], a1, a2), (nx, ny, t))
        av = oracle.run(p, cells, ob, 1)
        # what the recorders sample and the readers return is compared as bits: no NaN or Inf may be among it
        assert np.isfinite(av).all() and all(np.isfinite(f).all() for f in oracle.final_state(p, cells, ob).values()), t
    assert np.isfinite(cells).all()
    assert np.abs(cells).max() < 1e30          # eight decades of fp32 left


def test_second_batch_member_meets_its_threshold(lbm):
    """accel = 0.02 on the same ramp: the threshold lies at the ramp's crest, so the verdicts differ from member 0's."""
    p, ob, cells, _ = el.build(lbm, 256, 40, accel=0.02)
    cov = el.coverage(cells[38], ob[38], *el.accel_terms(p.density, 0.02))
    assert min(cov[0]["accept"], cov[1]["accept"], cov[0]["refuse"], cov[1]["refuse"]) >= 1, cov
    other = el.build(lbm, 256, 40)
    v = lambda q, accel: np.logical_and.reduce(el.verdicts(q[2][38], *el.accel_terms(el.DENSITY, accel)))
    assert (v((p, ob, cells), 0.02) != v(other, el.ACCEL)).sum() >= 16


def test_double_lattice_is_covered_before_every_step():
    """The double engine's case (128 x 16, ramp and lid specials only), by the float64 model."""
    ob, cells = el.build_double(128, 16)
    a1, a2 = el.accel_terms(el.DENSITY, el.ACCEL, np.float64)
    for t in range(el.STEPS):
        el.assert_covered(el.coverage(cells[14], ob[14], a1, a2), ("double", t))
        double_model.timestep(cells, ob, el.DENSITY, el.ACCEL, el.OMEGA)
    assert np.isfinite(cells).all()


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    import plan_tool
    return plan_tool, plan_tool.build(tmp_path_factory.mktemp("plan_dump"))


def test_kernel_cases_select_their_kernels(plan_dump):
    """What lbm_plan.h (the planner create_common runs on) makes of every case's knobs, without a device: the values
    Engine.info() is pinned to on the GPU, and the choices info() does not show (packed or scalar arithmetic, windows in
    LDS, prefetch, which tile shape)."""
    plan_tool, exe = plan_dump
    assert len({c["id"] for c in el.KERNEL_CASES}) == len(el.KERNEL_CASES)
    for c in el.KERNEL_CASES:
        nx, ny = c["shape"]
        got = plan_tool.run(exe, nx=nx, ny=ny, n_slabs=c["n_gpus"], halo=plan_tool.HALO[c["halo"]], cus=256, env=c["env"])
        pl = got["plan"]
        for k, v in c["plan"].items():
            assert pl[k] == v, (c["id"], k, pl)
        # lbm_get_info's reading of the plan
        stream = pl["fuse2"] and not (pl["tile_steps"] and c["halo"] == "none")
        info = {"steps_per_launch": pl["tile_steps"] if pl["tile_steps"] and c["halo"] == "none" else (pl["pass_steps"] if pl["fuse2"] else 1),
                "band_rows": pl["band_rows"] if stream else 0, "lane_cells": pl["lane_cells"] if stream else 0,
                "band_groups": pl["band_groups"] if stream else 1, "resident_steps": 4096 * pl["resident"],
                "resident_rows": pl["resident_rows"], "resident_group": pl["resident_group"], "resident_one_xcd": pl["resident_one_xcd"]}
        el.assert_pinned(info, c["pin"], c["id"])
        if c["n_gpus"] == 2:                    # the lid row is a halo row of slab 0, and slab 1's own
            assert [s["accel_row"] for s in got["slabs"]] == [-2, ny // 2 - 2], got["slabs"]
