"""The fast-math model of tests/fast_model.py, checked on the CPU (no GPU): the oracle's fmaf rounds once, its fast collision
stays within the derived bound of the rational / float64 BGK collision, the fast run is one function of its steps, and the
cases of tests/test_gpu_fast.py select -- by the planner's own answer -- every row of the fast dispatch tables."""
import collections
import ctypes

import numpy as np
import pytest

import av_model
import fast_model
import plan_tool
from fast_model import CASES, F, OMEGAS, U

P = collections.namedtuple("P", "nx ny max_iters reynolds_dim density accel omega")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def collide_cells(oracle, t, omega):
    """collision_fast on a row of cells: (relaxed (n, 9), u_sq (n,))."""
    n = len(t)
    p = P(n, 1, 1, 1, 0.1, 0.005, omega)
    out, usq = oracle.collision_fast(p, np.ascontiguousarray(t).reshape(1, n, 9), np.zeros((1, n), dtype=np.int32))
    return out.reshape(n, 9), usq.reshape(n)


# ---- fmaf is a real fused multiply-add --------------------------------------------------------------------------------------
def find_fma_witnesses(seed=7, count=6):
    """Seeded search for fp32 triples on which the two cheap imitations of an FMA both miss the correctly rounded
    a*b + c: float32(float64(a) * float64(b) + float64(c)) (rounding twice) and float32(float32(a * b) + c) (no fusion).
    a = 1 + m 2^-12, b = 1 + n 2^-12 with m, n odd: the product ends in the bit 2^-24, half an ulp of fp32, so it lies on
    the midpoint of two fp32 neighbours; c = +-2^-k, k >= 56, decides the side but is lost when the sum is first
    rounded to 53 bits, and the tie then goes to the even neighbour -- the wrong one in half of the draws."""
    rng = np.random.default_rng(seed)
    found = []
    while len(found) < count:
        m, n = (2 * int(rng.integers(0, 1024)) + 1 for _ in range(2))
        a, b = np.float32(1 + m * 2.0 ** -12), np.float32(1 + n * 2.0 ** -12)
        c = np.float32(float(rng.choice([-1, 1])) * 2.0 ** -int(rng.integers(56, 90)))
        exact = fast_model.round_to_float32(F(float(a)) * F(float(b)) + F(float(c)))
        twice = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
        unfused = np.float32(np.float32(a * b) + c)
        if twice != exact and unfused != exact:
            found.append((float(a).hex(), float(b).hex(), float(c).hex()))
    return found


# find_fma_witnesses(seed=7, count=6), hard-coded; test_fma_witnesses_are_witnesses repeats the search
FMA_WITNESSES = [
    ("0x1.4a10000000000p+0", "0x1.6350000000000p+0", "0x1.0000000000000p-63"),
    ("0x1.0710000000000p+0", "0x1.2670000000000p+0", "-0x1.0000000000000p-85"),
    ("0x1.74d0000000000p+0", "0x1.00b0000000000p+0", "-0x1.0000000000000p-83"),
    ("0x1.5c10000000000p+0", "0x1.2090000000000p+0", "0x1.0000000000000p-71"),
    ("0x1.4130000000000p+0", "0x1.7f70000000000p+0", "0x1.0000000000000p-82"),
    ("0x1.6dd0000000000p+0", "0x1.4e70000000000p+0", "-0x1.0000000000000p-57"),
]


def test_fma_witnesses_are_witnesses():
    assert find_fma_witnesses(seed=7, count=len(FMA_WITNESSES)) == FMA_WITNESSES
    assert len(FMA_WITNESSES) >= 4


@pytest.mark.parametrize("w", FMA_WITNESSES, ids=lambda w: w[0])
def test_oracle_fmaf_rounds_once(oracle, w):
    a, b, c = (np.float32(float.fromhex(x)) for x in w)
    exact = fast_model.round_to_float32(F(float(a)) * F(float(b)) + F(float(c)))
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) != exact       # rounding twice misses
    assert np.float32(np.float32(a * b) + c) != exact                               # not fusing misses
    assert bits(oracle.fmaf(a, b, c)) == bits(exact)


def test_round_to_float32():
    """The Fraction rounding the witnesses are judged by: exact on fp32 values, ties to even, and the nearest of the two
    neighbours otherwise."""
    rng = np.random.default_rng(3)
    for x in rng.standard_normal(200).astype(np.float32):
        assert fast_model.round_to_float32(F(float(x))) == x
    one = F(1)
    assert fast_model.round_to_float32(one + F(1, 2 ** 24)) == np.float32(1)                    # tie: to even (down)
    assert fast_model.round_to_float32(one + F(3, 2 ** 24)) == np.float32(1 + 2.0 ** -22)       # tie: to even (up)
    assert fast_model.round_to_float32(one + F(1, 2 ** 24) + F(1, 2 ** 60)) == np.float32(1 + 2.0 ** -23)
    assert fast_model.round_to_float32(-(one + F(1, 2 ** 24) - F(1, 2 ** 60))) == np.float32(-1)


# ---- one collision against the exact BGK collision ---------------------------------------------------------------------------
def test_weights_are_within_one_rounding_of_their_fractions():
    """kW0, kW1, kW2 (lbm_kernels.hip.h:54-56; the oracle's w0, w1, w2): the fp32 quotients 4.f / 9.f, 1.f / 9.f,
    1.f / 36.f, each within 2^-24 relative of its fraction, as the bound assumes."""
    for num, den in ((4, 9), (1, 9), (1, 36)):
        w = np.float32(num) / np.float32(den)
        assert w.dtype == np.float32
        assert abs(F(float(w)) - F(num, den)) <= F(num, den) * F(1, 2 ** 24)


def test_collision_cells_have_the_required_spread():
    t, kind = fast_model.collision_cells()
    _, _, rho, ux, uy = fast_model.bgk_float64(t, 1.85)
    speed = np.sqrt(ux * ux + uy * uy)
    assert len(t) >= 5000 and (t > 0).all()
    assert rho.min() < 0.012 and rho.max() > 0.8 and 1e-3 <= rho.min() and rho.max() <= 10       # two decades around 0.1
    assert speed.max() <= fast_model.UMAX
    assert ((speed >= 0.1) & (speed <= 0.3)).mean() >= 0.25
    assert (speed == 0).sum() >= 100                                                             # at rest exactly
    assert ((t[:, 0] / rho) > 0.95).sum() >= 100                                                 # one population dominating
    pair = np.max([t[:, a] + t[:, b] for a, b in ((1, 3), (2, 4), (5, 7), (6, 8))], axis=0)
    assert ((pair / rho) > 0.85).sum() >= 100                                                    # cancellation at full size


def test_float64_reference_is_exact_enough():
    """The float64 evaluation of R_k stays within 2^-20 of the BOUND of the rational one (it carries some twenty
    roundings of 2^-53), on a seeded subset of the cells and every omega."""
    t, _ = fast_model.collision_cells()
    pick = np.random.default_rng(11).choice(len(t), 150, replace=False)
    for omega in OMEGAS:
        R, bound, *_ = fast_model.bgk_float64(t[pick], omega)
        for i, cell in enumerate(t[pick]):
            exact = fast_model.bgk_fraction(cell, omega)
            for k in range(9):
                assert abs(F(float(R[i, k])) - exact[k]) <= F(float(bound[i, k])) / 2 ** 20


@pytest.mark.parametrize("omega", OMEGAS)
def test_fast_collision_within_the_derived_bound_of_bgk(oracle, omega):
    """Every population of every cell: |r_k - R_k| <= (A_k omega w_k P q_k + B |t_k|) 2^-24 (fast_model's docstring).
    The largest error / bound is printed; it never feeds back into the bound.  A bound twenty times slack would not see
    a constant that is off in its fourth digit: the figure has to stay above 0.05."""
    t, _ = fast_model.collision_cells()
    got, usq = collide_cells(oracle, t, omega)
    R, bound, rho, ux, uy = fast_model.bgk_float64(t, omega)
    ratio = np.abs(got.astype(np.float64) - R) / bound
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"fast collision vs float64 BGK, omega {omega}: A = {fast_model.A_REST}/{fast_model.A_AXIS}/{fast_model.A_DIAG}, "
          f"B = {fast_model.b_of(np.float32(omega)):.2f}, largest error / bound {ratio.max():.3f} (cell {worst[0]}, "
          f"population {worst[1]})")
    assert ratio.max() < 1.0
    assert ratio.max() > 0.05
    # u_sq, the value behind av_vels: two products and a sum of values each within 4.8u of U_x, U_y
    want = ux * ux + uy * uy
    assert np.all(np.abs(usq - want) <= (2 * (np.abs(ux) + np.abs(uy)) * (3 + 6 * fast_model.UMAX) + 2 * want) * U * 1.001)


# ---- the fast run is one function of its steps ---------------------------------------------------------------------------------
def test_run_fast_is_n_single_steps(oracle):
    p, ob, cells = av_model.lattice(130, 9)
    whole = cells.copy()
    usq = oracle.run_fast(p, whole, ob, 7, want_usq=True)
    split = cells.copy()
    for t in range(7):
        one = oracle.run_fast(p, split, ob, 1, want_usq=True)
        assert np.array_equal(bits(one[0]), bits(usq[t]))
    assert np.array_equal(bits(whole), bits(split))
    assert not usq[:, ob != 0].any() and (usq[:, ob == 0] > 0).all()
    again = cells.copy()
    assert oracle.run_fast(p, again, ob, 7) is None
    assert np.array_equal(bits(whole), bits(again))


def test_run_fast_is_the_four_sweeps_with_the_fast_collision(oracle):
    """accelerate, propagate, rebound (the oracle's own sweeps) and collision_fast, driven from here."""
    p, ob, cells = av_model.lattice(33, 19)
    ob = np.ascontiguousarray(ob, dtype=np.int32)
    whole = cells.copy()
    oracle.run_fast(p, whole, ob, 5)
    cur, tmp = cells.copy(), np.empty_like(cells)
    cp = ctypes.byref(oracle.cparams(p))
    for _ in range(5):
        oracle.lib.lbm_oracle_accelerate_flow(cp, cur.ctypes.data, ob.ctypes.data)
        oracle.lib.lbm_oracle_propagate(cp, cur.ctypes.data, tmp.ctypes.data)
        oracle.lib.lbm_oracle_rebound(cp, cur.ctypes.data, tmp.ctypes.data, ob.ctypes.data)
        blocked_before = cur[ob != 0].copy()
        cur, _ = oracle.collision_fast(p, tmp, ob, cells=cur)
        assert np.array_equal(bits(cur[ob != 0]), bits(blocked_before))             # blocked cells untouched
    assert np.array_equal(bits(whole), bits(cur))


def test_fast_run_conserves_mass(oracle):
    """Propagation and rebound move populations, the lid acceleration adds to three what it takes from three others (six
    roundings on one row), and the collision conserves the density up to the bound of fast_model summed over a cell's
    nine populations: sum_k A_k w_k = 17 * 4/9 + 33 * 4/9 + 49 * 4/36 = 27.7, times omega = 1.85 and q <= 1.3 (|u| < 0.1
    on this lattice), plus B = 2.55: 69 roundings of 2^-24, 72 with the lid's.  So over 50 steps of the 130x9 case the
    total mass (float64 sum) moves by at most 50 x 72 x 2^-24 relative -- and, the errors being signed, by far less."""
    p, ob, cells = av_model.lattice(130, 9)
    cur = cells.copy()
    before = cur.astype(np.float64).sum()
    usq = oracle.run_fast(p, cur, ob, 50, want_usq=True)
    after = cur.astype(np.float64).sum()
    print(f"fast run, 130x9, 50 steps: relative mass change {(after - before) / before:.3e}")
    assert float(usq.max()) < 0.1 ** 2
    assert abs(after - before) <= 50 * 72 * U * before
    assert np.isfinite(cur).all() and (cur > 0).all()


def test_fast_is_not_exact(oracle):
    p, ob, cells = av_model.lattice(320, 12)
    exact = cells.copy()
    oracle.run(p, exact, ob, 1)
    assert not np.array_equal(bits(exact), bits(fast_model.model(320, 12, 1).cells))


# ---- coverage: the cases and the dispatch tables ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return plan_tool.build(tmp_path_factory.mktemp("plan_dump_fast"))


def info_of_plan(plan, halo):
    """lbm_get_info's selection entries (lbm_hip.hip:2669-2685) of a synchronous context with this plan."""
    tile = plan["tile_steps"] and not halo
    stream = plan["fuse2"] and not tile
    adv = plan["tile_steps"] if tile else (plan["pass_steps"] if plan["fuse2"] else 1)
    passes = 64 // adv                      # chunk_passes, :1159-1168 (kPartSlots = 64)
    return {"steps_per_launch": adv, "band_rows": plan["band_rows"] if stream else 0,
            "lane_cells": plan["lane_cells"] if stream else 0, "nontemporal": plan["nts"],
            "graph_steps": (passes - (passes & 1)) * adv if plan["use_graph"] else 0,
            "resident_steps": 4096 if plan["resident"] else 0,
            "resident_min_steps": plan["resident_min_steps"] if plan["resident"] else 0,
            "band_groups": plan["band_groups"] if stream else 1}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_planner_selects_the_case_row(plan_dump, case):
    halo = case.slabs > 1
    env = {k: v for k, v in case.env.items() if k != "LBM_HALO"}
    got = plan_tool.run(plan_dump, nx=case.nx, ny=case.ny, n_slabs=case.slabs,
                        halo=plan_tool.HALO["memcpy"] if halo else plan_tool.HALO["none"], cus=256, env=env)
    plan = got["plan"]
    assert not plan["resident"]
    rows = fast_model.planned_rows(plan, halo)
    assert rows[0] == case.row, (rows, plan)
    assert all(r in fast_model.ALL_ROWS for r in rows)
    info = info_of_plan(plan, halo)
    for key, want in case.expect.items():
        assert info[key] == want, (key, info)
    if case.family == "default":
        assert plan["tile_steps"] == 4 and plan["tile_shape"] == 0 and not plan["fuse2"]
    if case.family == "step_tile":
        assert plan["tile_shape"] == case.tile


def test_cases_cover_every_row_of_the_fast_dispatch_tables():
    named = {c.row for c in CASES}
    assert len(fast_model.ALL_ROWS) == 6 + 1 + 4 + 10 + 7 == len(set(fast_model.ALL_ROWS))
    assert all(":" in where for _, where in fast_model.FAST_DISPATCH.values())       # every table names its lines
    missing = [r for r in fast_model.ALL_ROWS if r not in named]
    assert not missing, f"no GPU case for {missing}"
    assert named <= set(fast_model.ALL_ROWS)
    # both splittings unless the case says otherwise, and every case long enough for full passes, a remainder and an odd step
    for c in CASES:
        assert c.calls == ((13,), (1, 2, 5, 5)) or c.family == "graph"
        assert c.steps > 2 * c.expect["steps_per_launch"] or c.expect["steps_per_launch"] == 8


def test_packed_plan_is_not_a_fast_row(plan_dump):
    """The default packed plan serves both modes with the exact kernels: only the odd last step is a fast kernel."""
    nx, ny = fast_model.PACKED_SHAPE
    plan = plan_tool.run(plan_dump, nx=nx, ny=ny, cus=256, env=fast_model.PACKED_ENV)["plan"]
    assert plan["packed"] == 1 and plan["pass_steps"] == 4 and plan["band_groups"] == 1 and plan["vec4"] == 1
    info = info_of_plan(plan, False)
    for key, want in fast_model.PACKED_EXPECT.items():
        assert info[key] == want


# ---- the av_vels bound in fast mode ------------------------------------------------------------------------------------------------
def test_fast_argument_leaves_the_exact_bound_alone():
    for case in av_model.CASES:
        exact = av_model.bound(case.expect, case.tile, case.packed)
        assert av_model.bound(case.expect, case.tile, case.packed, fast=False) == exact == case.bound()
        assert av_model.speed_mode(case.expect) == av_model.speed_mode(case.expect, fast=False)
        assert av_model.bound(case.expect, case.tile, case.packed, fast=True) == \
            exact + (1 - av_model.speed_mode(case.expect)) * av_model.ULP
    one = {"steps_per_launch": 1, "lane_cells": 0}
    assert av_model.speed_mode(one) == 0 and av_model.speed_mode(one, fast=True) == 1
    assert av_model.bound(one, fast=True) == (14 + 2) * U + av_model.ULP            # step_vec4's depth, s = 1


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_fast_case_keeps_depth_40(case):
    assert av_model.depth(case.expect, case.tile, case.packed) <= av_model.DEPTH_MAX
    assert case.bound() <= (av_model.DEPTH_MAX + 2) * U + av_model.ULP
