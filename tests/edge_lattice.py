"""Lattices that drive the per-cell logic the near-equilibrium test lattices never reach: the refusal of
accelerate_flow (SerialCode/d2q9-bgk.c:229-242) and the edges of the exact kernels' guards (density within
[2^-60, 2^60), |u|^2 < 5e28, numerators below 2^-103: csrc/lbm_kernels.hip.h, "exact division").  Inputs only: the
oracle says what they do (tests/test_edge_lattice.py), the kernels are compared with it (tests/test_gpu_edge_arithmetic.py).

Refusal ramp.  Rows ny-4 .. ny-1 and row 0 of a random lattice (test_gpu_parity.random_case, weights x (1 +- 5 %)) are
scaled per column by s(x) = 0.00125 * 16^(|x mod 128 - 64| / 64): from 0.02 through the threshold s = accel down to
0.00125 and back, so the lid row ny-2 holds cells that accept, cells that refuse, and -- the noise -- cells whose three
sub-conditions disagree.  The cells of place_lid_specials sit on the lid row before step 0 (the first-step accelerate pass sees them).

Guard cells.  Each kind is a 9-vector T that is to be the PRE-COLLISION cell of the first step: its populations are
scattered against the stream directions into the 3 x 3 neighbourhood, whose obstacles are cleared first.  The three lid-row
cells that feed a placement on the lid row get f7 = 0, so step 0's acceleration refuses them and T arrives unchanged.
"""
import numpy as np

CX = (0, 1, 0, -1, 0, 1, -1, -1, 1)          # SerialCode/d2q9-bgk.c:9-15
CY = (0, 0, 1, 0, -1, 1, 1, -1, -1)
WEIGHTS = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)

DENSITY, ACCEL, OMEGA = 0.1, 0.005, 1.85
SEED = 4242
STEPS = 13                                    # the oracle's lattice stays finite this long (test_edge_lattice.py)

U_SQ_GUARD = np.float32(5.0e28)
RHO_LO, RHO_HI = np.float32(2.0 ** -60), np.float32(2.0 ** 60)
NUMERATOR_LO = np.float32(2.0 ** -103)


def _cell(**pops):
    t = np.zeros(9, dtype=np.float64)
    for name, v in pops.items():
        t[int(name[1])] = v
    return t


def _kinds():
    lo = _cell(f0=2.0 ** -61, f1=2.0 ** -63 + 2.0 ** -66, f2=2.0 ** -63, f3=2.0 ** -63 - 2.0 ** -66, f4=2.0 ** -63)
    lo_pred = lo.copy()
    lo_pred[2] = 2.0 ** -63 - 2.0 ** -84
    hi, hi_pred = lo * 2.0 ** 120, lo * 2.0 ** 120
    hi_pred[2] = 2.0 ** 57 - 2.0 ** 36
    tilted = WEIGHTS.copy()
    tilted[1] *= 1.1
    tilted[3] *= 0.9
    faint = WEIGHTS * 1e-40
    faint[1] *= 1.5
    faint[3] *= 0.5
    kinds = {
        "rho=2^-60": lo,
        "rho=pred(2^-60)": lo_pred,
        "rho=2^60": hi,
        "rho=pred(2^60)": hi_pred,
        "rho<0": -DENSITY * tilted,
        "u_sq>=5e28": _cell(f1=2.0 ** 7, f3=-2.0 ** 7, f4=2.0 ** -40),
        "u_sq<5e28": _cell(f1=0.7 * 2.0 ** 7, f3=-0.7 * 2.0 ** 7, f4=2.0 ** -40),
        "numerator<2^-103": _cell(f0=0.04, f1=1e-33),
        "numerator denormal": _cell(f0=0.04, f1=1e-40, f2=0.01, f4=0.01),
        "all denormal": faint,
        "rho=2^59": 2.0 ** 59 * tilted,
        "rho=2^-100": 2.0 ** -100 * tilted,
    }
    return {name: t.astype(np.float32) for name, t in kinds.items()}


GUARD_KINDS = _kinds()

# (rows of the placements off the lid row, column pitch, first column, lid-row columns of the guard cells): the pitch is
# odd, so four consecutive placements cover x mod 4 = 0, 1, 2, 3 and two consecutive ones both cells of a pair.  (Rows 6, 13, 23
# at 256 x 40 lead, after eight steps, to a cell whose populations of 1e21 sum to exactly 0: an infinite velocity in the
# oracle's own final_state and av_vels.  test_edge_lattice.py holds every step's fields and av_vels finite.)
LAYOUTS = {
    (256, 40): ((5, 14, 23), 9, 4, (4, 9, 14, 19, 44, 49, 54, 59, 136, 141, 146, 151)),
    (130, 12): ((2, 5), 3, 1, (1, 4, 7, 10, 13, 16, 19, 22, 50, 53, 56, 59)),
}
SPECIALS_X0 = 72                              # ten columns from here, in the ramp's refusing stretch


def moments_fp32(t):
    """rho (sequential sum in index order, as moments_exact takes it), the two numerators, u_x, u_y and |u|^2 of a
    cell, every operation rounded to fp32."""
    t = np.asarray(t, dtype=np.float32)
    rho = t[0]
    for k in range(1, 9):
        rho = np.float32(rho + t[k])
    with np.errstate(all="ignore"):
        num_x = np.float32(np.float32(np.float32(t[1] + t[5]) + t[8]) - np.float32(np.float32(t[3] + t[6]) + t[7]))
        num_y = np.float32(np.float32(np.float32(t[2] + t[5]) + t[6]) - np.float32(np.float32(t[4] + t[7]) + t[8]))
        ux, uy = np.float32(num_x / rho), np.float32(num_y / rho)
        u_sq = np.float32(np.float32(ux * ux) + np.float32(uy * uy))
    return {"rho": rho, "num_x": num_x, "num_y": num_y, "u_x": ux, "u_y": uy, "u_sq": u_sq}


def accel_terms(density, accel, dtype=np.float32):
    """a1, a2 as the host forms them: density * accel / 9 and / 36 in the lattice's own precision."""
    d, a = dtype(density), dtype(accel)
    return dtype(d * a / dtype(9)), dtype(d * a / dtype(36))


def ramp(nx, lo=0.00125, span=16.0):
    """lo at x mod 128 = 64, lo * span at x mod 128 = 0 (the defaults: the fp32 lattices' ramp)."""
    x = np.arange(nx)
    return lo * span ** (np.abs(x % 128 - 64) / 64.0)


def apply_ramp(cells, lo=0.00125, span=16.0):
    """In place, in the array's own precision."""
    ny, nx = cells.shape[:2]
    s = ramp(nx, lo, span).astype(cells.dtype)[:, None]
    for y in (ny - 4, ny - 3, ny - 2, ny - 1, 0):
        cells[y] *= s


def place_lid_specials(cells, ob, density, accel, x0=SPECIALS_X0):
    """Five lid-row cells whose verdict hangs on one comparison, each at an even and at an odd column, the exact-zero
    difference and its accepting neighbour sharing a pair both ways round.  Returns [(x, name, accepts)]."""
    dtype = cells.dtype.type
    a1, a2 = accel_terms(density, accel, dtype)
    lid = cells.shape[0] - 2
    ok1, ok2 = dtype(4) * a1, dtype(4) * a2                 # comfortably positive after the subtraction
    specials = [("f3==a1", {3: a1, 6: ok2, 7: ok2}, False),
                ("f3==next(a1)", {3: np.nextafter(a1, dtype(np.inf)), 6: ok2, 7: ok2}, True),
                ("f3==next(a1)", {3: np.nextafter(a1, dtype(np.inf)), 6: ok2, 7: ok2}, True),
                ("f3==a1", {3: a1, 6: ok2, 7: ok2}, False),
                ("f6==a2", {3: ok1, 6: a2, 7: ok2}, False),
                ("all zero", {k: dtype(0) for k in range(9)}, False),
                ("f7<0", {3: ok1, 6: ok2, 7: -ok2}, False),
                ("f6==a2", {3: ok1, 6: a2, 7: ok2}, False),
                ("all zero", {k: dtype(0) for k in range(9)}, False),
                ("f7<0", {3: ok1, 6: ok2, 7: -ok2}, False)]
    out = []
    for i, (name, pops, accepts) in enumerate(specials):
        x = x0 + i
        ob[lid, x] = 0
        for k, v in pops.items():
            cells[lid, x, k] = v
        out.append((x, name, accepts))
    return out


def _scatter(cells, ob, x, y, t):
    ny, nx = ob.shape
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ob[(y + dy) % ny, (x + dx) % nx] = 0
    for k in range(9):
        cells[(y - CY[k]) % ny, (x - CX[k]) % nx, k] = t[k]


def build(lbm, nx, ny, seed=SEED, accel=ACCEL, guards=True):
    """(p, ob, cells, placed): placed = [{"kind", "x", "y", "where": "plain" | "pair blocked" | "lid", "T"}], the
    guard cells (the lid specials: place_lid_specials)."""
    from test_gpu_parity import random_case
    p, ob, cells = random_case(lbm, nx, ny, seed, walls=False)
    p.accel = accel
    assert (p.density, p.omega) == (DENSITY, OMEGA)
    apply_ramp(cells)
    lid = ny - 2
    placed = []
    if guards:
        rows, pitch, x0, lid_xs = LAYOUTS[(nx, ny)]
        per_row = ((nx - 2 - x0) // pitch + 1) // 6 * 6           # a kind's six placements share a row
        slot = 0
        for kind, t in GUARD_KINDS.items():
            for variant in range(6):                       # four plain ones, two with the other cell of the pair blocked
                y, x = rows[slot // per_row], x0 + pitch * (slot % per_row)
                slot += 1
                _scatter(cells, ob, x, y, t)
                if variant >= 4:
                    ob[y, x ^ 1] = 1
                placed.append({"kind": kind, "x": x, "y": y, "where": "plain" if variant < 4 else "pair blocked", "T": t})
        assert slot <= per_row * len(rows)
        for (kind, t), x in zip(GUARD_KINDS.items(), lid_xs):
            _scatter(cells, ob, x, lid, t)
            for dx in (-1, 0, 1):                           # step 0 must not accelerate the cells that feed T
                cells[lid, x + dx, 7] = 0
            placed.append({"kind": kind, "x": x, "y": lid, "where": "lid", "T": t})
    place_lid_specials(cells, ob, p.density, accel)
    return p, ob, cells, placed


DOUBLE_SEED = 5     # of seeds 1..7 the one whose lid row keeps four accepting cells per parity through all 13 steps


def build_double(nx, ny, seed=DOUBLE_SEED, accel=ACCEL):
    """(ob, cells): the ramp and the lid specials on a float64 lattice of 0.5 .. 1.5 x equilibrium, the double engine's
    own test lattice (its arithmetic has no guards, so no guard cells)."""
    rng = np.random.default_rng(seed)
    ob = (rng.random((ny, nx)) < 0.05).astype(np.int32)
    ob[ny - 2, nx // 2] = 1
    cells = DENSITY * WEIGHTS * (0.5 + rng.random((ny, nx, 9)))
    apply_ramp(cells)
    place_lid_specials(cells, ob, DENSITY, accel)
    return ob, cells


# ---- a quotient that overflows ---------------------------------------------------------------------------------------
# The fast constant divide q = x R, r = fma(-C, q, x), q' = fma(r, R, q) equals x / C for every dividend of 1e28 and above
# whose IEEE quotient is finite; where x / C overflows it gives NaN (Inf - Inf) and IEEE gives Inf: from |x| = 7.56e37
# for C = 2 c_sq^2, 1.13e38 for c_sq, 2.27e38 for 2 c_sq (every fp32 dividend tried on the CPU).  So below an overflow
# the |u|^2 < 5e28 guard cannot be seen in any result, and only this cell sees it: rho = 2^-40, u_x = 2^63, u_x^2 = 2^126 =
# 8.5e37.  The oracle relaxes it to +Inf in the six populations with an x component and to finite values in the other
# three -- no NaN, so bits can be compared -- but the step after, the Inf meets arithmetic and becomes NaN.  Hence:
#   when = 1: T is the pre-collision cell of step 1 (scattered, fluid neighbours); run ONE step.
#   when = 2: the cell sits in a box of eight blocked cells and starts as T mirrored; the walls hand T's moving populations
#             back for the collision of step 2 (the rest population is step 1's, and vanishes in the sum next to 2^22), and
#             the Inf that leaves the cell is only copied by them; run TWO steps (one two-step pass).
OVERFLOW_T = _cell(f1=2.0 ** 22, f3=-2.0 ** 22, f4=2.0 ** -40).astype(np.float32)
OVERFLOWS = (1, 3, 5, 6, 7, 8)                # the populations the oracle relaxes to +Inf
QUOTIENT_OVERFLOWS_FROM = np.float32(7.56183145e37)
OPPOSITE = (0, 3, 4, 1, 2, 7, 8, 5, 6)


def build_overflow(lbm, nx, ny, when, seed=SEED):
    """(p, ob, cells, placed) on a plain random lattice: the overflowing cell at x mod 4 = 0, 1, 2, 3 on two rows and at
    both cells of a pair on the lid row."""
    from test_gpu_parity import random_case
    p, ob, cells = random_case(lbm, nx, ny, seed, walls=False)
    lid = ny - 2
    rows = (5, 14) if ny >= 20 else (2, 5)
    placed = []
    for x, y in [(4 + 9 * j, y) for y in rows for j in range(4)] + [(4, lid), (13, lid)]:
        if when == 1:
            _scatter(cells, ob, x, y, OVERFLOW_T)
            if y == lid:
                for dx in (-1, 0, 1):
                    cells[lid, x + dx, 7] = 0
        else:
            ob[y - 1:y + 2, x - 1:x + 2] = 1
            ob[y, x] = 0
            cells[y, x] = OVERFLOW_T[list(OPPOSITE)]
        placed.append({"kind": "quotient overflows", "x": x, "y": y, "where": "lid" if y == lid else "plain", "T": OVERFLOW_T})
    return p, ob, cells, placed


def verdicts(lid_cells, a1, a2):
    """The three sub-conditions of accelerate_flow on a row of cells, in the cells' own precision: (c3, c6, c7)."""
    return (lid_cells[:, 3] - a1) > 0, (lid_cells[:, 6] - a2) > 0, (lid_cells[:, 7] - a2) > 0


def coverage(lid_cells, lid_ob, a1, a2):
    """What the lid row offers accelerate_flow: per x-parity the fluid cells that accept, that refuse, and whose three
    sub-conditions disagree; and the aligned pairs (2i, 2i+1) of two fluid cells with different verdicts."""
    c3, c6, c7 = verdicts(lid_cells, a1, a2)
    fluid = np.asarray(lid_ob) == 0
    accept = c3 & c6 & c7
    mixed = (c3 | c6 | c7) & ~accept
    out = {}
    for parity in (0, 1):
        sel = fluid & (np.arange(len(fluid)) % 2 == parity)
        out[parity] = {"accept": int((accept & sel).sum()), "refuse": int((~accept & sel).sum()),
                       "mixed": int((mixed & sel).sum())}
    n = len(fluid) // 2 * 2
    out["split pairs"] = int((fluid[0:n:2] & fluid[1:n:2] & (accept[0:n:2] != accept[1:n:2])).sum())
    return out


def assert_covered(cov, tag=""):
    for parity in (0, 1):
        for what in ("accept", "refuse", "mixed"):
            assert cov[parity][what] >= 4, (tag, parity, what, cov)
    assert cov["split pairs"] >= 4, (tag, cov)


# ---- the kernels the lattice is run through ------------------------------------------------------------------------
# One entry per case of test_gpu_edge_arithmetic.test_kernel_matches_the_oracle: the LBM_* knobs that select the kernel,
# what Engine.info() must then report (`pin`: the case fails if another kernel served it), and what lbm_plan.h must decide
# beyond that (`plan`: checked without a device through tests/plan_dump.cpp, test_edge_lattice.py).
def _pin(steps_per_launch, lane_cells=0, band_rows=0, band_groups=1, resident=False, **more):
    return dict(steps_per_launch=steps_per_launch, lane_cells=lane_cells, band_rows=band_rows, band_groups=band_groups,
                resident=resident, **more)


def _kernel_cases():
    cases = []

    def add(name, env, pin, plan, shape=(256, 40), n_gpus=1, halo="none"):
        cases.append(dict(id=name, env={"LBM_" + k: str(v) for k, v in env.items()}, pin=pin, plan=plan, shape=shape,
                          n_gpus=n_gpus, halo=halo))

    # one step per pass
    for neigh in (0, 2):
        add(f"step_vec4 neigh{neigh}", dict(FUSE2=0, VEC4=1, NEIGH=neigh), _pin(1), dict(vec4=1, neigh=neigh, fuse2=0, tile_steps=0))
    add("step_scalar 130x12", dict(VEC4=0), _pin(1), dict(vec4=0, fuse2=0, tile_steps=0), shape=(130, 12))
    add("step_scalar", dict(FUSE2=0), _pin(1), dict(vec4=0, fuse2=0, tile_steps=0))
    # LDS tiles
    add("step_tile 16x8 x4", dict(TILE_STEPS=4), _pin(4), dict(tile_steps=4, tile_shape=0))
    add("step_tile 32x16 x3", dict(TILE_SHAPE=3, TILE_STEPS=3), _pin(3), dict(tile_steps=3, tile_shape=3))
    # scalar stream kernels
    scalar = dict(packed=0, tile_steps=0, fuse2=1, xcd_chunk=0)
    add("step2_stream 4 cells", dict(FUSE2=1, PACKED=0, LANE_CELLS=4, PASS_STEPS=2, BAND_ROWS=5), _pin(2, 4, 5),
        dict(scalar, use_stepk=0, prefetch=0))
    add("step2_stream 2 cells", dict(FUSE2=1, PACKED=0, LANE_CELLS=2, BAND_ROWS=3), _pin(2, 2, 3), dict(scalar, use_stepk=0))
    for k, band in ((2, 2), (3, 5), (4, 7)):
        add(f"stepk_stream K={k}", dict(FUSE2=1, PACKED=0, LANE_CELLS=4, PASS_STEPS=k, STEPK=1, BAND_ROWS=band), _pin(k, 4, band),
            dict(scalar, use_stepk=1))
    # packed stream kernels: one pair per lane, two pairs per lane
    for k in (2, 3, 4):
        add(f"stepk_pk 1 pair K={k}", dict(FUSE2=1, LANE_CELLS=2, PASS_STEPS=k, BAND_ROWS=3, LDS_WINDOWS=k % 2), _pin(k, 2, 3),
            dict(packed=1, fuse2=1, tile_steps=0, lds_windows=k % 2))
    for k in (2, 3, 4):
        for lds in (0, 1, 2):
            for prefetch in (0, 1):
                for band in (2, 7):
                    add(f"stepk_pk 2 pairs K={k} lds{lds} pf{prefetch} band{band}",
                        dict(FUSE2=1, LANE_CELLS=4, PASS_STEPS=k, LDS_WINDOWS=lds, PREFETCH=prefetch, BAND_ROWS=band), _pin(k, 4, band),
                        dict(packed=1, fuse2=1, tile_steps=0, lds_windows=lds, prefetch=prefetch))
    add("stepk_pk K=4 two band groups", dict(FUSE2=1, LANE_CELLS=4, PASS_STEPS=4, BAND_ROWS=3, GRAPH=0, BAND_GROUPS=2),
        _pin(4, 4, 3, band_groups=2), dict(packed=1, fuse2=1, tile_steps=0, use_graph=0))
    # across slabs: the lid row ny-2 is a halo row of slab 0 (two slabs) -- the redundant acceleration
    for slabs in (2, 5):
        for name, env, plan in (("packed K=3", dict(PASS_STEPS=3), dict(packed=1)), ("packed K=4", dict(PASS_STEPS=4), dict(packed=1)),
                                ("scalar K=2", dict(PACKED=0, PASS_STEPS=2), dict(packed=0, use_stepk=0))):
            add(f"{slabs} slabs {name}", dict(env, HALO="memcpy", LANE_CELLS=4, BAND_ROWS=3), _pin(env["PASS_STEPS"], 4, 3),
                dict(plan, fuse2=1), n_gpus=slabs, halo="memcpy")
    add("1 slab RCCL halo packed K=4", dict(FORCE_HALO=1, HALO="rccl", LANE_CELLS=4, PASS_STEPS=4, BAND_ROWS=3), _pin(4, 4, 3),
        dict(packed=1, fuse2=1), halo="rccl")
    # the resident kernel
    res = dict(RESIDENT_MIN_STEPS=1)
    add("resident", res, _pin(4, resident=True, resident_rows=2, resident_group=1, resident_one_xcd=1), dict(resident=1))
    for joint in (0, 1):
        add(f"resident rows4 joint{joint}", dict(res, RESIDENT_ROWS=4, RESIDENT_JOINT=joint),
            _pin(4, resident=True, resident_rows=4, resident_group=1, resident_one_xcd=0), dict(resident=1, resident_joint=joint))
    add("resident all XCDs", dict(res, RESIDENT_ONE_XCD=0), _pin(4, resident=True, resident_rows=2, resident_group=1, resident_one_xcd=0),
        dict(resident=1))
    add("resident group2", dict(res, RESIDENT_GROUP=2), _pin(4, resident=True, resident_rows=2, resident_group=2, resident_one_xcd=1),
        dict(resident=1))
    return cases


KERNEL_CASES = _kernel_cases()


def assert_pinned(info, pin, tag=""):
    """Engine.info() against a case's pin."""
    want = dict(pin)
    resident = want.pop("resident")
    assert (info["resident_steps"] > 0) == resident, (tag, info)
    for k, v in want.items():
        assert info[k] == v, (tag, k, info)
