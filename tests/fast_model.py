"""The fast-math mode (math="fast"): what one fast collision must be, and the GPU cases that hold every fast kernel to it.

TEST INFRASTRUCTURE: numpy, fractions and the oracle binding only, no GPU.  tests/test_fast_model.py checks all of this on
the CPU; tests/test_gpu_fast.py holds every fast kernel family to the oracle's fast collision bit for bit.

Two things stand behind the fast mode.

1.  oracle/lbm_oracle.c `fast_collide` restates collide<false> (lbm-asynchronous_amd/csrc/lbm_kernels.hip.h:279-306)
    operation for operation.  The library is built with -ffp-contract=off, collide<false> spells its FMAs (__fmaf_rn),
    1.f / rho is the IEEE divide and everything else is one correctly rounded fp32 operation, so a fast lattice has one
    right answer bit for bit, whichever kernel family and call splitting produced it.

2.  A restatement can share a wrong constant with what it restates.  So the restatement answers to the BGK collision in
    exact rational arithmetic first,

        R_k = t_k + omega (w_k P (1 + 3 U_k + 4.5 U_k^2 - 1.5 |U|^2) - t_k),      w = 4/9, 1/9, 1/36 (fractions),

    P = sum t_k, U = momentum / P, U_k = c_k . U, within a bound DERIVED from the expression tree, never fitted.

The bound (u = 2^-24; t_k > 0; |U| <= UMAX = 0.3; first order in u, second order covered by rounding A up)
-----------------------------------------------------------------------------------------------------------------------
Every fp32 operation returns its exact result times (1 + d), |d| <= u; fmaf(a, b, c) = (ab + c)(1 + d), one rounding.
Line numbers are those of lbm_kernels.hip.h.  q_k = 1 + 3|U_k| + 4.5 U_k^2 + 1.5|U|^2 (>= 1, >= |poly_k|).

  :284  rho: 8 additions, pairwise, of positive terms: t0..t7 pass through 4 of them, t8 through 1
            rho = P (1 + 4u)
  :285  inv = 1.f / rho, one IEEE divide                                     inv = (1 / P)(1 + 5u)
  :286  X = ((t1 + t5) + t8) - ((t3 + t6) + t7): each bracket is a sum of positive terms of depth 2, the subtraction rounds
        once.  With S = t1 + t5 + t8 + t3 + t6 + t7 <= P:  |X - M_x| <= 2u S + u |M_x| <= 3u P.  THE CANCELLATION: the
        absolute error scales with P, not with |M_x| = P |U_x|.
        ux = X * inv, one more rounding:   |ux - U_x| <= 3u + 6u |U_x| <= e = (3 + 6 UMAX) u = 4.8u      (:287 uy alike)
  :297-304  u_k: +-ux, +-uy exactly (negation), E_axis = e;  ux + uy etc.: one rounding of |U_x +- U_y| <= sqrt(2) UMAX,
        E_diag = 2e + sqrt(2) UMAX u = 10.03u
  :288  u_sq = fmaf(ux, ux, uy * uy) = (ux^2 + uy^2 (1 + d))(1 + d'):
        err(u_sq) <= 2(|U_x| + |U_y|) e + 2u |U|^2
  :289  base = fmaf(-1.5, u_sq, 1):  err(base) <= 1.5 err(u_sq) + u |1 - 1.5|U|^2| <= 1.5 err(u_sq) + u
  :293  inner = fmaf(4.5, u_k, 3):   err(inner) <= 4.5 E_k + u (3 + 4.5|U_k|)
        poly = fmaf(u_k, inner, base): err(poly) <= E_k (3 + 4.5|U_k|) + |U_k| err(inner) + err(base) + u |poly_k|
                                                 <= E_k (3 + 9|U_k|) + 1.5 err(u_sq) + 2u q_k
        (u (3|U_k| + 4.5 U_k^2) + u <= u q_k and |poly_k| <= q_k), and 3 + 9|U_k| <= 3 q_k
  :290  wr = (omega * kW) * rho: two roundings, kW within u of its fraction (test_fast_model.py checks it), rho 4u
            wr = omega w_k P (1 + 7u)
  :291  keep = 1.f - omega, exact for omega in [0.5, 2] (Sterbenz), else one rounding;  keep * t_k: one more
            keep * t_k = (1 - omega) t_k (1 + 2u)
  :294  r_k = fmaf(wr, poly, keep * t_k), one rounding of |R_k| <= omega w_k P q_k + |1 - omega| t_k:

        |r_k - R_k| <= omega w_k P [7u q_k + err(poly) + u q_k] + 3u |1 - omega| t_k
                    <= omega w_k P u [10 q_k + 3 (E_k / u) q_k + 3 sqrt(2) UMAX (e / u) + 3 |U|^2] + 3u |1 - omega| t_k

        with 1.5 * 2(|U_x| + |U_y|) e <= 3 sqrt(2) UMAX e = 6.11u and 3|U|^2 = 2 (1.5|U|^2) <= 2 (q_k - 1):

        |r_k - R_k| <= (A_k omega w_k P q_k + B |t_k|) 2^-24,     B = 3 |1 - omega|  (<= 3)
            A_axis = 12 + 6.11 + 3 * 4.8   = 32.51 -> 33
            A_diag = 12 + 6.11 + 3 * 10.03 = 48.20 -> 49
  :296  r_0 = fmaf(w0r, base, keep * t_0): no poly;  omega w_0 P [7u |base| + err(base) + u q_0] with |base| <= q_0 and
        err(base) <= 6.11u + 3u |U|^2 + u <= 6.11u + (2 q_0 - 1) u:
            A_rest = 10 + 6.11             = 16.11 -> 17

The second-order terms are below (50u)^2 = 1e-11 relative, 2e-4 u; rounding A up to the next integer adds at least 0.49u.
"""
import collections
import fractions
import functools
import math

import numpy as np

import av_model
from av_model import U, stream_env

F = fractions.Fraction
UMAX = 0.3                                  # largest |U| of the cells the bound is stated for
W_FRACTIONS = (F(4, 9),) + (F(1, 9),) * 4 + (F(1, 36),) * 4
CX = (0, 1, 0, -1, 0, 1, -1, -1, 1)
CY = (0, 0, 1, 0, -1, 1, 1, -1, -1)

_E = 3 + 6 * UMAX                           # |ux - U_x| / u
_E_DIAG = 2 * _E + math.sqrt(2) * UMAX
_CROSS = 3 * math.sqrt(2) * UMAX * _E       # 1.5 * 2 (|U_x| + |U_y|) e / u
A_REST = math.ceil(10 + _CROSS)
A_AXIS = math.ceil(12 + _CROSS + 3 * _E)
A_DIAG = math.ceil(12 + _CROSS + 3 * _E_DIAG)
A = (A_REST,) + (A_AXIS,) * 4 + (A_DIAG,) * 4


def b_of(omega):
    return 3.0 * abs(1.0 - float(omega))


# ---------------------------------------------------------------------------------------------------------------------
# the BGK collision in float64 and in rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def bgk_float64(t, omega):
    """(R, bound) for post-propagate populations t (n, 9 float32) and the fp32 omega: the BGK collision with the exact
    weights in float64, and the derived bound of |r_k - R_k| for every population.  Also returns P and the velocity."""
    t = np.asarray(t, dtype=np.float64)
    om = float(np.float32(omega))
    w = np.array([float(x) for x in W_FRACTIONS])
    P = t.sum(axis=1)
    ux = (t[:, 1] + t[:, 5] + t[:, 8] - t[:, 3] - t[:, 6] - t[:, 7]) / P
    uy = (t[:, 2] + t[:, 5] + t[:, 6] - t[:, 4] - t[:, 7] - t[:, 8]) / P
    usq = ux * ux + uy * uy
    uk = np.outer(ux, CX) + np.outer(uy, CY)
    poly = 1.0 + 3.0 * uk + 4.5 * uk * uk - 1.5 * usq[:, None]
    R = t + om * (w * P[:, None] * poly - t)
    q = 1.0 + 3.0 * np.abs(uk) + 4.5 * uk * uk + 1.5 * usq[:, None]
    bound = (np.array(A, dtype=np.float64) * om * w * P[:, None] * q + b_of(om) * np.abs(t)) * U
    return R, bound, P, ux, uy


def bgk_fraction(t, omega):
    """The same collision of ONE cell (9 float32) in exact rational arithmetic: list of 9 Fractions."""
    t = [F(float(x)) for x in t]
    om = F(float(np.float32(omega)))
    P = sum(t)
    ux = (t[1] + t[5] + t[8] - t[3] - t[6] - t[7]) / P
    uy = (t[2] + t[5] + t[6] - t[4] - t[7] - t[8]) / P
    usq = ux * ux + uy * uy
    out = []
    for k in range(9):
        uk = CX[k] * ux + CY[k] * uy
        out.append(t[k] + om * (W_FRACTIONS[k] * P * (1 + 3 * uk + F(9, 2) * uk * uk - F(3, 2) * usq) - t[k]))
    return out


def round_to_float32(x):
    """The fp32 nearest to the Fraction x, ties to even (normal range)."""
    if x == 0:
        return np.float32(0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if F(2) ** e > a:
        e -= 1
    assert F(2) ** e <= a < F(2) ** (e + 1) and -126 <= e <= 127
    scaled = a / F(2) ** (e - 23)                       # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > F(1, 2) or (rem == F(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(s * float(n) * 2.0 ** (e - 23))


# ---------------------------------------------------------------------------------------------------------------------
# the cells the collision is checked on
# ---------------------------------------------------------------------------------------------------------------------
def collision_cells(seed=20241, n=6000):
    """n seeded cells of post-propagate populations (n, 9 float32), all positive: densities log-uniform over two decades
    around 0.1; velocities at rest exactly, slow, and with |U| in [0.1, 0.3] (a third of the cells); populations within
    5 % of the equilibrium, except two kinds that are far from it: the rest population holding 97 % of the density, and
    an opposite pair (1 and 3, or 2 and 4, or a diagonal pair) holding 90 % of it, where the momentum numerators cancel
    two numbers of the size of the density."""
    rng = np.random.default_rng(seed)
    w = np.array([float(x) for x in W_FRACTIONS])
    rho = 10.0 ** rng.uniform(-2.0, 0.0, n)
    kind = rng.integers(0, 6, n)                         # 0 rest, 1 slow, 2-3 fast, 4 rest population, 5 opposite pair
    speed = np.where(kind == 0, 0.0, np.where(kind == 1, rng.uniform(0.0, 0.1, n), rng.uniform(0.1, 0.27, n)))
    angle = rng.uniform(0.0, 2.0 * np.pi, n)
    ux, uy = speed * np.cos(angle), speed * np.sin(angle)
    uk = np.outer(ux, CX) + np.outer(uy, CY)
    feq = w * rho[:, None] * (1.0 + 3.0 * uk + 4.5 * uk * uk - 1.5 * (ux * ux + uy * uy)[:, None])
    t = feq * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (n, 9)))
    # at rest exactly: opposite populations equal
    rest = kind == 0
    for a, b in ((3, 1), (4, 2), (7, 5), (8, 6)):
        t[rest, a] = t[rest, b]
    t[rest, 6] = t[rest, 5]
    t[rest, 8] = t[rest, 5]
    t[rest, 7] = t[rest, 5]
    # the rest population dominating
    dom = kind == 4
    small = rho[dom, None] * 0.03 / 8.0 * rng.uniform(0.5, 1.5, (int(dom.sum()), 8))
    t[dom, 1:] = small
    t[dom, 0] = 0.97 * rho[dom]
    # an opposite pair dominating, nearly balanced
    idx = np.nonzero(kind == 5)[0]
    pairs = ((1, 3), (2, 4), (5, 7), (6, 8))
    for i in idx:
        a, b = pairs[rng.integers(0, 4)]
        t[i] = rho[i] * 0.1 / 7.0 * rng.uniform(0.5, 1.5, 9)
        tilt = rng.uniform(-0.2, 0.2)
        t[i, a] = rho[i] * 0.45 * (1.0 + tilt)
        t[i, b] = rho[i] * 0.45 * (1.0 - tilt)
    t = t.astype(np.float32)
    assert (t > 0).all()
    return np.ascontiguousarray(t), kind


OMEGAS = (1.85, 0.6, 1.2)


# ---------------------------------------------------------------------------------------------------------------------
# the fast dispatch tables, as data
# ---------------------------------------------------------------------------------------------------------------------
# Every row a context created with math="fast" can select, read from lbm-asynchronous_amd/csrc/lbm_hip.hip.
FAST_DISPATCH = {
    # launch_step, :620-628: table[1][neigh][nts]
    "step_vec4": ([("step_vec4", neigh, nts) for neigh in (0, 1, 2) for nts in (0, 1)], "lbm_hip.hip:624-626, 628"),
    # launch_step, :631: exact ? step_scalar<true> : step_scalar<false>
    "step_scalar": ([("step_scalar",)], "lbm_hip.hip:631"),
    # launch_step2, :662-667: table[1][nts][lane_cells == 2]
    "step2_stream": ([("step2_stream", nts, c) for nts in (0, 1) for c in (4, 2)], "lbm_hip.hip:665-667"),
    # launch_stepk, :706-709, :732: table[1][nts][k - 2][prefetch]; K = 4 with prefetch is the kernel without it (:708)
    "stepk_stream": ([("stepk_stream", nts, k, pf) for nts in (0, 1) for k, pf in ((2, 0), (2, 1), (3, 0), (3, 1), (4, 0))],
                     "lbm_hip.hip:706-709, 732"),
    # launch_tile, :282-287, :766: kTileKernels[shape].fast
    "step_tile": ([("step_tile", shape) for shape in range(7)], "lbm_hip.hip:282-287, 766"),
}
ALL_ROWS = [row for rows, _ in FAST_DISPATCH.values() for row in rows]


def planned_rows(plan, halo=False):
    """The dispatch rows a context with this lbm_plan::KernelPlan (tests/plan_tool.py) launches in fast mode, first the
    one its full passes run: run_passes (lbm_hip.hip:1609-1612) takes tile_steps per launch on a periodic slab, else
    pass_steps per pass while that many remain, two for a remainder of two or three, one for the odd last step;
    launch_pass (:738-744) sends a pass to stepk_stream or step2_stream; launch_step (:616-634) is step_vec4 or
    step_scalar.  The packed kernels (plan.packed) are exact and are no row of these tables."""
    one = ("step_vec4", plan["neigh"], plan["nts"]) if plan["vec4"] else ("step_scalar",)
    if plan["tile_steps"] and not halo:
        return [("step_tile", plan["tile_shape"])]
    if not plan["fuse2"]:
        return [one]
    assert not plan["packed"], "a packed plan runs the exact kernels"
    rows = []
    for k in sorted({plan["pass_steps"], 2}, reverse=True):
        stepk = plan["lane_cells"] == 4 and (k > 2 or plan["prefetch"] or plan["xcd_chunk"] or plan["use_stepk"])
        if stepk:
            rows.append(("stepk_stream", plan["nts"], k, 1 if (plan["prefetch"] and k < 4) else 0))
        else:
            rows.append(("step2_stream", plan["nts"], plan["lane_cells"]))
    return rows + [one]


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_fast.py
# ---------------------------------------------------------------------------------------------------------------------
class Case(av_model.Case):
    """An av_model.Case run with math="fast".  row: the row of FAST_DISPATCH the case is about (asserted against the
    planner on the CPU, against Engine.info() on the GPU)."""

    def __init__(self, family, nx, ny, env, expect, row, **kw):
        super().__init__(family, nx, ny, env, expect, "fast", **kw)
        self.row = row
        self.id = "fast-" + self.id

    def bound(self, info=None):
        return av_model.bound(info if info is not None else self.expect, self.tile, self.packed, fast=True)


def _cases():
    out = []
    one = {"steps_per_launch": 1}
    # step_vec4<1, NEIGH, NTS>: every flavour
    for neigh in (0, 1, 2):
        for nts in (0, 1):
            env = {"LBM_FUSE2": "0", "LBM_VEC4": "1", "LBM_NEIGH": str(neigh), "LBM_NTS": str(nts)}
            out.append(Case("step_vec4", 320, 12, env, {**one, "nontemporal": nts}, ("step_vec4", neigh, nts)))
    # step_scalar<false>: more than one workgroup with a ragged last one; two grids smaller than a workgroup
    for nx, ny in ((130, 9), (7, 6), (3, 2)):
        out.append(Case("step_scalar", nx, ny, {"LBM_FUSE2": "0"}, one, ("step_scalar",)))
    # step_tile, shapes 0 and 3: 96x40 (the top row of 32x16 tiles is cut) and 33x19 (both edges cut through tiles)
    for nx, ny in ((96, 40), (33, 19)):
        for env, k, shape in (({"LBM_TILE_STEPS": "4"}, 4, 0), ({"LBM_TILE_STEPS": "1"}, 1, 0),
                              ({"LBM_TILE_STEPS": "3", "LBM_TILE_SHAPE": "3"}, 3, 3)):
            out.append(Case("step_tile", nx, ny, env, {"steps_per_launch": k}, ("step_tile", shape), tile=shape))
    # the other five tile shapes on 200x51: no tile width or height divides the grid
    for shape, k in ((1, 8), (2, 2), (4, 4), (5, 2), (6, 1)):
        env = {"LBM_TILE_SHAPE": str(shape), "LBM_TILE_STEPS": str(k)}
        out.append(Case("step_tile", 200, 51, env, {"steps_per_launch": k}, ("step_tile", shape), tile=shape))
    # the default fast path of a single-slab grid below 300 Ki cells that is not resident-shaped: nothing forced
    out.append(Case("default", 200, 51, {}, {"steps_per_launch": 4}, ("step_tile", 0), tile=0))
    # step2_stream<1, NTS, C>
    for lc in (4, 2):
        for nts in (0, 1):
            env = {**stream_env(2, 5, stepk=0, packed=0, lane_cells=lc), "LBM_NTS": str(nts)}
            out.append(Case("step2_stream", 320, 24, env,
                            {"steps_per_launch": 2, "band_rows": 5, "lane_cells": lc, "nontemporal": nts},
                            ("step2_stream", nts, lc), packed=False))
    # stepk_stream<1, NTS, 4, K, PF>: strips 248 + 248 + 16
    for k in (2, 3, 4):
        for band in (3, 7):
            for pf in (0, 1):
                for nts in ((0, 1) if band == 3 else (0,)):
                    env = {**stream_env(k, band, prefetch=pf, packed=0), "LBM_NTS": str(nts)}
                    out.append(Case("stepk_stream", 512, 20, env,
                                    {"steps_per_launch": k, "band_rows": band, "lane_cells": 4, "nontemporal": nts},
                                    ("stepk_stream", nts, k, pf if k < 4 else 0), packed=False))
    # three slabs with device-copy halos: K = 3 passes with boundary bands, and the one-step kernel on boundary rows
    halo = {"LBM_HALO": "memcpy"}
    out.append(Case("slabs", 512, 24, {**stream_env(3, 5, prefetch=1, packed=0), **halo},
                    {"steps_per_launch": 3, "band_rows": 5, "lane_cells": 4}, ("stepk_stream", 0, 3, 1), slabs=3,
                    packed=False))
    out.append(Case("slabs", 512, 23, {"LBM_FUSE2": "0", **halo}, one, ("step_vec4", 0, 0), slabs=3))
    # graph replay of the one-step fast kernel: a chunk of 64 steps replayed inside the first and the last call
    out.append(Case("graph", 192, 40, {"LBM_GRAPH": "1", "LBM_FUSE2": "0"}, {**one, "graph_steps": 64}, ("step_scalar",),
                    calls=((70, 1, 64),)))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), "case ids must be unique"
    return out


CASES = _cases()

# the default packed plan in fast mode (tests/test_gpu_fast.py): the packed kernels are exact, the odd step is not
PACKED_SHAPE = (512, 20)
PACKED_ENV = stream_env(4, 5, prefetch=1, packed=12)
PACKED_EXPECT = {"steps_per_launch": 4, "band_rows": 5, "lane_cells": 4}

FastModel = collections.namedtuple("FastModel", "cells usq")


@functools.lru_cache(maxsize=None)
def model(nx, ny, steps):
    """The oracle's fast run of the shape's lattice (av_model.lattice): final cells and the per-step u_sq maps, computed
    once per (shape, steps) and never changed."""
    import oracle_binding
    p, ob, cells = av_model.lattice(nx, ny)
    cur = cells.copy()
    usq = oracle_binding.load().run_fast(p, cur, ob, steps, want_usq=True)
    cur.setflags(write=False)
    usq.setflags(write=False)
    return FastModel(cur, usq)


def want_av(usq_map, ob):
    """float64 mean over the fluid cells of sqrt(u_sq)."""
    fluid = ob == 0
    return float(np.sqrt(usq_map[fluid].astype(np.float64)).sum()) / float(fluid.sum())
