"""What av_vels must be, per kernel family, and how far the fp32 sums inside a partial may move it.

TEST INFRASTRUCTURE: numpy and the oracle binding only, no GPU.  tests/test_av_model.py checks the model on the CPU,
tests/test_gpu_av_vels.py holds every kernel family to it.

The value a kernel adds per fluid cell is known almost exactly:

* SPEED = 0 kernels (step_vec4, step_scalar, step_tile) take |u| from the relaxed populations with the IEEE sqrt
  (collide_exact<0>, lbm_kernels.hip.h:262-266): bit-identical to the oracle's final_state `u`   -> the `relaxed` map.
* SPEED = 1 kernels (step2_stream, stepk_stream, stepk_pk, resident_band; LBM_STREAM_SPEED = 1, :246-248) take
  v_sqrt_f32(ux*ux + uy*uy) of the PRE-collision moments (:256, :268; relax_pair_core :978-979), i.e. of the
  post-propagate populations.  ux and uy are the correctly rounded quotients of moments_shared, the same bits as
  moments_exact's, the sum is unfused and the native sqrt is within 1 ulp                          -> the `moment` map.

What remains is the fp32 summation inside a partial: for non-negative terms it is bounded by the number of fp32
additions a term passes through, whatever their order (each addition multiplies what it carries by 1 + d, |d| <= 2^-24).
The partials are widened to double before they meet (reduce_partials :2536, reduce_band_partials_at :2316); those
additions (2^-53 each) and the second-order terms of the fp32 ones are below 1e-6 of the bound and are not counted.
"""
import collections
import ctypes
import functools

import numpy as np

U = 2.0 ** -24           # unit roundoff of fp32
ULP = 2.0 ** -23         # one ulp of fp32, relative, at most

# ---------------------------------------------------------------------------------------------------------------------
# the model: per-cell |u| of every step
# ---------------------------------------------------------------------------------------------------------------------
Speeds = collections.namedtuple("Speeds", "relaxed moment cells rho_min rho_max usq_max")


def moment_speed(f, ob):
    """|u| of the populations `f` (ny, nx, 9 float32) in moments_exact's expression order (lbm_kernels.hip.h:103-110):
    every operation a single IEEE fp32 one (numpy does not contract), IEEE divide and sqrt.  Blocked cells are 0.
    Also returns the density and |u|^2 maps."""
    f = [np.ascontiguousarray(f[..., k]) for k in range(9)]
    d = f[0]
    for k in range(1, 9):
        d = d + f[k]
    with np.errstate(all="ignore"):
        ux = (f[1] + f[5] + f[8] - (f[3] + f[6] + f[7])) / d
        uy = (f[2] + f[5] + f[6] - (f[4] + f[7] + f[8])) / d
        usq = ux * ux + uy * uy
        speed = np.sqrt(usq)
    assert speed.dtype == np.float32
    return np.where(ob != 0, np.float32(0), speed), d, usq


def step_speeds(oracle, p, ob, cells, steps):
    """Advance a copy of `cells` through the oracle's four sweeps.  Per step two (ny, nx) float32 maps: `relaxed`
    (final_state's u of the step's result) and `moment` (moment_speed of the post-propagate populations); the final
    lattice; and the extremes of the fluid cells' density (before and after the collision) and |u|^2 over the run."""
    lib = oracle.lib
    ob = np.ascontiguousarray(ob, dtype=np.int32)
    cur, tmp = cells.copy(), np.empty_like(cells)
    cp = ctypes.byref(oracle.cparams(p))
    fluid = ob == 0
    relaxed, moment = [], []
    rho_min, rho_max, usq_max = np.inf, 0.0, 0.0
    for _ in range(steps):
        lib.lbm_oracle_accelerate_flow(cp, cur.ctypes.data, ob.ctypes.data)
        lib.lbm_oracle_propagate(cp, cur.ctypes.data, tmp.ctypes.data)
        m, rho, usq = moment_speed(tmp, ob)
        lib.lbm_oracle_rebound(cp, cur.ctypes.data, tmp.ctypes.data, ob.ctypes.data)
        lib.lbm_oracle_collision(cp, cur.ctypes.data, tmp.ctypes.data, ob.ctypes.data)
        r, rho2, usq2 = moment_speed(cur, ob)
        u = oracle.final_state(p, cur, ob)["u"]
        assert np.array_equal(u.view(np.uint32), r.view(np.uint32)), "moment_speed is not final_state's arithmetic"
        for a in (rho, rho2):
            rho_min, rho_max = min(rho_min, float(a[fluid].min())), max(rho_max, float(a[fluid].max()))
        usq_max = max(usq_max, float(usq[fluid].max()), float(usq2[fluid].max()))
        relaxed.append(u)
        moment.append(m)
    for a in (cur, *relaxed, *moment):
        a.setflags(write=False)
    return Speeds(relaxed, moment, cur, rho_min, rho_max, usq_max)


def want_av(speed_map, ob):
    """float64 sum over the fluid cells divided by the float64 cell count."""
    fluid = ob == 0
    return float(speed_map[fluid].astype(np.float64).sum()) / float(fluid.sum())


def weights(speed_map, ob):
    """Each cell's share of the step's sum (blocked cells 0)."""
    w = np.where(ob == 0, speed_map.astype(np.float64), 0.0)
    return w / w.sum()


# ---------------------------------------------------------------------------------------------------------------------
# depth: the most fp32 additions a cell's |u| passes through before it is widened to double
# ---------------------------------------------------------------------------------------------------------------------
# Read from lbm-asynchronous_amd/csrc/lbm_kernels.hip.h (and lbm_plan.h / lbm_hip.hip for the geometry), never fitted.
# An addition to an accumulator that still holds 0 is exact but is counted all the same: depth is an upper bound.
WAVE_TREE = 6     # wave_sum :325-329 (six __shfl_down levels) and wave_sum_dpp :1726-1734 (six DPP levels)
ROW16_TREE = 4    # row16_sum_dpp :1696-1702: four DPP levels over the <= 16 waves of a band
BLOCK_WAVES = 4   # block_sum<256> :338-342: thread 0 adds the kBlock / 64 = 4 wave partials one after the other

# step_tile instantiations (lbm_plan.h:24-32): (tw, th, kmax, threads).  A thread adds at most MAXC own cells
# (lbm_kernels.hip.h:1410 MAXC, :1437-1454 my_sum), then block_sum<THREADS>: the wave tree and THREADS / 64 wave partials.
TILE_DIMS = ((16, 8, 4, 384), (16, 8, 8, 768), (32, 16, 2, 640), (32, 16, 3, 768), (32, 16, 4, 896), (64, 16, 2, 640),
             (64, 8, 2, 704))


def _tile_depth(tw, th, kmax, threads):
    maxc = -(-((tw + 2 * kmax - 2) * (th + 2 * kmax - 2)) // threads)
    return maxc + WAVE_TREE + threads // 64


DEPTH_TABLE = {
    # family: (depth as a function of the geometry, where it was read)
    "step_vec4": (lambda g: 4 + WAVE_TREE + BLOCK_WAVES,
                  "lbm_kernels.hip.h:465-476 my_sum += speed over the lane's 4 cells; :492 block_sum<256>"),
    "step_scalar": (lambda g: 1 + WAVE_TREE + BLOCK_WAVES,
                    "lbm_kernels.hip.h:2359 my_sum = speed (one cell, counted as one); :2366 block_sum<256>"),
    "step_tile": (lambda g: max(_tile_depth(*d) for d in (TILE_DIMS if g.get("shape") is None else [TILE_DIMS[g["shape"]]])),
                  "lbm_kernels.hip.h:1437-1454 my_sum over <= MAXC cells; :1468 block_sum<THREADS>; info() does not "
                  "report the tile shape (LBM_TILE_SHAPE; default lbm_plan.h:412: 0 up to 200 Ki cells, else 3): the "
                  "caller's, or the largest of lbm_plan.h:24-32 (32x16 kmax 4: 1 + 6 + 14)"),
    "scalar_stream": (lambda g: g["rows"] * g["lane_cells"] + WAVE_TREE,
                      "lbm_kernels.hip.h:653,686 (step2_stream) / :853,891 (stepk_stream) sum[s] += speed per cell, "
                      "C cells per row over the band's rows; :711-712 / :926 wave_sum"),
    "stepk_pk": (lambda g: (1 if g["lane_cells"] == 2 else 2) + g["rows"] + WAVE_TREE,
                 "lbm_kernels.hip.h:1080 sp0 + sp1 (pair), :1216-1217 s0 + pair (two pairs per lane); "
                 ":1285,1327 sum[s] += sp once per row of the band; :1375 wave_sum"),
    "resident_band": (lambda g: 2 + WAVE_TREE + ROW16_TREE,
                      "lbm_kernels.hip.h:1673 sp0 + sp1 (pair), :2249 sum += edge pair (or :1714 the joint form: two "
                      "levels as well); :2271 wave_sum_dpp; :2133,2297 row16_sum_dpp over the band's waves"),
}

# roundings lbm_read_av_vels applies after the double total (lbm_hip.hip:3092): (float)total, then the fp32 division by
# (float)fluid_cells (exact below 2^24 cells)
READ_ROUNDINGS = 2


def families(info, tile=None):
    """The kernel families an engine with this Engine.info() launches, with the geometry depth needs.  `tile`: whether
    the LDS-tile kernel runs the passes -- info() shows it only through steps_per_launch > 1 without a stream kernel, so
    a caller that asked for LBM_TILE_STEPS=1 says so: True, or the index of the tile shape it knows to be planned."""
    k = info["steps_per_launch"]
    out = []
    if info.get("resident_steps", 0) > 0:
        out.append(("resident_band", {}))          # calls of at least resident_min_steps; shorter ones: the plan below
        if info.get("resident_min_steps", 0) <= 1:
            return out                              # every call is resident (lbm_hip.hip:1636)
    if info["lane_cells"] > 0:                      # a stream kernel (lbm_hip.hip:2573-2575)
        # rows a lane accumulates over: the band height; the 2K-row seam bands of a grouped pass (lbm_hip.hip:1127);
        # the K-row boundary bands of a slab with halos (:1037)
        rows = max(info["band_rows"], 2 * k if info.get("band_groups", 1) > 1 else k)
        geom = {"rows": rows, "lane_cells": info["lane_cells"]}
        # which stream kernel (lbm_hip.hip:719-721, 729-732) is the plan's LBM_PACKED, which info() does not report:
        # take the deeper of the two
        out.append(("scalar_stream", geom))
        out.append(("stepk_pk", geom))
        out.append(("step_vec4", {}))               # the odd last step of a call (lbm_hip.hip:1598, 1014)
    elif tile is not False and (tile is not None or k > 1):
        out.append(("step_tile", {"shape": None if tile is None or tile is True else int(tile)}))
    else:
        out.append(("step_vec4", {}))               # or step_scalar, which is shallower; info() does not tell them apart
    return out


def depth(info, tile=None, packed=None):
    """Largest number of fp32 additions a cell's |u| passes through before the value is widened to double, over the
    kernel families this engine launches.  `packed` (True / False): the caller knows which stream kernel was asked for."""
    fams = families(info, tile)
    if packed is not None:
        fams = [f for f in fams if f[0] != ("scalar_stream" if packed else "stepk_pk")]
    return max(DEPTH_TABLE[name][0](geom) for name, geom in fams)


def speed_mode(info, tile=None, fast=False):
    """s of bound(): 1 where the engine's long passes run a SPEED = 1 kernel (stream kernels, resident_band).
    fast: the engine was created with math="fast" and runs the scalar fast kernels, whose collide<false> takes |u| from
    the pre-collision moments with the native sqrt in EVERY family (lbm_kernels.hip.h:305): s = 1 also for step_vec4,
    step_scalar and step_tile."""
    return 1 if (fast or info["lane_cells"] > 0 or info.get("resident_steps", 0) > 0) else 0


def bound(info, tile=None, packed=None, fast=False):
    """Relative bound of |av_vels[t] - want_av(map_t)|: (depth + R) 2^-24 + s 2^-23.  The sums are the same code in
    both math modes, so depth does not depend on `fast`; s does (speed_mode)."""
    return (depth(info, tile, packed) + READ_ROUNDINGS) * U + speed_mode(info, tile, fast) * ULP


# absolute allowance on av_vels[t]: cells whose u_sq is below FLT_MIN (|u| < 2^-63) may be flushed by the native sqrt;
# n_fluid 2^-63 on the total is 2^-63 on the mean
FLUSH_ALLOWANCE = 2.0 ** -63


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_av_vels.py, shared with the coverage check of tests/test_av_model.py
# ---------------------------------------------------------------------------------------------------------------------
def stream_env(k, band, prefetch=0, chunk=0, stepk=1, packed=None, lane_cells=4):
    """The knobs of test_gpu_stream_k.force_stream as a dict."""
    env = {"LBM_FUSE2": "1", "LBM_LANE_CELLS": str(lane_cells), "LBM_PASS_STEPS": str(k), "LBM_BAND_ROWS": str(band),
           "LBM_PREFETCH": str(prefetch), "LBM_XCD_CHUNK": str(chunk), "LBM_STEPK": str(stepk)}
    if packed is not None:
        env["LBM_PACKED"] = "1" if packed else "0"
        env["LBM_LDS_WINDOWS"] = str(packed % 10 if packed > 1 else 0)
    return env


class Case:
    """One engine configuration.  expect: the Engine.info() entries that show the kernel was selected (asserted on the
    GPU; the CPU coverage check takes its bound from them).  period: the step-index modulus after which a kernel's
    per-step slots repeat (K of a K-step pass; the resident kernel's two wave_part slots)."""

    def __init__(self, family, nx, ny, env, expect, speed, calls=((13,), (1, 2, 5, 5)), slabs=1, rank=False, tile=None,
                 packed=None, period=None, reference=False, label=""):
        # tile: the tile shape planned (lbm_plan.h:412-416: shape 0 up to 200 Ki cells unless LBM_TILE_SHAPE says otherwise)
        self.family, self.nx, self.ny, self.env, self.speed = family, nx, ny, dict(env), speed
        self.expect = {"lane_cells": 0, "band_rows": 0, "band_groups": 1, "resident_steps": 0, "resident_min_steps": 0,
                       **expect}
        self.calls, self.slabs, self.rank, self.tile, self.packed, self.reference = calls, slabs, rank, tile, packed, reference
        self.period = period if period is not None else self.expect["steps_per_launch"]
        self.steps = sum(calls[0])
        assert all(sum(c) == self.steps for c in calls)
        short = {"LBM_PASS_STEPS": "K", "LBM_BAND_ROWS": "band", "LBM_LANE_CELLS": "C", "LBM_LDS_WINDOWS": "LW",
                 "LBM_PREFETCH": "PF", "LBM_BAND_GROUPS": "G"}
        quiet = ("LBM_FUSE2", "LBM_XCD_CHUNK", "LBM_STEPK", "LBM_PACKED") if "LBM_PASS_STEPS" in self.env else ()
        knobs = " ".join(f"{short.get(k, k[4:])}={v}" for k, v in sorted(self.env.items()) if k not in quiet)
        self.id = f"{family}-{nx}x{ny}" + (f"-{slabs}slabs" if slabs > 1 else "") + (f"-{label}" if label else "") + \
                  (f"[{knobs}]" if knobs else "")

    def bound(self, info=None):
        return bound(info if info is not None else self.expect, self.tile, self.packed)


def _cases():
    out = []
    one = {"steps_per_launch": 1}
    # one-step kernels.  On grids this small the planner takes one cell per lane unless LBM_VEC4 says otherwise
    out.append(Case("step_vec4", 320, 12, {"LBM_FUSE2": "0", "LBM_VEC4": "1"}, one, "relaxed"))
    out.append(Case("step_scalar", 130, 9, {"LBM_FUSE2": "0"}, one, "relaxed"))
    # LDS tiles.  96x40: the top row of 32x16 tiles is cut (40 = 16 + 16 + 8); 33x19: both edges cut through tiles and
    # the grid is smaller than one staged tile
    for nx, ny in ((96, 40), (33, 19)):
        for env, k, shape in (({"LBM_TILE_STEPS": "4"}, 4, 0), ({"LBM_TILE_STEPS": "1"}, 1, 0),
                              ({"LBM_TILE_STEPS": "3", "LBM_TILE_SHAPE": "3"}, 3, 3)):
            out.append(Case("step_tile", nx, ny, env, {"steps_per_launch": k}, "relaxed", tile=shape))
    # step2_stream: the scalar two-step kernel, four and two cells per lane (strips of 248 / 124 cells)
    for lc in (4, 2):
        out.append(Case("step2_stream", 320, 24, stream_env(2, 5, stepk=0, packed=0, lane_cells=lc),
                        {"steps_per_launch": 2, "band_rows": 5, "lane_cells": lc}, "moment", packed=False))
    # stepk_stream: strips 248 + 248 + 16
    for k in (2, 3, 4):
        for band in (3, 7):
            out.append(Case("stepk_stream", 512, 20, stream_env(k, band, packed=0),
                            {"steps_per_launch": k, "band_rows": band, "lane_cells": 4}, "moment", packed=False))
    # stepk_pk, one pair per lane: strips 120 + 120 + 16 beyond two steps (two halo lanes per side), 124 + 124 + 8 at two
    for k in (2, 3, 4):
        for lw in (0, 1):
            env = {**stream_env(k, 5, packed=1, lane_cells=2), "LBM_LDS_WINDOWS": str(lw)}
            out.append(Case("stepk_pk1", 256, 24, env, {"steps_per_launch": k, "band_rows": 5, "lane_cells": 2}, "moment",
                            packed=True))
    # stepk_pk, two pairs per lane
    for nx, ny in ((320, 24), (512, 20)):
        for lw in (0, 1, 2):
            for pf in (0, 1):
                out.append(Case("stepk_pk2", nx, ny, stream_env(4, 5, prefetch=pf, packed=(1 if lw == 0 else 10 + lw)),
                                {"steps_per_launch": 4, "band_rows": 5, "lane_cells": 4}, "moment", packed=True))
    # three slabs with device-copy halos.  23 rows over three slabs leave slabs of 7 rows, too thin for four-step passes
    # (lbm_plan.h:241-242: a K-step pass needs slabs of 2K rows): the request runs two-step passes of the packed kernel.
    # 24 rows (slabs of 8) run the four-step passes asked for.
    halo = {"LBM_HALO": "memcpy"}
    out.append(Case("slabs", 512, 23, {**stream_env(4, 5, prefetch=1, packed=12), **halo},
                    {"steps_per_launch": 2, "band_rows": 5, "lane_cells": 4}, "moment", slabs=3, packed=True))
    out.append(Case("slabs", 512, 24, {**stream_env(4, 5, prefetch=1, packed=12), **halo},
                    {"steps_per_launch": 4, "band_rows": 5, "lane_cells": 4}, "moment", slabs=3, packed=True))
    out.append(Case("slabs", 512, 23, {"LBM_FUSE2": "0", **halo}, one, "relaxed", slabs=3))
    # the rank API, a world of one whose halo rows travel through RCCL to itself
    out.append(Case("rank", 256, 24, {**stream_env(3, 5, prefetch=1), "LBM_FORCE_HALO": "1"},
                    {"steps_per_launch": 3, "band_rows": 5, "lane_cells": 4}, "moment", rank=True))
    # band groups: interiors and 2K-row seam bands of one pass write disjoint ranges of the pass's slots
    for g in (2, 3):
        for band in (5, 7):
            env = {**stream_env(4, band, prefetch=1, packed=12), "LBM_GRAPH": "0", "LBM_BAND_GROUPS": str(g)}
            out.append(Case("band_groups", 256, 128, env,
                            {"steps_per_launch": 4, "band_rows": band, "lane_cells": 4, "band_groups": g}, "moment",
                            calls=((27,), (1, 2, 5, 19)), packed=True))
    # graph replay: chunks of 64 steps and their reduce as one graph; the 64-slot ring wraps inside the first call
    out.append(Case("graph", 192, 40, {"LBM_GRAPH": "1"}, {"steps_per_launch": 4, "graph_steps": 64}, "relaxed",
                    calls=((70, 1, 64),), tile=0))
    # resident_band, every call resident
    res = {"LBM_RESIDENT_MIN_STEPS": "1"}
    for nx, ny, env, more in ((64, 8, {}, {}), (128, 16, {}, {}), (320, 24, {"LBM_RESIDENT_JOINT": "0"}, {}),
                              (320, 24, {"LBM_RESIDENT_JOINT": "1"}, {}),
                              (128, 64, {"LBM_RESIDENT_GROUP": "2"}, {"resident_group": 2}),
                              (128, 128, {"LBM_RESIDENT_ROWS": "4"}, {"resident_rows": 4}),
                              (128, 128, {"LBM_RESIDENT_ONE_XCD": "0"}, {"resident_one_xcd": 0})):
        out.append(Case("resident_band", nx, ny, {**res, **env},
                        {"steps_per_launch": 4, "resident_steps": 4096, "resident_min_steps": 1, **more}, "moment", period=2))
    # the ring of 64 partial slots: one call that drains it more than twice.  (LBM_RESIDENT=0: by default a call this
    # long on this grid runs the resident kernel, which has no ring)
    out.append(Case("ring", 256, 24, {"LBM_RESIDENT": "0"}, {"steps_per_launch": 4}, "relaxed", calls=((140,),), tile=0,
                    label="tile"))
    out.append(Case("ring", 256, 24, stream_env(4, 5, prefetch=1, packed=12),
                    {"steps_per_launch": 4, "band_rows": 5, "lane_cells": 4}, "moment", calls=((140,),), packed=True,
                    label="pk"))
    # the reference's own start (fluid at rest: |u| ~ 1e-5 in the first steps) on 128x256; tile kernel / resident kernel
    out.append(Case("reference", 128, 256, {"LBM_RESIDENT": "0"}, {"steps_per_launch": 4}, "relaxed", calls=((40,),),
                    tile=0, reference=True))
    # (resident from 8 steps per call on this grid, lbm_plan.h:473; shorter calls would run the tile kernel)
    out.append(Case("reference", 128, 256, {"LBM_RESIDENT": "1"},
                    {"steps_per_launch": 4, "resident_steps": 4096, "resident_min_steps": 8},
                    "moment", calls=((40,),), tile=0, reference=True, period=2))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), "case ids must be unique"
    return out


CASES = _cases()
DEPTH_MAX = 40      # every case keeps depth <= 40, so that one cell's weight stays above 8 x bound (test_av_model.py)


def seed_of(nx, ny):
    return 5000 + nx + ny


@functools.lru_cache(maxsize=None)
def lattice(nx, ny):
    """(Params, obstacles, cells) of the random lattice every case of this shape starts from: no side walls, so both
    wraps are live, and a blocked cell on the lid row."""
    import conftest
    from test_gpu_parity import random_case
    p, ob, cells = random_case(conftest.load_package(), nx, ny, seed_of(nx, ny), walls=False)
    ob.setflags(write=False)
    cells.setflags(write=False)
    return p, ob, cells


@functools.lru_cache(maxsize=None)
def reference_lattice(name="128x256"):
    import conftest
    import oracle_binding
    p, ob = conftest.dataset(name)
    cells = oracle_binding.load().init_cells(p)
    ob.setflags(write=False)
    cells.setflags(write=False)
    return p, ob, cells


@functools.lru_cache(maxsize=None)
def model(nx, ny, steps, reference=False):
    """step_speeds of the shape's lattice, computed once per (shape, steps) and never changed."""
    import oracle_binding
    p, ob, cells = reference_lattice() if reference else lattice(nx, ny)
    return step_speeds(oracle_binding.load(), p, ob, cells, steps)


def case_inputs(case):
    return reference_lattice() if case.reference else lattice(case.nx, case.ny)


def case_model(case):
    return model(case.nx, case.ny, case.steps, case.reference)
