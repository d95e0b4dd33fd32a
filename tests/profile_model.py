"""The line profiles of include/lbm_hip.h (lbm_set_profiles) in numpy float32, for the tests: per cell the moments of
tests/stats_model.py (every operation rounded to float32, none contracted), per line the sums exact (math.fsum: the
correctly rounded sum of the exact terms) over the line's finite fluid cells, and the two counts."""
import math

import numpy as np

import stats_model

SUMS = ("sum_rho", "sum_jx", "sum_jy", "sum_ux", "sum_uy")
FIELDS = SUMS + ("fluid", "nonfinite")


def line(values, counted, fluid):
    """one line: values = the five float32 vectors of the line's cells, counted / fluid = bool vectors"""
    out = {k: math.fsum(v[counted].astype(np.float64).tolist()) for k, v in zip(SUMS, values)}
    out["fluid"] = int(counted.sum())
    out["nonfinite"] = int((fluid & ~counted).sum())
    return out


def record(cells_aos, obstacles):
    """{"rows": [ny lines], "columns": [nx lines]} of one lattice, a line being {field: value}"""
    ob = np.asarray(obstacles) != 0
    rho, jx, jy, ux, uy, usq, _ = stats_model.moments(np.asarray(cells_aos, dtype=np.float32).reshape(ob.shape + (9,)))
    fluid = ~ob
    counted = fluid & np.isfinite(rho) & np.isfinite(jx) & np.isfinite(jy) & np.isfinite(usq)
    v = (rho, jx, jy, ux, uy)
    ny, nx = ob.shape
    return {"rows": [line([a[y, :] for a in v], counted[y, :], fluid[y, :]) for y in range(ny)],
            "columns": [line([a[:, x] for a in v], counted[:, x], fluid[:, x]) for x in range(nx)]}


def oracle_records(oracle, p, ob, cells, first, total, every):
    """(final lattice, {tt: record}) of the oracle run from global step `first` for `total` steps, sampled after every tt
    with tt % every == 0"""
    ref = cells.copy()
    out = {}
    for tt in range(first, first + total):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, 1)
        if tt % every == 0:
            out[tt] = record(ref, ob)
    return ref, out


def same_bits(got, want):
    """lines of the engine (numpy records of lbm.PROFILE_DTYPE, [n]) against the model's lines of one axis, bit for bit;
    returns what differs"""
    diff = []
    if len(got) != len(want):
        return [("lines", len(got), len(want))]
    for i, (g, w) in enumerate(zip(got, want)):
        for k in SUMS:
            if np.float64(g[k]).view(np.uint64) != np.float64(w[k]).view(np.uint64):
                diff.append((i, k, float(g[k]), w[k]))
        for k in ("fluid", "nonfinite"):
            if int(g[k]) != int(w[k]):
                diff.append((i, k, int(g[k]), int(w[k])))
    return diff
