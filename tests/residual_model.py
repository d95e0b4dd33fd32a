"""The velocity residuals of include/lbm_hip.h (lbm_set_residual) in numpy float32, for the tests: per cell the moments
of tests/stats_model.py (as lbm_read_final_state computes them, every operation rounded to float32, none contracted),
blocked cells at velocity 0, the sums exact (math.fsum), the maximum with its first cell."""
import math

import numpy as np

import stats_model

FIELDS = ("sum_du_sq", "sum_u_sq", "nonfinite", "max_du", "max_x", "max_y", "span")


def field(cells_aos, obstacles):
    """the remembered field of a lattice: (u_x, u_y) float32 [ny, nx], blocked cells 0, 0"""
    ob = np.asarray(obstacles) != 0
    _, _, _, ux, uy, _, _ = stats_model.moments(np.asarray(cells_aos, dtype=np.float32).reshape(ob.shape + (9,)))
    zero = np.float32(0.0)
    return np.where(ob, zero, ux), np.where(ob, zero, uy)


def row(cells_aos, obstacles, remembered, span):
    """({field: value} of one sample against `remembered` = (pux, puy), the field this sample leaves behind)"""
    ob = np.asarray(obstacles) != 0
    pux, puy = remembered
    rho, jx, jy, ux, uy, usq, _ = stats_model.moments(np.asarray(cells_aos, dtype=np.float32).reshape(ob.shape + (9,)))
    with np.errstate(all="ignore"):
        dux = ux - pux
        duy = uy - puy
        dsq = (dux * dux) + (duy * duy)
        dmag = np.sqrt(dsq)
    for v in (dux, duy, dsq, dmag):
        assert v.dtype == np.float32
    fluid = ~ob
    finite = np.isfinite(rho) & np.isfinite(jx) & np.isfinite(jy) & np.isfinite(usq) & np.isfinite(dsq)
    counted = fluid & finite
    out = {"sum_du_sq": math.fsum(float(v) for v in dsq[counted]), "sum_u_sq": math.fsum(float(v) for v in usq[counted]),
           "nonfinite": int((fluid & ~finite).sum()), "span": int(span)}
    if counted.any():
        key = np.where(counted, dmag, np.float32(-1.0)).reshape(-1)
        at = int(np.argmax(key))                                         # the first of the largest: the smallest y * nx + x
        out.update(max_du=np.float32(key[at]), max_x=at % ob.shape[1], max_y=at // ob.shape[1])
    else:
        out.update(max_du=np.float32(0.0), max_x=-1, max_y=-1)
    return out, field(cells_aos, ob)


def oracle_rows(oracle, p, ob, cells, first, total, every):
    """(final lattice, {tt: row}) of the oracle run from global step `first` for `total` steps: the baseline is the field
    of `cells` (the lattice after `first` steps), sampled after every tt with tt % every == 0"""
    ref = cells.copy()
    remembered, at = field(ref, ob), first
    out = {}
    for tt in range(first, first + total):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, 1)
        if tt % every == 0:
            out[tt], remembered = row(ref, ob, remembered, tt + 1 - at)
            at = tt + 1
    return ref, out


POISON_COUNTS = (4, 18, 48)


def poisoned(cells_16x8):
    """a 16 x 8 start lattice with one NaN and one +Inf population in fluid cells far apart: with the 2 x 2 block at
    ob[3:5, 6:8] the model's rows after steps 1-3 count POISON_COUNTS cells (after step 1: the two cells the populations
    moved to and the two whose remembered velocity is not a number; then what spreads from them)"""
    c = np.array(cells_16x8, dtype=np.float32, copy=True)
    c[0, 0, 1] = np.nan
    c[5, 10, 3] = np.inf
    return c


def same_bits(got, want):
    """a row of the engine (numpy record of lbm.RESIDUAL_DTYPE) against a model row, bit for bit; returns what differs"""
    diff = []
    for k in ("sum_du_sq", "sum_u_sq"):
        if np.float64(got[k]).view(np.uint64) != np.float64(want[k]).view(np.uint64):
            diff.append((k, float(got[k]), want[k]))
    if np.float32(got["max_du"]).view(np.uint32) != np.float32(want["max_du"]).view(np.uint32):
        diff.append(("max_du", float(got["max_du"]), float(want["max_du"])))
    for k in ("nonfinite", "max_x", "max_y", "span"):
        if int(got[k]) != int(want[k]):
            diff.append((k, int(got[k]), int(want[k])))
    return diff
