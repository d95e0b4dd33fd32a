"""The lattice statistics of include/lbm_hip.h (lbm_set_stats) in numpy float32, for the tests: per cell the moments as
lbm_read_final_state computes them (every operation rounded to float32, none contracted), the sums exact (math.fsum:
the correctly rounded sum of the exact terms), the maximum with its first cell."""
import math

import numpy as np

FIELDS = ("mass", "mom_x", "mom_y", "sum_u_sq", "nonfinite", "max_u", "max_x", "max_y")


def moments(cells_aos):
    """rho, jx, jy, ux, uy, usq, umag as float32 [ny, nx]"""
    f = np.asarray(cells_aos, dtype=np.float32)
    with np.errstate(all="ignore"):
        rho = f[..., 0]
        for k in range(1, 9):
            rho = rho + f[..., k]
        jx = ((f[..., 1] + f[..., 5]) + f[..., 8]) - ((f[..., 3] + f[..., 6]) + f[..., 7])
        jy = ((f[..., 2] + f[..., 5]) + f[..., 6]) - ((f[..., 4] + f[..., 7]) + f[..., 8])
        ux = jx / rho
        uy = jy / rho
        usq = (ux * ux) + (uy * uy)
        umag = np.sqrt(usq)
    for v in (rho, jx, jy, ux, uy, usq, umag):
        assert v.dtype == np.float32
    return rho, jx, jy, ux, uy, usq, umag


def terms(cells_aos, obstacles):
    """({name: [float terms]}, nonfinite, (max_u float32, max_x, max_y)) of one lattice"""
    ob = np.asarray(obstacles) != 0
    rho, jx, jy, _, _, usq, umag = moments(np.asarray(cells_aos, dtype=np.float32).reshape(ob.shape + (9,)))
    fluid = ~ob
    finite = np.isfinite(rho) & (ob | (np.isfinite(jx) & np.isfinite(jy) & np.isfinite(usq)))
    counted = finite & fluid
    t = {"mass": [float(v) for v in rho[finite]], "mom_x": [float(v) for v in jx[counted]],
         "mom_y": [float(v) for v in jy[counted]], "sum_u_sq": [float(v) for v in usq[counted]]}
    if counted.any():
        key = np.where(counted, umag, np.float32(-1.0)).reshape(-1)
        at = int(np.argmax(key))                                         # the first of the largest: the smallest y * nx + x
        peak = (np.float32(key[at]), at % ob.shape[1], at // ob.shape[1])
    else:
        peak = (np.float32(0.0), -1, -1)
    return t, int((~finite).sum()), peak


def row(cells_aos, obstacles):
    """{field: value} of one lattice: the sums exact and rounded once"""
    t, bad, (max_u, max_x, max_y) = terms(cells_aos, obstacles)
    out = {k: math.fsum(v) for k, v in t.items()}
    out.update(nonfinite=bad, max_u=max_u, max_x=max_x, max_y=max_y)
    return out


def bound(cells_aos, obstacles):
    """{sum: n * 2^-52 * sum |term|}: the distance a double sum of the terms in ANY order may have from the exact sum"""
    t, _, _ = terms(cells_aos, obstacles)
    return {k: len(v) * 2.0 ** -52 * math.fsum(map(abs, v)) for k, v in t.items()}


def oracle_rows(oracle, p, ob, cells, first, total, every):
    """(final lattice, {tt: row}) of the oracle run from global step `first` for `total` steps, sampled after every tt
    with tt % every == 0"""
    ref = cells.copy()
    out = {}
    for tt in range(first, first + total):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, 1)
        if tt % every == 0:
            out[tt] = row(ref, ob)
    return ref, out


def same_bits(got, want):
    """a row of the engine (numpy record of lbm.STATS_DTYPE) against a model row, bit for bit; returns what differs"""
    diff = []
    for k in ("mass", "mom_x", "mom_y", "sum_u_sq"):
        if np.float64(got[k]).view(np.uint64) != np.float64(want[k]).view(np.uint64):
            diff.append((k, float(got[k]), want[k]))
    if np.float32(got["max_u"]).view(np.uint32) != np.float32(want["max_u"]).view(np.uint32):
        diff.append(("max_u", float(got["max_u"]), float(want["max_u"])))
    for k in ("nonfinite", "max_x", "max_y"):
        if int(got[k]) != int(want[k]):
            diff.append((k, int(got[k]), int(want[k])))
    if "reserved" in getattr(got.dtype, "names", ()) and int(got["reserved"]) != 0:
        diff.append(("reserved", int(got["reserved"]), 0))
    return diff
