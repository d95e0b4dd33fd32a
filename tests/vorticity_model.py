"""The vorticity and the enstrophy row of include/lbm_hip.h (lbm_read_vorticity, lbm_set_enstrophy) in numpy float32, for
the tests: per cell the velocities as lbm_read_final_state computes them (stats_model.moments: every operation rounded
to float32, none contracted), blocked cells 0, np.roll for both periodic wraps, the sums exact (math.fsum: the correctly
rounded sum of the exact terms), the maximum with its first cell."""
import math

import numpy as np

import stats_model

FIELDS = ("enstrophy", "circulation", "nonfinite", "max_abs_w", "max_x", "max_y", "fluid")
MIN_BAND, TARGET_UNITS, BLOCK_WAVES, MAX_GROUPS = 8, 4096, 4, 512      # the host's band rule (lbm_hip.hip: vorticity_band_rows)


def vector(nx):
    return 4 if nx % 4 == 0 else 1


def strips(nx):
    return -(-nx // (64 * vector(nx)))


def band_rows(rows, nx):
    """rows of a band of vorticity_gather for a slab (or a reader's chunk) of `rows` rows: the host's vorticity_band_rows"""
    bands = max(TARGET_UNITS // strips(nx), 1)
    return max(-(-rows // bands), MIN_BAND)


def groups(rows, nx):
    """workgroups of one launch: the host's vorticity_groups"""
    return min(-(-(strips(nx) * -(-rows // band_rows(rows, nx))) // BLOCK_WAVES), MAX_GROUPS)


def field(cells_aos, obstacles):
    """(w float32 [ny, nx] -- 0 on blocked cells, non-finite values as computed --, counted bool [ny, nx]: the finite fluid
    cells, bad bool [ny, nx]: the fluid cells that are not finite)"""
    ob = np.asarray(obstacles) != 0
    rho, jx, jy, ux, uy, usq, _ = stats_model.moments(np.asarray(cells_aos, dtype=np.float32).reshape(ob.shape + (9,)))
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        ux = np.where(ob, zero, ux)
        uy = np.where(ob, zero, uy)
        dvdx = np.roll(uy, -1, axis=1) - np.roll(uy, 1, axis=1)
        dudy = np.roll(ux, -1, axis=0) - np.roll(ux, 1, axis=0)
        w = np.where(ob, zero, np.float32(0.5) * (dvdx - dudy))
        wsq = w * w
    assert w.dtype == np.float32 and wsq.dtype == np.float32
    own = np.isfinite(rho) & np.isfinite(jx) & np.isfinite(jy) & np.isfinite(usq)
    finite = own & np.isfinite(w) & np.isfinite(wsq)
    return w, ~ob & finite, ~ob & ~finite


def row(cells_aos, obstacles):
    """{field: value} of one lattice: the sums exact and rounded once"""
    w, counted, bad = field(cells_aos, obstacles)
    with np.errstate(all="ignore"):
        wsq = w * w
    out = {"enstrophy": math.fsum(float(v) for v in wsq[counted]), "circulation": math.fsum(float(v) for v in w[counted]),
           "nonfinite": int(bad.sum()), "fluid": int(counted.sum())}
    if counted.any():
        key = np.where(counted, np.abs(w), np.float32(-1.0)).reshape(-1)
        at = int(np.argmax(key))                                         # the first of the largest: the smallest y * nx + x
        out.update(max_abs_w=np.float32(key[at]), max_x=at % w.shape[1], max_y=at // w.shape[1])
    else:
        out.update(max_abs_w=np.float32(0.0), max_x=-1, max_y=-1)
    return out


def oracle_rows(oracle, p, ob, cells, first, total, every, fields_at=()):
    """(final lattice, {tt: row}, {tt: w}) of the oracle run from global step `first` for `total` steps, sampled after
    every tt with tt % every == 0; the field after the steps tt of fields_at"""
    ref = cells.copy()
    out, fields = {}, {}
    for tt in range(first, first + total):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, 1)
        if tt % every == 0:
            out[tt] = row(ref, ob)
        if tt in fields_at:
            fields[tt] = field(ref, ob)[0]
    return ref, out, fields


def same_bits(got, want):
    """a row of the engine (numpy record of lbm.ENSTROPHY_DTYPE) against a model row, bit for bit; returns what differs"""
    diff = []
    for k in ("enstrophy", "circulation"):
        if np.float64(got[k]).view(np.uint64) != np.float64(want[k]).view(np.uint64):
            diff.append((k, float(got[k]), want[k]))
    if np.float32(got["max_abs_w"]).view(np.uint32) != np.float32(want["max_abs_w"]).view(np.uint32):
        diff.append(("max_abs_w", float(got["max_abs_w"]), float(want["max_abs_w"])))
    for k in ("nonfinite", "max_x", "max_y", "fluid"):
        if int(got[k]) != int(want[k]):
            diff.append((k, int(got[k]), int(want[k])))
    return diff


def same_field(got, want):
    """the engine's field against the model's: the same cells NaN (a NaN's payload is not the arithmetic's to keep), the
    rest bit for bit"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(nan, np.isnan(got)) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
