"""The mass stream function and its row of include/lbm_hip.h (lbm_read_psi, lbm_set_psi) for the tests: per cell jx in numpy
float32 in the header's order (stats_model.moments: every operation rounded to float32, none contracted), a term is jx of
a finite fluid cell and 0 of every other cell, each term a Python integer in units of 2^-149, the prefixes along y
cumulative sums of Python integers, each taken as int / 2**149 -- CPython's true division of integers is correctly
rounded, so every psi is the exact sum rounded once, to nearest-even: math.fsum's value of the same terms."""
import numpy as np

import stats_model

FIELDS = ("psi_min", "psi_max", "nonfinite", "min_x", "min_y", "max_x", "max_y", "fluid", "reserved")
UNIT = 2 ** 149                                       # every finite float32 is an integer multiple of 2^-149
COLUMNS, MIN_BAND, TARGET_GROUPS = 256, 8, 1024       # the host's band rule (lbm_hip.hip: psi_band_rows)


def band_rows(rows, nx, override=0):
    """rows of a band of the scan for a slab of `rows` rows: the host's psi_band_rows"""
    if override > 0:
        return override
    bands = max(TARGET_GROUPS // -(-nx // COLUMNS), 1)
    return max(-(-rows // bands), MIN_BAND)


def terms(cells_aos, obstacles):
    """(t float32 [ny, nx]: jx of the finite fluid cells, +0 elsewhere; counted bool: the finite fluid cells; bad bool: the
    fluid cells that are not finite)"""
    ob = np.asarray(obstacles) != 0
    with np.errstate(all="ignore"):
        rho, jx, jy, ux, uy, usq, _ = stats_model.moments(np.asarray(cells_aos, dtype=np.float32).reshape(ob.shape + (9,)))
    assert jx.dtype == np.float32
    finite = np.isfinite(rho) & np.isfinite(jx) & np.isfinite(jy) & np.isfinite(usq)
    counted = ~ob & finite
    return np.where(counted, jx, np.float32(0.0)), counted, ~ob & ~finite


def as_units(t):
    """the finite float32 values of t as Python integers in units of 2^-149, [ny][nx]"""
    out = []
    for row in np.asarray(t, dtype=np.float32):
        ints = []
        for v in row.tolist():                        # (a Python float holds a float32 exactly)
            num, den = float(v).as_integer_ratio()
            assert UNIT % den == 0
            ints.append(num * (UNIT // den))
        out.append(ints)
    return out


def field(cells_aos, obstacles):
    """(psi float64 [ny, nx], counted, bad)"""
    t, counted, bad = terms(cells_aos, obstacles)
    units = as_units(t)
    ny, nx = t.shape
    psi = np.zeros((ny, nx), dtype=np.float64)
    run = [0] * nx
    for y in range(ny):
        for x in range(nx):
            run[x] += units[y][x]
            psi[y, x] = run[x] / UNIT                 # correctly rounded; 0 / UNIT is +0.0
    return psi, counted, bad


def extrema(psi, counted):
    """(psi_min, min_x, min_y, psi_max, max_x, max_y) over the counted cells; ties: the smallest y * nx + x; none: 0, -1, -1"""
    if not counted.any():
        return 0.0, -1, -1, 0.0, -1, -1
    nx = psi.shape[1]
    lo = np.where(counted, psi, np.inf).reshape(-1)
    hi = np.where(counted, psi, -np.inf).reshape(-1)
    a, b = int(np.argmin(lo)), int(np.argmax(hi))     # the first of the smallest / largest (+0.0 == -0.0)
    return float(lo[a]) + 0.0, a % nx, a // nx, float(hi[b]) + 0.0, b % nx, b // nx


def row(cells_aos, obstacles):
    """{field: value} of one lattice"""
    psi, counted, bad = field(cells_aos, obstacles)
    lo, lx, ly, hi, hx, hy = extrema(psi, counted)
    return {"psi_min": lo, "psi_max": hi, "nonfinite": int(bad.sum()), "min_x": lx, "min_y": ly, "max_x": hx, "max_y": hy,
            "fluid": int(counted.sum()), "reserved": 0}


def oracle_rows(oracle, p, ob, cells, first, total, every):
    """(final lattice, {tt: row}) of the oracle run from global step `first` for `total` steps, sampled after every tt with
    tt % every == 0"""
    ref = cells.copy()
    out = {}
    for tt in range(first, first + total):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, 1)
        if tt % every == 0:
            out[tt] = row(ref, ob)
    return ref, out


def same_bits(got, want):
    """a row of the engine (numpy record of lbm.PSI_DTYPE) against a model row, bit for bit; returns what differs"""
    diff = []
    for k in ("psi_min", "psi_max"):
        if np.float64(got[k]).view(np.uint64) != np.float64(want[k]).view(np.uint64):
            diff.append((k, float(got[k]), want[k]))
    for k in ("nonfinite", "min_x", "min_y", "max_x", "max_y", "fluid", "reserved"):
        if int(got[k]) != int(want[k]):
            diff.append((k, int(got[k]), int(want[k])))
    return diff


def same_field(got, want):
    """the engine's field against the model's through uint64 views (no psi is a NaN: non-finite cells add 0)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
