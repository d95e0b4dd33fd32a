"""The coarse frames of include/lbm_hip.h (lbm_set_coarse_frames, lbm_read_coarse) in numpy float32, for the tests: per
cell the moments of tests/stats_model.py (every operation rounded to float32, none contracted), per box of bx x by cells
what tests/profile_model.py gives per line: the sums exact (math.fsum) over the box's finite fluid cells, and the two
counts.  Boxes tile the grid from cell (0, 0); the last box of an axis may be ragged."""
import numpy as np

import profile_model
import stats_model

SUMS = profile_model.SUMS
FIELDS = profile_model.FIELDS


def shape(nx, ny, box):
    """(cy, cx)"""
    bx, by = box
    return -(-ny // by), -(-nx // bx)


def frame(cells_aos, obstacles, box):
    """[cy][cx] boxes of one lattice, a box being {field: value} as a line of profile_model"""
    bx, by = box
    ob = np.asarray(obstacles) != 0
    rho, jx, jy, ux, uy, usq, _ = stats_model.moments(np.asarray(cells_aos, dtype=np.float32).reshape(ob.shape + (9,)))
    fluid = ~ob
    counted = fluid & np.isfinite(rho) & np.isfinite(jx) & np.isfinite(jy) & np.isfinite(usq)
    v = (rho, jx, jy, ux, uy)
    ny, nx = ob.shape
    cy, cx = shape(nx, ny, box)
    cut = lambda a, X, Y: a[Y * by:(Y + 1) * by, X * bx:(X + 1) * bx].ravel()  # noqa: E731
    return [[profile_model.line([cut(a, X, Y) for a in v], cut(counted, X, Y), cut(fluid, X, Y)) for X in range(cx)] for Y in range(cy)]


def oracle_frames(oracle, p, ob, cells, first, total, every, box):
    """(final lattice, {tt: frame}) of the oracle run from global step `first` for `total` steps, sampled after every tt
    with tt % every == 0"""
    ref = cells.copy()
    out = {}
    for tt in range(first, first + total):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, 1)
        if tt % every == 0:
            out[tt] = frame(ref, ob, box)
    return ref, out


def same_bits(got, want):
    """a frame of the engine (numpy records of lbm.PROFILE_DTYPE, [cy][cx]) against the model's, bit for bit; returns what
    differs"""
    got = np.asarray(got)
    if got.ndim != 2 or got.shape != (len(want), len(want[0])):
        return [("shape", got.shape, (len(want), len(want[0])))]
    diff = []
    for Y, row in enumerate(want):
        diff += [((Y,) + d) for d in profile_model.same_bits(got[Y], row)]
    return diff
