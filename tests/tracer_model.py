"""numpy float64 model of the tracer particles (lbm_set_tracers), written from the definition in include/lbm_hip.h, not
from csrc/lbm_tracer_step.h: a tracer is (x, y) with the centre of cell (i, j) at (i, j); V is the bilinear interpolation
of the cell velocities (float32 widened, blocked cells 0, 0) with periodic neighbours; W wraps into [0, n); one advance
over a span of h timesteps is the midpoint rule in the field of the sample step.  numpy evaluates every +, -, * as one
IEEE double operation of its own, in the order written: nothing is fused.  Everything is vectorised over the tracers."""
import numpy as np


def wrap(z, n):
    """W(z, n) = z - n * floor(z / n); outside [0, n) (rounding) -> 0.0; of a z that is not finite: NaN"""
    z = np.asarray(z, dtype=np.float64)
    n = np.float64(n)
    with np.errstate(all="ignore"):
        w = z - n * np.floor(z / n)
    w = np.where((w >= 0.0) & (w < n), w, 0.0)
    return np.where(np.isfinite(z), w, np.nan)


def cell(z, n):
    """(i0, i1, f) of positions in [0, n)"""
    i0 = np.floor(z).astype(np.int64)
    f = z - i0.astype(np.float64)
    i1 = np.where(i0 + 1 == n, 0, i0 + 1)
    return i0, i1, f


def interp(ux, uy, x, y):
    """V(x, y): ux, uy float (ny, nx) planes with the blocked cells 0; x, y float64 arrays of positions inside the grid"""
    ny, nx = ux.shape
    i0, i1, fx = cell(x, nx)
    j0, j1, fy = cell(y, ny)
    out = []
    with np.errstate(all="ignore"):
        for plane in (ux, uy):
            u = np.asarray(plane).astype(np.float64)
            a = u[j0, i0] + fx * (u[j0, i1] - u[j0, i0])
            b = u[j1, i0] + fx * (u[j1, i1] - u[j1, i0])
            out.append(a + fy * (b - a))
    return out[0], out[1]


def advance(ux, uy, xy, h, unwrapped=False):
    """the positions xy float64 (..., 2) after one advance over a span of h timesteps in the field (ux, uy); lost
    tracers are (NaN, NaN) and stay so.  unwrapped: also (x + H * v2x, y + H * v2y), the end points before W -- what the
    tests ask for which edges a case crosses"""
    xy = np.asarray(xy, dtype=np.float64)
    ny, nx = ux.shape
    x, y = xy[..., 0], xy[..., 1]
    H = np.float64(h)
    alive = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(alive, x, 0.0), np.where(alive, y, 0.0)          # (no index from a position that is not finite)
    with np.errstate(all="ignore"):
        v1x, v1y = interp(ux, uy, xs, ys)
        xm, ym = wrap(xs + (np.float64(0.5) * H) * v1x, nx), wrap(ys + (np.float64(0.5) * H) * v1y, ny)
        alive = alive & np.isfinite(v1x) & np.isfinite(v1y) & np.isfinite(xm) & np.isfinite(ym)
        v2x, v2y = interp(ux, uy, np.where(alive, xm, 0.0), np.where(alive, ym, 0.0))
        x1, y1 = wrap(xs + H * v2x, nx), wrap(ys + H * v2y, ny)
        alive = alive & np.isfinite(v2x) & np.isfinite(v2y) & np.isfinite(x1) & np.isfinite(y1)
        ends = np.stack([xs + H * v2x, ys + H * v2y], axis=-1)
    out = np.stack([np.where(alive, x1, np.nan), np.where(alive, y1, np.nan)], axis=-1)
    return (out, ends) if unwrapped else out


def crossed(ends, nx, ny):
    """which of the four edges the unwrapped end points of `advance` lie beyond: (west, east, south, north)"""
    return (bool((ends[..., 0] < 0).any()), bool((ends[..., 0] >= nx).any()), bool((ends[..., 1] < 0).any()), bool((ends[..., 1] >= ny).any()))


def spans(first, total, every):
    """{tt: span} of the samples of `total` steps from global step `first`, armed there: the steps since the previous
    sample, or since arming"""
    out, last = {}, first
    for tt in range(first, first + total):
        if tt % every == 0:
            out[tt] = tt + 1 - last
            last = tt + 1
    return out


def oracle_rows(oracle, p, ob, cells, first, total, every, xy):
    """(final lattice, {tt: positions after the sample of step tt}) of the oracle run from global step `first` for `total`
    steps with the tracers xy armed at `first`: oracle.final_state's u_x, u_y of each sample step, advanced over its span"""
    ref = cells.copy()
    xy = np.asarray(xy, dtype=np.float64).copy()
    span, out = spans(first, total, every), {}
    for tt in range(first, first + total):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, 1)
        if tt in span:
            with np.errstate(all="ignore"):
                state = oracle.final_state(p, ref, ob)
            xy = advance(state["u_x"], state["u_y"], xy, span[tt])
            out[tt] = xy
    return ref, out


def same_bits(a, b):
    """two arrays of positions, bit for bit; NaNs by position"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])
