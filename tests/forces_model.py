"""The obstacle forces of include/lbm_hip.h (lbm_set_forces) in numpy, for the tests: the boundary links of an obstacle
map and the momentum the populations on them handed to the solid, summed exactly (math.fsum: the correctly rounded sum
of the exact terms)."""
import math

import numpy as np

CX = (0, 1, 0, -1, 0, 1, -1, -1, 1)   # SerialCode/d2q9-bgk.c:9-15:  6 2 5 / 3 0 1 / 7 4 8
CY = (0, 0, 1, 0, -1, 1, 1, -1, -1)


def links(obstacles, bodies=None):
    """[(body, y, x, k), ...] of the boundary links -- (b, k), k in 1..8, b blocked, b + c_k (both periodic wraps) not --
    ordered by body, then cell index y * nx + x, then k; `bodies` None: every blocked cell is body 0."""
    ob = np.asarray(obstacles) != 0
    ny, nx = ob.shape
    out = []
    for y, x in zip(*np.nonzero(ob)):
        for k in range(1, 9):
            if not ob[(y + CY[k]) % ny, (x + CX[k]) % nx]:
                out.append((0 if bodies is None else int(np.asarray(bodies)[y, x]), int(y), int(x), k))
    out.sort()
    return out


def link_counts(obstacles, bodies=None, n_bodies=1):
    counts = [0] * n_bodies
    for b, _, _, _ in links(obstacles, bodies):
        counts[b] += 1
    return counts


def terms(cells_aos, obstacles, bodies=None, n_bodies=1):
    """per body: ([x terms], [y terms]) = (double)(-2 c[k]) * (double)cells[b].speeds[k] over its links, each exact"""
    cells = np.asarray(cells_aos, dtype=np.float32).reshape(np.asarray(obstacles).shape + (9,))
    out = [([], []) for _ in range(n_bodies)]
    for b, y, x, k in links(obstacles, bodies):
        f = float(cells[y, x, k])
        out[b][0].append(-2.0 * CX[k] * f)
        out[b][1].append(-2.0 * CY[k] * f)
    return out


def force(cells_aos, obstacles, bodies=None, n_bodies=1):
    """float64 [n_bodies, 2]: F_x, F_y of every body, each the exact sum of its terms rounded once"""
    return np.array([[math.fsum(tx), math.fsum(ty)] for tx, ty in terms(cells_aos, obstacles, bodies, n_bodies)], dtype=np.float64)


def bound(cells_aos, obstacles, bodies=None, n_bodies=1):
    """float64 [n_bodies, 2]: n_links * 2^-52 * sum |term|, the distance a double sum of the terms in ANY order may have
    from the exact sum ((n - 1) 2^-53 sum |x| to first order, doubled for the higher orders)"""
    return np.array([[len(tx) * 2.0 ** -52 * math.fsum(map(abs, tx)), len(ty) * 2.0 ** -52 * math.fsum(map(abs, ty))]
                     for tx, ty in terms(cells_aos, obstacles, bodies, n_bodies)], dtype=np.float64)


def oracle_forces(oracle, p, ob, cells, first, total, every, bodies=None, n_bodies=1):
    """(final lattice, {tt: (force [n_bodies, 2], bound [n_bodies, 2])}) of the oracle run from global step `first` for
    `total` steps, sampled after every tt with tt % every == 0"""
    ref = cells.copy()
    out = {}
    for tt in range(first, first + total):
        oracle.run(p, ref, ob, 1)
        if tt % every == 0:
            out[tt] = (force(ref, ob, bodies, n_bodies), bound(ref, ob, bodies, n_bodies))
    return ref, out
