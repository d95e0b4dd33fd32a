"""The second moments' definition on the CPU (not a test): the sums lbm_set_mean_order(ctx, every, 2) / lbm_read_mean2 must
reproduce bit for bit.  On every sample step of mean_model.oracle_sums the products of the oracle's final_state fields,
each factor widened to float64 first (so the product is exact), are added to four more per-cell sums that start at +0.0 --
sequentially, in step order."""
import numpy as np

import test_frames_format as model
from mean_model import FIELDS

PAIRS = {"u_x u_x": ("u_x", "u_x"), "u_y u_y": ("u_y", "u_y"), "u_x u_y": ("u_x", "u_y"), "pressure pressure": ("pressure", "pressure")}
FIELDS2 = tuple(PAIRS)


def oracle_sums2(oracle, p, ob, cells, start, total, every):
    """(lattice after `total` steps, first-moment sums, second-moment sums, n) for the sample steps tt in [start, total);
    `cells` is the lattice after `start` steps and is left unchanged.  The first-moment sums are mean_model.oracle_sums'."""
    ref = cells.copy()
    sums = {k: np.zeros((p.ny, p.nx), dtype=np.float64) for k in FIELDS}
    sums2 = {k: np.zeros((p.ny, p.nx), dtype=np.float64) for k in FIELDS2}
    done, n = start, 0
    for tt in model.frame_steps(start, total, every):
        oracle.run(p, ref, ob, tt + 1 - done)
        done = tt + 1
        state = oracle.final_state(p, ref, ob)
        for k in FIELDS:
            sums[k] = sums[k] + state[k].astype(np.float64)
        for k, (a, b) in PAIRS.items():
            sums2[k] = sums2[k] + state[a].astype(np.float64) * state[b].astype(np.float64)
        n += 1
    oracle.run(p, ref, ob, total - done)
    return ref, sums, sums2, n
