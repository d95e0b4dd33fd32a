"""The mean fields' definition on the CPU (not a test): the sums lbm_set_mean / lbm_read_mean must reproduce bit for bit.
After every global step tt with tt % every == 0 the oracle's final_state of the lattice after tt + 1 steps is added, widened
to float64, to four per-cell sums that start at +0.0 -- sequentially, in step order."""
import numpy as np

import test_frames_format as model

FIELDS = ("u_x", "u_y", "u", "pressure")


def oracle_sums(oracle, p, ob, cells, start, total, every):
    """(lattice after `total` steps, {field: float64 (ny, nx)}, n) for the sample steps tt in [start, total); `cells` is
    the lattice after `start` steps and is left unchanged."""
    ref = cells.copy()
    sums = {k: np.zeros((p.ny, p.nx), dtype=np.float64) for k in FIELDS}
    done, n = start, 0
    for tt in model.frame_steps(start, total, every):
        oracle.run(p, ref, ob, tt + 1 - done)
        done = tt + 1
        state = oracle.final_state(p, ref, ob)
        for k in FIELDS:
            sums[k] = sums[k] + state[k].astype(np.float64)
        n += 1
    oracle.run(p, ref, ob, total - done)
    return ref, sums, n


def means_of(sums, n):
    """What Engine.mean() returns for these sums."""
    out = {k: sums[k] / float(n) for k in FIELDS}
    out["samples"] = n
    return out
