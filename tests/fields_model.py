"""The field frames' definition on the CPU (not a test): what lbm_set_field_frames / lbm_read_field_frames must reproduce
bit for bit.  After every global step tt with tt % every == 0 the oracle's final_state of the lattice after tt + 1 steps,
cut to the window, for the chosen fields."""
import numpy as np

import test_frames_format as model

FIELDS = ("u_x", "u_y", "u", "pressure")


def oracle_field_frames(oracle, p, ob, cells, start, total, every, fields=FIELDS, window=None):
    """(lattice after `total` steps, {tt: {field: float32 (wny, wnx)}}) for the sample steps tt in [start, total); `cells`
    is the lattice after `start` steps and is left unchanged; `window` is (x0, y0, nx, ny), None: the whole grid."""
    x0, y0, wnx, wny = window if window is not None else (0, 0, p.nx, p.ny)
    ref = cells.copy()
    frames, done = {}, start
    for tt in model.frame_steps(start, total, every):
        oracle.run(p, ref, ob, tt + 1 - done)
        done = tt + 1
        state = oracle.final_state(p, ref, ob)
        frames[tt] = {k: state[k][y0:y0 + wny, x0:x0 + wnx].copy() for k in FIELDS if k in fields}
    oracle.run(p, ref, ob, total - done)
    return ref, frames


def assert_field_frames(steps, got, want, fields=FIELDS):
    """`got` = Engine.field_frames()'s dictionary for `steps`; `want` = oracle_field_frames' frames."""
    assert steps.tolist() == sorted(want), (steps.tolist(), sorted(want))
    assert list(got) == [k for k in FIELDS if k in fields]
    for i, tt in enumerate(steps.tolist()):
        for k in got:
            assert got[k][i].shape == want[tt][k].shape, (tt, k, got[k][i].shape, want[tt][k].shape)
            assert np.array_equal(got[k][i].view(np.uint32), want[tt][k].view(np.uint32)), f"field frame tt={tt} {k} differs"
