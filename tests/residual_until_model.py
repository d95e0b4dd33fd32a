"""The criterion of lbm_run_until_residual (include/lbm_hip.h, "steady-state runs on the velocity residual") over model
rows of tests/residual_model.py, for the tests: one row per check, taken every check_every steps against the field of the
check before (the first: of the start of the call).  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

import residual_model
import steady_model as sm


def rel(row) -> float:
    """r = sqrt(sum_du_sq / sum_u_sq) in IEEE double, division and square root correctly rounded; residual_l2's corners"""
    du, u = float(row["sum_du_sq"]), float(row["sum_u_sq"])
    if u == 0.0:
        return 0.0 if du == 0.0 else math.inf
    return math.sqrt(du / u)


def run_until(rows, max_steps: int, check_every: int, tol: float, patience: int) -> dict:
    """What lbm_run_until_residual(max_steps, check_every, tol, patience) decides on a run whose checks give `rows`
    (rows[j - 1]: the row after segment j; at least as many as the call judges).  Also returns every r_j (`rels`) and
    `end_step`, the steps after which the verdict froze (steady or diverged; -1: it did not)."""
    E = int(check_every)
    res = {"steps_run": 0, "steady": False, "steady_step": -1, "checks": 0, "diverged": False, "last_rel": math.inf, "last": None,
           "rels": [], "end_step": -1}
    streak = 0
    for j in range(1, max_steps // E + 1):
        assert len(rows) >= j, "fewer rows than the run has checks"
        row = rows[j - 1]
        assert int(row["span"]) == E
        r = rel(row)
        res["steps_run"] = j * E
        res["checks"] += 1
        res["last_rel"], res["last"] = r, row
        res["rels"].append(r)
        if int(row["nonfinite"]) > 0:
            res["diverged"], res["end_step"] = True, j * E
            return res
        streak = streak + 1 if r <= tol else 0
        if streak >= patience:
            res["steady"], res["steady_step"], res["end_step"] = True, j * E, j * E
            return res
    res["steps_run"] = max_steps     # the rest of the cap is run, not checked
    return res


def batch_run_until(member_rows: list, max_steps: int, check_every: int, tol: float, patience: int) -> tuple[int, list]:
    """lbm_batch_run_until_residual: every member's own verdict, frozen once it is steady or diverged; the batch stops when
    every member is one or the other, or at max_steps.  The history has steps // check_every rows of all members."""
    members = [run_until(rows, max_steps, check_every, tol, patience) for rows in member_rows]
    steps = max(m["end_step"] for m in members) if all(m["end_step"] >= 0 for m in members) else max_steps
    for m in members:
        m["steps_run"] = steps
    return steps, members


def oracle_rows(oracle, p, ob, cells, n_checks: int, check_every: int):
    """(final lattice, [row]) of the oracle advanced from `cells` by n_checks segments of check_every steps: the baseline
    is the field of `cells`, row j - 1 compares the lattice after j segments with the one after j - 1."""
    ref = np.array(cells, dtype=np.float32, copy=True)
    remembered = residual_model.field(ref, ob)
    rows = []
    for _ in range(n_checks):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, check_every)
        row, remembered = residual_model.row(ref, ob, remembered, check_every)
        rows.append(row)
    return ref, rows


# ---- the cases the GPU tests run (tests/test_gpu_residual_until.py); tests/test_residual_until_abi.py pins on the CPU
# ---- oracle where each of them stops and that every r_j is a factor >= MARGIN from tol.  The rows are exact sums over
# ---- the oracle's lattice, which the kernels reproduce bit for bit, so the margin guards the pinned figures against a
# ---- change of the cases, not against rounding.
MARGIN = 2.5           # the single-lattice cases (the nearest r_j: 2.52e-4 against tol 1e-4)
BATCH_MARGIN = 2.4     # the batch: member (omega 1.0, accel 0.01) has r_2 = 2.466e-4, a factor 2.466 from tol, not 2.5
STEADY = {"max_steps": 4096, "check_every": 512, "tol": 1e-4, "patience": 2}       # both shapes: steady after 2048, 4 checks
NOT_STEADY = {"max_steps": 1300, "check_every": 512, "tol": 1e-9, "patience": 2}   # below the fp32 floor: never met
STEADY_STEPS = 2048
BATCH_STEADY_STEPS = (1536, 2560, 1536, 2560, 2048, 2560, 2048, 2560)              # the members of steady_model.BATCH
ODD = (102, 16)                                                                    # nx % 4 != 0: the one-cell gather


def case(lbm, shape, omega: float = sm.OMEGA, accel: float = sm.ACCEL):
    """(params, obstacles) of a steady_model shape name or of an (nx, ny) pair"""
    nx, ny = sm.SHAPES[shape] if isinstance(shape, str) else shape
    return lbm.Params(nx, ny, sm.CAPACITY, ny, sm.DENSITY, accel, omega), sm.obstacle_map(nx, ny)
