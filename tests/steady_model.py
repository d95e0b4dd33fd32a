"""numpy model of the steady-state criterion of lbm_run_until (include/lbm_hip.h, "steady-state runs"), including the
order of the sums, so that a run's verdict can be re-computed from its av_vels series bit for bit.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np


def segment_mean(av: np.ndarray) -> float:
    """(sum of av as double) / len(av) in the order of the engine's 64-lane reduction: lane i adds elements i, i+64,
    ... in turn, then acc[i] += acc[i+off] for off = 32, 16, ..., 1."""
    av = np.asarray(av, dtype=np.float32)
    acc = np.zeros(64, dtype=np.float64)
    for start in range(0, av.size, 64):          # one element per lane and turn
        chunk = av[start:start + 64].astype(np.float64)
        acc[:chunk.size] = acc[:chunk.size] + chunk
    off = 32
    while off:
        acc[:off] = acc[:off] + acc[off:2 * off]
        off >>= 1
    return float(acc[0] / np.float64(av.size))


def rel_change(m: float, prev: float) -> float:
    if m == 0.0:
        return 0.0 if prev == 0.0 else math.inf
    return abs(m - prev) / abs(m)


def run_until(av_vels: np.ndarray, max_steps: int, check_every: int, tol: float, patience: int) -> dict:
    """What lbm_run_until(max_steps, check_every, tol, patience) decides on a run whose av_vels series (counted from the
    start of the call, at least as long as the call gets) is `av_vels`.  Also returns every r_j (`rels`, j = 2, ...)."""
    av = np.asarray(av_vels, dtype=np.float32)
    E = int(check_every)
    res = {"steps_run": 0, "steady": False, "steady_step": -1, "checks": 0, "last_rel": math.inf, "last_mean": 0.0,
           "rels": []}
    prev, streak = None, 0
    for j in range(1, max_steps // E + 1):
        m = segment_mean(av[(j - 1) * E:j * E])
        assert av.size >= j * E, "the series is shorter than the run"
        res["steps_run"] = j * E
        if prev is not None:
            r = rel_change(m, prev)
            streak = streak + 1 if r <= tol else 0
            res["checks"] += 1
            res["last_rel"] = r
            res["rels"].append(r)
            if streak >= patience:
                res["steady"], res["steady_step"] = True, j * E
        prev = m
        res["last_mean"] = m
        if res["steady"]:
            return res
    res["steps_run"] = max_steps     # the rest of the cap is run, not checked
    return res


def batch_run_until(series: list, max_steps: int, check_every: int, tol: float, patience: int) -> tuple[int, list]:
    """lbm_batch_run_until: every member's own verdict (frozen once steady); the batch stops when all are steady."""
    members = [run_until(av, max_steps, check_every, tol, patience) for av in series]
    steps = max(m["steady_step"] for m in members) if all(m["steady"] for m in members) else max_steps
    for m in members:
        m["steps_run"] = steps
    return steps, members


def margin(rels, tol: float) -> float:
    """Smallest factor between any r_j and tol (>= 1; inf for an empty run): how far every decision is from flipping."""
    out = math.inf
    for r in rels:
        if r == tol:
            return 1.0
        if r == 0.0 or math.isinf(r) or tol == 0.0:
            continue
        out = min(out, max(r / tol, tol / r))
    return out


# ---- the cases the GPU tests run (tests/test_gpu_steady.py); tests/test_steady_model.py checks on the CPU oracle that
# ---- every decision in them is a factor >= 3 away from tol, so that the kernels' av_vels (within 2e-4 of the oracle's)
# ---- cannot move one
MARGIN = 3.0


def obstacle_map(nx: int, ny: int) -> np.ndarray:
    """Row 0 blocked plus the block rows 6..9 x columns 16..19."""
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0, :] = 1
    ob[6:10, 16:20] = 1
    return ob


# shape -> (nx, ny); "resident" runs the resident kernel with one segment of look-ahead, "per_pass" (nx not a multiple
# of 64) the launch-per-pass kernels
SHAPES = {"resident": (64, 16), "per_pass": (100, 16)}
DENSITY, ACCEL, OMEGA = 0.1, 0.005, 1.0
STEADY = {"max_steps": 4096, "check_every": 512, "tol": 1e-3, "patience": 2}       # both shapes: steady after 2048
NOT_STEADY = {"max_steps": 1300, "check_every": 512, "tol": 1e-9, "patience": 2}   # never met; 1300 = 2 * 512 + 276
GO_ON = 37                                                                          # run(k) after the steady stop
SECOND = {"max_steps": 2048, "check_every": 512, "tol": 1e-3, "patience": 2}       # a second call, its own segments
CAPACITY = 8192
# batch of 8 x 64x16 (omega, accel): four members are steady after 2048 steps, four after 2560
BATCH = [(0.6, 0.005), (1.38, 0.005), (0.8, 0.01), (1.36, 0.004), (1.0, 0.005), (1.38, 0.01), (1.0, 0.01), (1.4, 0.01)]
BATCH_STEADY = {"max_steps": 4096, "check_every": 512, "tol": 1e-3, "patience": 2}


def case_params(lbm, shape: str, omega: float = OMEGA, accel: float = ACCEL):
    nx, ny = SHAPES[shape]
    return lbm.Params(nx, ny, CAPACITY, ny, DENSITY, accel, omega), obstacle_map(nx, ny)
