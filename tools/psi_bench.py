"""One stream-function sample (Engine.set_psi: psi_band_totals, psi_band_bases, psi_scan, psi_extrema) next to a
profile_columns-only sample (Engine.set_profiles(.., ("columns",))) and a stats_gather sample (Engine.set_stats) of the same
engine, alternating in one process; us per timestep with psi armed at every = 100 against the same engine unarmed; one
psi() call; and the only other way to the same series: the loop of run(every) + final_state() + numpy on the host.
python tools/psi_bench.py [--sizes 128,1024,8192]

The reference's 128^2 and 1024^2 data sets and the benchmark's 8192^2 grid (the 1024^2 obstacle map tiled 8 x 8).
One sample: `calls` calls of run(1) armed at every = 1 against as many unarmed, the difference per call; the three kinds
take turns, three rounds, the median of each; the ratios are psi / profile columns and psi / statistics.
Per step: calls of N timesteps (4000, 1000, 100), median of 3 timed calls (run + sync) each after one warm-up call; the
recorder is re-armed outside the timed region before every call.  The host loop: run(100), final_state(), then
rho * u_x per cell, a float64 np.cumsum along y and its extrema over the fluid cells -- plain double sums, cheaper than the
exact prefixes the engine gives (one call; 2 samples at 8192^2)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402

KINDS = {"psi": lambda eng, every, cap: eng.set_psi(every, cap),
         "columns": lambda eng, every, cap: eng.set_profiles(every, cap, ("columns",)),
         "stats": lambda eng, every, cap: eng.set_stats(every, cap)}


def disarm(eng):
    eng.set_psi(0)
    eng.set_profiles(0)
    eng.set_stats(0)


def timed(eng, steps, arm, repeats=3):
    samples = []
    for i in range(repeats + 1):
        disarm(eng)
        arm(eng)
        eng.sync()
        t0 = time.perf_counter()
        eng.run(steps)
        eng.sync()
        if i:
            samples.append(time.perf_counter() - t0)
    return statistics.median(samples) / steps * 1e6


def run1_us(eng, calls, arm):
    disarm(eng)
    arm(eng)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        eng.run(1)
    eng.sync()
    return (time.perf_counter() - t0) / calls * 1e6


def sample_us(eng, calls, rounds=3):
    """{kind: us of one sample}, the kinds alternating; the unarmed run(1) measured in every round too"""
    t = {"unarmed": [], **{k: [] for k in KINDS}}
    run1_us(eng, calls, lambda e: None)                                  # warm-up
    for _ in range(rounds):
        t["unarmed"].append(run1_us(eng, calls, lambda e: None))
        for kind, setter in KINDS.items():
            t[kind].append(run1_us(eng, calls, lambda e: setter(e, 1, calls)))
    base = statistics.median(t["unarmed"])
    return {k: statistics.median(v) - base for k, v in t.items() if k != "unarmed"}, base


def host_row(state, fluid):
    with np.errstate(all="ignore"):
        jx = np.where(fluid, state["u_x"].astype(np.float64) * (3.0 * state["pressure"]), 0.0)      # rho = pressure / c_sq
    psi = np.cumsum(np.where(np.isfinite(jx), jx, 0.0), axis=0)
    return int(np.argmin(np.where(fluid, psi, np.inf))), int(np.argmax(np.where(fluid, psi, -np.inf)))


def loop(eng, samples, every, fluid):
    disarm(eng)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(samples):
        eng.run(every)
        host_row(eng.final_state(), fluid)
    return (time.perf_counter() - t0) / (samples * every) * 1e6


def psi_us(eng, repeats=3):
    disarm(eng)
    samples = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        eng.psi()
        samples.append(time.perf_counter() - t0)
    return statistics.median(samples[1:]) * 1e6


def case(lbm, n, calls):
    if n == 8192:
        tile = lbm.read_obstacles(os.path.join(conftest.GOLDEN, "inputs", "obstacles_1024x1024.dat"), 1024, 1024)
        p = lbm.Params(n, n, 80 * calls, 10, 0.1, 0.01, 1.85)
        return p, tile, True, np.tile(np.asarray(tile).reshape(1024, 1024), (8, 8)) == 0
    p, ob = conftest.dataset(f"{n}x{n}")
    p.max_iters = 80 * calls
    return p, ob, False, np.asarray(ob).reshape(n, n) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,1024,8192")
    args = ap.parse_args()
    lbm = conftest.load_package()
    for n in [int(v) for v in args.sizes.split(",")]:
        steps = {128: 4000, 1024: 1000}.get(n, 100)
        p, ob, tiled, fluid = case(lbm, n, steps)
        with lbm.Engine(p, ob, tiled=tiled) as eng:
            resident = "yes" if eng.info()["resident_steps"] else "no"
            cols = [("unarmed", lambda e: None), ("unarmed again", lambda e: None),
                    ("psi", lambda e: e.set_psi(100, -(-steps // 100))),
                    ("columns", lambda e: e.set_profiles(100, -(-steps // 100), ("columns",))),
                    ("stats", lambda e: e.set_stats(100, -(-steps // 100)))]
            t = {label: timed(eng, steps, arm) for label, arm in cols}
            t["run+final_state+numpy loop"] = loop(eng, 5 if n < 8192 else 2, 100, fluid)
            base = t["unarmed"]
            print(f"{n:>5}^2 every 100 ({steps} steps per call): us/step  "
                  + "  ".join(f"{label} {v:10.3f} ({v / base:7.3f}x)" for label, v in t.items()) + f"  [resident {resident}]", flush=True)
            one, step1 = sample_us(eng, 50 if n < 8192 else 20)
            print(f"{n:>5}^2 one sample: psi scan {one['psi']:9.2f} us   memset + profile_columns {one['columns']:9.2f} us   "
                  f"memset + stats_gather {one['stats']:9.2f} us   psi / columns {one['psi'] / one['columns']:6.3f}   "
                  f"psi / stats {one['psi'] / one['stats']:6.3f}   (run(1) unarmed {step1:9.2f} us)   one psi() call "
                  f"{psi_us(eng):10.2f} us", flush=True)


if __name__ == "__main__":
    main()
