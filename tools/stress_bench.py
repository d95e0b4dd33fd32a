"""One stress_gather sample (Engine.set_stress) next to one stats_gather sample (Engine.set_stats) and one vorticity_gather
sample (Engine.set_enstrophy) of the same engine, alternating in one process; us per timestep with the stress armed at
every = 100 and every = 1 against the same engine unarmed; one stress() call; and the only other way to the same series:
the loop of run(every) + cells() + numpy on the host.
python tools/stress_bench.py [--sizes 128,1024,8192]

The reference's 128^2 and 1024^2 data sets and the benchmark's 8192^2 grid (the 1024^2 obstacle map tiled 8 x 8).
One sample: `calls` calls of run(1) armed at every = 1 against as many unarmed, the difference per call (one memset + one
gather launch); the kinds take turns, three rounds, the median of each; the ratios are against the statistics' sample,
whose kernel this tree does not change (profiles/stress_isa.txt).
Per step: calls of N timesteps (4000, 1000, 100), median of 3 timed calls (run + sync) each after one warm-up call; the
recorder is re-armed outside the timed region before every call.  every = 1 is the unarmed run(1) plus one sample, from
the sample measurement.  The host loop: run(100), cells(), then the second moments per cell in float32 numpy and the
float64 sums of q and txy, the maximum and the count of non-finite cells -- plain double sums, cheaper than the exact
ones the engine gives (5 samples; 1 at 8192^2)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402

KINDS = {"stress": lambda eng, every, cap: eng.set_stress(every, cap), "stats": lambda eng, every, cap: eng.set_stats(every, cap),
         "enstrophy": lambda eng, every, cap: eng.set_enstrophy(every, cap)}


def disarm(eng):
    eng.set_stress(0)
    eng.set_stats(0)
    eng.set_enstrophy(0)


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
    """({kind: us of one sample}, us of the unarmed run(1)), the kinds alternating; the unarmed run(1) measured in every round too"""
    t = {"unarmed": [], **{kind: [] for kind in KINDS}}
    run1_us(eng, calls, lambda e: None)                                  # warm-up
    for _ in range(rounds):
        t["unarmed"].append(run1_us(eng, calls, lambda e: None))
        for kind, setter in KINDS.items():
            t[kind].append(run1_us(eng, calls, lambda e: setter(e, 1, calls)))
    base = statistics.median(t["unarmed"])
    return {k: statistics.median(v) - base for k, v in t.items() if k != "unarmed"}, base


def host_row(cells, fluid):
    f = np.asarray(cells, dtype=np.float32).reshape(fluid.shape + (9,))
    with np.errstate(all="ignore"):
        rho = f.sum(axis=-1, dtype=np.float32)
        jx = f[..., 1] + f[..., 5] + f[..., 8] - (f[..., 3] + f[..., 6] + f[..., 7])
        jy = f[..., 2] + f[..., 5] + f[..., 6] - (f[..., 4] + f[..., 7] + f[..., 8])
        diag = f[..., 5] + f[..., 6] + f[..., 7] + f[..., 8]
        third = rho / np.float32(3.0)
        txx = ((f[..., 1] + f[..., 3] + diag - third) - jx * (jx / rho)) / rho
        tyy = ((f[..., 2] + f[..., 4] + diag - third) - jy * (jy / rho)) / rho
        txy = ((f[..., 5] + f[..., 7] - (f[..., 6] + f[..., 8])) - jx * (jy / rho)) / rho
        q = txx * txx + tyy * tyy + np.float32(2.0) * txy * txy
    ok = fluid & np.isfinite(q)
    at = int(np.argmax(np.where(ok, q, -1.0)))
    return float(q.sum(dtype=np.float64, where=ok)), float(txy.sum(dtype=np.float64, where=ok)), int((fluid & ~ok).sum()), at


def loop(eng, samples, every, fluid):
    disarm(eng)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(samples):
        eng.run(every)
        host_row(eng.cells(), fluid)
    return (time.perf_counter() - t0) / (samples * every) * 1e6


def stress_us(eng, repeats=5):
    disarm(eng)
    samples = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        eng.stress()
        samples.append(time.perf_counter() - t0)
    return statistics.median(samples[1:]) * 1e6


def case(lbm, n, calls):
    if n == 8192:
        tile = lbm.read_obstacles(os.path.join(conftest.GOLDEN, "inputs", "obstacles_1024x1024.dat"), 1024, 1024)
        p = lbm.Params(n, n, 60 * calls, 10, 0.1, 0.01, 1.85)
        return p, tile, True, np.tile(np.asarray(tile).reshape(1024, 1024), (8, 8)) == 0
    p, ob = conftest.dataset(f"{n}x{n}")
    p.max_iters = 60 * calls
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
            cap = -(-steps // 100)
            cols = [("unarmed", lambda e: None), ("unarmed again", lambda e: None), ("stress", lambda e: e.set_stress(100, cap)),
                    ("stats", lambda e: e.set_stats(100, cap)), ("enstrophy", lambda e: e.set_enstrophy(100, cap))]
            t = {label: timed(eng, steps, arm) for label, arm in cols}
            t["run+cells+numpy loop"] = loop(eng, 5 if n < 8192 else 1, 100, fluid)
            base = t["unarmed"]
            print(f"{n:>5}^2 every 100 ({steps} steps per call): us/step  "
                  + "  ".join(f"{label} {v:10.3f} ({v / base:7.3f}x)" for label, v in t.items())
                  + f"  speed-up of stress over the loop {t['run+cells+numpy loop'] / t['stress']:8.1f}x  [resident {resident}]", flush=True)
            one, step1 = sample_us(eng, 50 if n < 8192 else 20)
            print(f"{n:>5}^2 every 1: us/step  unarmed run(1) {step1:9.2f}   stress {step1 + one['stress']:9.2f} ({(step1 + one['stress']) / step1:6.3f}x)",
                  flush=True)
            print(f"{n:>5}^2 one sample: memset + stress_gather {one['stress']:9.2f} us   memset + stats_gather {one['stats']:9.2f} us   "
                  f"memset + vorticity_gather {one['enstrophy']:9.2f} us   stress / stats {one['stress'] / one['stats']:6.3f}   "
                  f"enstrophy / stats {one['enstrophy'] / one['stats']:6.3f}   one stress() call {stress_us(eng):10.2f} us", flush=True)


if __name__ == "__main__":
    main()
