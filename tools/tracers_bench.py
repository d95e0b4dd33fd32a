"""What the tracer particles (Engine.set_tracers) cost, in one process:
us per timestep armed at every = 4 and 16 against the same engine unarmed; the time of one sample (one tracer_advance
launch) against the number of tracers, for seeds in row-major order and for the same seeds randomly permuted; and the
only other way to the same positions: the loop of run(span) + final_state() + the numpy model on the host.
python tools/tracers_bench.py [--sizes 128,1024,8192]

The reference's 128^2 and 1024^2 data sets and the benchmark's 8192^2 grid (the 1024^2 obstacle map tiled 8 x 8); n = 1 024,
65 536 and 1 048 576 tracers on the three (seeds of tracer_seeds at the spacing that gives at least n, cut to n).
Per step: calls of N timesteps (4000, 1000, 96), median of 3 timed calls (run + sync) each after one warm-up call; the
tracers are re-armed, without a ring, outside the timed region before every call, and the unarmed engine is measured
before and after the armed ones.
One sample: `calls` calls of run(1) armed at every = 1 without a ring against as many unarmed, the difference per call;
armed and unarmed alternate, three rounds, the median of each.
The host loop: run(16), final_state(), tests/tracer_model.advance (5 samples; 1 at 8192^2)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import tracer_model  # noqa: E402


def disarm(eng):
    eng.set_tracers(np.zeros((0, 2)), 0)


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


def sample_us(eng, calls, xy, rounds=3):
    """us of one sample of the tracers xy: run(1) armed at every = 1 minus run(1) unarmed, alternating"""
    armed, unarmed = [], []
    run1_us(eng, calls, lambda e: None)                                  # warm-up
    for _ in range(rounds):
        unarmed.append(run1_us(eng, calls, lambda e: None))
        armed.append(run1_us(eng, calls, lambda e: e.set_tracers(xy, 1, 0)))
    return statistics.median(armed) - statistics.median(unarmed), statistics.median(unarmed)


def loop(eng, samples, span, xy):
    disarm(eng)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(samples):
        eng.run(span)
        state = eng.final_state()
        xy = tracer_model.advance(state["u_x"], state["u_y"], xy, span)
    return (time.perf_counter() - t0) / (samples * span) * 1e6


def case(lbm, n, calls):
    if n == 8192:
        tile = lbm.read_obstacles(os.path.join(conftest.GOLDEN, "inputs", "obstacles_1024x1024.dat"), 1024, 1024)
        p = lbm.Params(n, n, 80 * calls, 10, 0.1, 0.01, 1.85)
        return p, tile, True, np.tile(np.asarray(tile).reshape(1024, 1024), (8, 8))
    p, ob = conftest.dataset(f"{n}x{n}")
    p.max_iters = 80 * calls
    return p, ob, False, np.asarray(ob).reshape(n, n)


def seeds(lbm, ob, n):
    """n row-major seeds, and all the counts the sample is timed at"""
    spacing = 1
    while len(lbm.tracer_seeds(ob, spacing + 1)) >= n:
        spacing += 1
    return lbm.tracer_seeds(ob, spacing)[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,1024,8192")
    args = ap.parse_args()
    lbm = conftest.load_package()
    for size in [int(v) for v in args.sizes.split(",")]:
        steps = {128: 4000, 1024: 1000}.get(size, 96)
        n = {128: 1024, 1024: 65536}.get(size, 1048576)
        p, ob, tiled, full = case(lbm, size, steps)
        xy = seeds(lbm, full, n)
        shuffled = xy[np.random.default_rng(1).permutation(len(xy))]
        with lbm.Engine(p, ob, tiled=tiled) as eng:
            resident = "yes" if eng.info()["resident_steps"] else "no"
            cols = [("unarmed", lambda e: None), ("every 4", lambda e: e.set_tracers(xy, 4, 0)), ("every 16", lambda e: e.set_tracers(xy, 16, 0)),
                    ("every 16 shuffled", lambda e: e.set_tracers(shuffled, 16, 0)), ("unarmed again", lambda e: None)]
            t = {label: timed(eng, steps, arm) for label, arm in cols}
            t["run+final_state+numpy loop, span 16"] = loop(eng, 5 if size < 8192 else 1, 16, xy)
            base = t["unarmed"]
            print(f"{size:>5}^2 {len(xy)} tracers ({steps} steps per call): us/step  "
                  + "  ".join(f"{label} {v:10.3f} ({v / base:7.3f}x)" for label, v in t.items())
                  + f"  the loop over every 16: {t['run+final_state+numpy loop, span 16'] / t['every 16']:8.1f}x  [resident {resident}]", flush=True)
            calls = 50 if size < 8192 else 20
            for m in sorted({min(n, v) for v in (1024, 16384, 65536, 262144, 1048576)}):
                ordered, step1 = sample_us(eng, calls, xy[:m])
                permuted, _ = sample_us(eng, calls, np.ascontiguousarray(xy[:m][np.random.default_rng(2).permutation(m)]))
                print(f"{size:>5}^2 one sample of {m:>8} tracers: row-major {ordered:9.2f} us ({ordered / m * 1e3:7.3f} ns per tracer)   "
                      f"permuted {permuted:9.2f} us ({permuted / ordered:6.2f}x)   [unarmed run(1) {step1:9.2f} us]", flush=True)


if __name__ == "__main__":
    main()
