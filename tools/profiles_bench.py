"""us per timestep with the line profiles armed (Engine.set_profiles: each axis alone and both) against the same engine
unarmed, the time of one sample next to the compulsory bytes, and the loop the recorder replaces: run(every) +
final_state() + numpy line sums on the host; same process.
python tools/profiles_bench.py [--sizes 128,1024,8192] [--batch-only]

The reference's 128^2 and 1024^2 data sets and the benchmark's 8192^2 grid (the 1024^2 obstacle map tiled 8 x 8): calls
of N timesteps (4000, 1000, 100), median of 5 timed calls (run + sync) each after one warm-up call; the recorder is
re-armed outside the timed region before every call, so the ring is never drained inside it.  Columns at every = 100:
unarmed (twice, back to back: their spread is the noise of the box), rows, columns, both, and the host loop (one call):
run(every), final_state(), then per row and per column the float64 numpy sums of u_x and u_y over the fluid cells and
their counts -- plain double sums of two of the five quantities, cheaper than the exact ones the engine gives.
One sample: 50 calls of run(1) armed at every = 1 against 50 unarmed, the difference per call (per slab one memset and
one launch per selected axis), for each choice of axes; beside it the compulsory bytes, 37 B per cell (nine populations
and the mask byte) and per selected axis, at the copy rate the statistics' bench measured on this device with one
device-to-device copy of 1 GiB (4.733 TB/s, read + write counted).  The batch leg: 8 members of 128^2, 4000 steps per call."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402

COPY_RATE = 4.733e12          # bytes per second, profiles/stats_bench.log
AXES = (("rows", 1), ("columns", 2), ("both", 3))


def timed(eng, steps, arm, repeats=5):
    samples = []
    for i in range(repeats + 1):
        arm(eng)
        eng.sync()
        t0 = time.perf_counter()
        eng.run(steps)
        eng.sync()
        if i:
            samples.append(time.perf_counter() - t0)
    return statistics.median(samples) / steps * 1e6


def unarmed(eng):
    eng.set_profiles(0)


def profiles(every, steps, axes):
    def arm(eng):
        eng.set_profiles(every, -(-steps // every), axes)
    return arm


def host_lines(state, fluid):
    out = []
    for axis in (1, 0):
        out.append(fluid.sum(axis=axis))
        for k in ("u_x", "u_y"):
            out.append(state[k].sum(axis=axis, dtype=np.float64, where=fluid))
    return out


def loop(eng, steps, every, fluid):
    unarmed(eng)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(steps // every):
        eng.run(every)
        host_lines(eng.final_state(), fluid)
    return (time.perf_counter() - t0) / (steps // every * every) * 1e6


def one_sample_us(eng, calls=50):
    t = {}
    for label, arm in [("unarmed", unarmed)] + [(name, profiles(1, calls, axes)) for name, axes in AXES]:
        samples = []
        for i in range(4):
            arm(eng)
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                eng.run(1)
            eng.sync()
            if i:
                samples.append(time.perf_counter() - t0)
        t[label] = statistics.median(samples) / calls * 1e6
    return {name: t[name] - t["unarmed"] for name, _ in AXES}, t["unarmed"]


def case(lbm, n, calls):
    if n == 8192:
        tile = lbm.read_obstacles(os.path.join(conftest.GOLDEN, "inputs", "obstacles_1024x1024.dat"), 1024, 1024)
        p = lbm.Params(n, n, 80 * calls, 10, 0.1, 0.01, 1.85)
        return p, tile, True, np.tile(np.asarray(tile).reshape(1024, 1024), (8, 8)) == 0
    p, ob = conftest.dataset(f"{n}x{n}")
    p.max_iters = 80 * calls
    return p, ob, False, np.asarray(ob).reshape(n, n) == 0


def batch_leg(lbm, steps=4000, members=8):
    p, ob = conftest.dataset("128x128")
    p.max_iters = 40 * steps
    params = [lbm.Params(p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel * (1 + 0.05 * i), p.omega) for i in range(members)]
    with lbm.Batch(params, [ob] * members) as batch:
        t = {}
        for label, every, axes in (("unarmed", 0, 3), ("unarmed again", 0, 3), ("rows every 100", 100, 1), ("columns every 100", 100, 2),
                                   ("both every 100", 100, 3)):
            samples = []
            for i in range(4):
                batch.set_profiles(every, -(-steps // every) if every else 0, axes)
                batch.sync()
                t0 = time.perf_counter()
                batch.run(steps)
                batch.sync()
                if i:
                    samples.append(time.perf_counter() - t0)
            t[label] = statistics.median(samples) / steps * 1e6
        base = t["unarmed"]
        print(f"batch of {members} x 128x128 ({steps} steps per call): us/step  "
              + "  ".join(f"{label} {v:8.3f} ({v / base:6.3f}x)" for label, v in t.items()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,1024,8192")
    ap.add_argument("--batch-only", action="store_true")
    args = ap.parse_args()
    lbm = conftest.load_package()
    if args.batch_only:
        return batch_leg(lbm)
    every = 100
    for n in [int(v) for v in args.sizes.split(",")]:
        steps = {128: 4000, 1024: 1000}.get(n, 100)
        p, ob, tiled, fluid = case(lbm, n, steps)
        with lbm.Engine(p, ob, tiled=tiled) as eng:
            resident = "yes" if eng.info()["resident_steps"] else "no"
            cols = [("unarmed", unarmed), ("unarmed again", unarmed)] + [(name, profiles(every, steps, axes)) for name, axes in AXES]
            t = {label: timed(eng, steps, arm) for label, arm in cols}
            t["run+final_state+numpy loop"] = loop(eng, steps, every, fluid)
            base = t["unarmed"]
            print(f"{n:>5}^2 every {every:>3} ({steps} steps per call): us/step  "
                  + "  ".join(f"{label} {v:10.3f} ({v / base:7.3f}x)" for label, v in t.items())
                  + f"  [resident {resident}]", flush=True)
            sample, step1 = one_sample_us(eng)
            bytes_us = 37.0 * n * n / COPY_RATE * 1e6
            print(f"{n:>5}^2 one sample (memset + launches): "
                  + "  ".join(f"{name} {sample[name]:9.2f} us ({sample[name] / (bytes_us * (2 if name == 'both' else 1)):6.2f}x its bytes)" for name, _ in AXES)
                  + f"  (run(1) unarmed {step1:9.2f} us)   37 B/cell and axis at the copy rate: {bytes_us:9.2f} us", flush=True)
    batch_leg(lbm)


if __name__ == "__main__":
    main()
