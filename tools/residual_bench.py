"""us per timestep with the velocity residuals armed (Engine.set_residual) against the same engine unarmed, the time of
one residual_gather sample next to one stats_gather sample, and the only other way to the same series: the loop of
run(every) + final_state() with a host subtraction; same process.
python tools/residual_bench.py [--sizes 128,1024,8192] [--batch-only]

The reference's 128^2 and 1024^2 data sets and the benchmark's 8192^2 grid (the 1024^2 obstacle map tiled 8 x 8): calls
of N timesteps (4000, 1000, 100), median of 5 timed calls (run + sync) each after one warm-up call; the recorder is
re-armed outside the timed region before every call, so the ring is never drained inside it (and the baseline launch is
not timed).  Columns, each at every = 100 and every = 1: unarmed (twice, back to back: their spread is the noise of the
box), residual, and the host loop (one call; at every = 1 over N / 20 steps, 2 at 8192^2): run(every), final_state(), then
|u - u_before|^2 and |u|^2 per cell in float32 and their float64 numpy sums and the maximum -- plain double sums, cheaper
than the exact ones the engine gives.
One sample: 50 calls of run(1) armed at every = 1 against 50 unarmed, the difference per call (one memset + one gather
per slab), for the residuals and for the statistics in turn, twice each; by bytes a residual sample moves 36 + 1 + 8 + 8 =
53 B per cell against stats_gather's 37.  The batch leg: 8 members of 128^2, 4000 steps per call."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402


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
    eng.set_residual(0)
    eng.set_stats(0)


def residual(every, steps):
    def arm(eng):
        eng.set_stats(0)
        eng.set_residual(every, -(-steps // every))
    return arm


def stats(every, steps):
    def arm(eng):
        eng.set_residual(0)
        eng.set_stats(every, -(-steps // every))
    return arm


def host_row(state, before, fluid):
    ux, uy = state["u_x"], state["u_y"]
    with np.errstate(all="ignore"):
        dsq = (ux - before[0]) ** 2 + (uy - before[1]) ** 2
        usq = ux * ux + uy * uy
    ok = fluid & np.isfinite(dsq) & np.isfinite(usq)
    at = int(np.argmax(np.where(ok, dsq, -1.0)))
    return (float(dsq.sum(dtype=np.float64, where=ok)), float(usq.sum(dtype=np.float64, where=ok)), int((fluid & ~ok).sum()), at), (ux, uy)


def loop(eng, steps, every, fluid):
    unarmed(eng)
    state = eng.final_state()
    before = (state["u_x"], state["u_y"])
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(steps // every):
        eng.run(every)
        _, before = host_row(eng.final_state(), before, fluid)
    return (time.perf_counter() - t0) / (steps // every * every) * 1e6


def one_sample_us(eng, arm_with, calls=50):
    t = {}
    for label, arm in (("unarmed", unarmed), ("armed", arm_with(1, calls))):
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
    return t["armed"] - t["unarmed"], t["unarmed"]


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
        for label, every in (("unarmed", 0), ("unarmed again", 0), ("residual every 100", 100), ("residual every 1", 1)):
            samples = []
            for i in range(4):
                batch.set_residual(every, -(-steps // every) if every else 0)
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
    for n in [int(v) for v in args.sizes.split(",")]:
        steps = {128: 4000, 1024: 1000}.get(n, 100)
        p, ob, tiled, fluid = case(lbm, n, steps)
        with lbm.Engine(p, ob, tiled=tiled) as eng:
            resident = "yes" if eng.info()["resident_steps"] else "no"
            for every in (100, 1):
                cols = [("unarmed", unarmed), ("unarmed again", unarmed), ("residual", residual(every, steps))]
                t = {label: timed(eng, steps, arm) for label, arm in cols}
                t["run+final_state+numpy loop"] = loop(eng, steps if every > 1 else (steps // 20 if n < 8192 else 2), every, fluid)
                base = t["unarmed"]
                print(f"{n:>5}^2 every {every:>3} ({steps} steps per call): us/step  "
                      + "  ".join(f"{label} {v:10.3f} ({v / base:7.3f}x)" for label, v in t.items())
                      + f"  [resident {resident}]", flush=True)
            spread = abs(t["unarmed again"] - t["unarmed"]) / t["unarmed"]
            for _ in range(2):
                res, step1 = one_sample_us(eng, residual)
                sta, _ = one_sample_us(eng, stats)
                print(f"{n:>5}^2 one sample (memset + gather): residual_gather {res:9.2f} us   stats_gather {sta:9.2f} us   ratio {res / sta:6.3f} "
                      f"(by bytes 53/37 = {53 / 37:.3f})   run(1) unarmed {step1:9.2f} us   spread of the two unarmed runs at every = 1: {spread:.3%}",
                      flush=True)
    batch_leg(lbm)


if __name__ == "__main__":
    main()
