"""us per timestep with the lattice statistics armed (Engine.set_stats) against the same engine unarmed, the time of one
stats_gather sample next to one lbm_total_density call and to the compulsory bytes, and the only other way to the same
series: the loop of run(every) + cells() + numpy on the host; same process.
python tools/stats_bench.py [--sizes 128,1024,8192] [--batch-only]

The reference's 128^2 and 1024^2 data sets and the benchmark's 8192^2 grid (the 1024^2 obstacle map tiled 8 x 8): calls
of N timesteps (4000, 1000, 100), median of 5 timed calls (run + sync) each after one warm-up call; the recorder is
re-armed outside the timed region before every call, so the ring is never drained inside it.  Columns, each at every = 100
and every = 1: unarmed (twice, back to back: their spread is the noise of the box), stats, and the host loop (one call;
at every = 1 over N / 20 steps, 2 at 8192^2): run(every), cells(), then rho, j and |u|^2 per cell in float32 and their float64 numpy
sums, the maximum and the count of non-finite cells -- plain double sums, cheaper than the exact ones the engine gives.
One sample: 50 calls of run(1) armed at every = 1 against 50 unarmed, the difference per call (one memset + one
stats_gather per slab); one lbm_total_density call (lattice_sums + its reduction + the read-back: the same bytes in plain
double arithmetic), median of 20; the compulsory bytes, 36 B per cell, at the copy rate measured with one device-to-device
hipMemcpy of 1 GiB through torch (read + write counted).  The batch leg: 8 members of 128^2, 4000 steps per call."""
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
    eng.set_stats(0)


def stats(every, steps):
    def arm(eng):
        eng.set_stats(every, -(-steps // every))
    return arm


def host_row(cells, fluid):
    f = cells
    with np.errstate(all="ignore"):
        rho = f[..., 0].copy()
        for k in range(1, 9):
            rho += f[..., k]
        jx = ((f[..., 1] + f[..., 5]) + f[..., 8]) - ((f[..., 3] + f[..., 6]) + f[..., 7])
        jy = ((f[..., 2] + f[..., 5]) + f[..., 6]) - ((f[..., 4] + f[..., 7]) + f[..., 8])
        ux, uy = jx / rho, jy / rho
        usq = ux * ux + uy * uy
    ok = np.isfinite(rho) & (~fluid | (np.isfinite(jx) & np.isfinite(jy) & np.isfinite(usq)))
    both = ok & fluid
    at = int(np.argmax(np.where(both, usq, -1.0)))
    return (float(rho.sum(dtype=np.float64, where=ok)), float(jx.sum(dtype=np.float64, where=both)),
            float(jy.sum(dtype=np.float64, where=both)), float(usq.sum(dtype=np.float64, where=both)), int((~ok).sum()), at)


def loop(eng, steps, every, fluid):
    unarmed(eng)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(steps // every):
        eng.run(every)
        host_row(eng.cells(), fluid)
    return (time.perf_counter() - t0) / (steps // every * every) * 1e6


def one_sample_us(eng, calls=50):
    t = {}
    for label, arm in (("unarmed", unarmed), ("armed", stats(1, calls))):
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


def total_density_us(eng, repeats=20):
    unarmed(eng)
    eng.sync()
    samples = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        eng.total_density()
        samples.append(time.perf_counter() - t0)
    return statistics.median(samples[1:]) * 1e6


def copy_rate():
    """bytes per second of a device-to-device copy, read + write counted; None without torch"""
    try:
        import torch
        a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
        b = torch.empty_like(a)
        samples = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.copy_(a)
            torch.cuda.synchronize()
            samples.append(time.perf_counter() - t0)
        del a, b
        torch.cuda.empty_cache()
        return 2.0 * (1 << 30) / min(samples[1:])
    except Exception as exc:  # noqa: BLE001
        print("copy rate not measured:", exc)
        return None


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
        for label, every in (("unarmed", 0), ("unarmed again", 0), ("stats every 100", 100), ("stats every 1", 1)):
            samples = []
            for i in range(4):
                batch.set_stats(every, -(-steps // every) if every else 0)
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
    rate = copy_rate()
    if rate:
        print(f"device copy rate (read + write): {rate / 1e12:.3f} TB/s", flush=True)
    for n in [int(v) for v in args.sizes.split(",")]:
        steps = {128: 4000, 1024: 1000}.get(n, 100)
        p, ob, tiled, fluid = case(lbm, n, steps)
        with lbm.Engine(p, ob, tiled=tiled) as eng:
            resident = "yes" if eng.info()["resident_steps"] else "no"
            for every in (100, 1):
                cols = [("unarmed", unarmed), ("unarmed again", unarmed), ("stats", stats(every, steps))]
                t = {label: timed(eng, steps, arm) for label, arm in cols}
                t["run+cells+numpy loop"] = loop(eng, steps if every > 1 else (steps // 20 if n < 8192 else 2), every, fluid)
                base = t["unarmed"]
                print(f"{n:>5}^2 every {every:>3} ({steps} steps per call): us/step  "
                      + "  ".join(f"{label} {v:10.3f} ({v / base:7.3f}x)" for label, v in t.items())
                      + f"  [resident {resident}]", flush=True)
            gather, step1 = one_sample_us(eng)
            density = total_density_us(eng)
            bytes_us = 36.0 * n * n / rate * 1e6 if rate else float("nan")
            print(f"{n:>5}^2 one sample (memset + stats_gather): {gather:9.2f} us  (run(1) unarmed {step1:9.2f} us)   one lbm_total_density call: "
                  f"{density:9.2f} us   ratio {gather / density:6.3f}   36 B/cell at the copy rate: {bytes_us:9.2f} us", flush=True)
    batch_leg(lbm)


if __name__ == "__main__":
    main()
