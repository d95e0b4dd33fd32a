"""us per timestep with point probes armed (Engine.set_probes) against the same engine unarmed and against animation
frames at the same interval, same process.
python tools/probes_bench.py [--steps N]

Resident shapes (the reference's 128^2, 256^2, 1024^2 data sets): calls of N timesteps (default 4000), median of 5 timed
calls (run + sync) each after one warm-up call; the recorder is re-armed (its ring emptied) outside the timed region
before every call.  Columns: unarmed (twice, back to back: their spread is the noise of the box), 1 / 16 / 256 probes
at every = 1, 16 probes at every = 100, frames at every = 1 and 100.  Then 4096^2 (the 1024^2 map tiled) on the per-pass
kernels, N / 4 timesteps per call: unarmed, 16 probes at every = 100 and every = 4.  Last, the same series obtained
without probes -- a loop of run(1) + final_state() -- over N / 2 steps at 128^2 and 1024^2."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import conftest  # noqa: E402


def cells_for(p, n):
    rng = np.random.default_rng(1)
    cells = [(int(x), int(y)) for x, y in zip(rng.integers(0, p.nx, n), rng.integers(0, p.ny, n))]
    cells[0] = (p.nx // 2, p.ny - 2)      # one probe on the lid row: its band defers the lid's acceleration
    return cells


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
    eng.set_probes([], 0)
    eng.set_frames(0)


def probes(p, n, every, steps):
    cells = cells_for(p, n)

    def arm(eng):
        eng.set_frames(0)
        eng.set_probes(cells, every, -(-steps // every))
    return arm


def frames(every, steps):
    def arm(eng):
        eng.set_probes([], 0)
        eng.set_frames(every, -(-steps // every))
    return arm


def loop_series(eng, cells, steps):
    """The series the way an engine without probes gives it: one call and one read of the four fields per step."""
    xs = np.array([c[0] for c in cells])
    ys = np.array([c[1] for c in cells])
    out = np.empty((steps, len(cells), 4), dtype=np.float32)
    t0 = time.perf_counter()
    for t in range(steps):
        eng.run(1)
        f = eng.final_state()
        for k, name in enumerate(("u_x", "u_y", "u", "pressure")):
            out[t, :, k] = f[name][ys, xs]
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    args = ap.parse_args()
    lbm = conftest.load_package()
    steps = args.steps
    for name in ("128x128", "256x256", "1024x1024"):
        p, ob = conftest.dataset(name)
        p.max_iters = 60 * steps
        with lbm.Engine(p, ob) as eng:
            cols = [("unarmed", unarmed), ("unarmed again", unarmed), ("1 probe /1", probes(p, 1, 1, steps)),
                    ("16 probes /1", probes(p, 16, 1, steps)), ("256 probes /1", probes(p, 256, 1, steps)),
                    ("16 probes /100", probes(p, 16, 100, steps)), ("frames /1", frames(1, steps)),
                    ("frames /100", frames(100, steps))]
            t = {label: timed(eng, steps, arm) for label, arm in cols}
            base = t["unarmed"]
            print(f"{name:>10}: us/step  " + "  ".join(f"{label} {v:7.3f} ({v / base:5.3f}x)" for label, v in t.items())
                  + f"  [resident {'yes' if eng.info()['resident_steps'] else 'no'}]", flush=True)
            spread = abs(t["unarmed again"] - t["unarmed"])
            for e in (1, 100):
                a, b = t[f"16 probes /{e}"], t[f"frames /{e}"]
                print(f"{'':>10}  bound, every {e:>3}: 16 probes {a:7.3f} <= frames {b:7.3f} + spread {spread:5.3f}: "
                      f"{'met' if a <= b + spread else 'MISSED by %.3f us' % (a - b - spread)}", flush=True)
    p, ob = conftest.dataset("1024x1024")
    big_steps = steps // 4
    big = lbm.Params(4096, 4096, 40 * big_steps, p.reynolds_dim, p.density, p.accel, p.omega)
    with lbm.Engine(big, lbm.tile_obstacles(ob, 4096, 4096)) as eng:
        t = {label: timed(eng, big_steps, arm) for label, arm in
             (("unarmed", unarmed), ("16 probes /100", probes(big, 16, 100, big_steps)), ("16 probes /4", probes(big, 16, 4, big_steps)))}
        print(f"{'4096x4096':>10}: us/step  " + "  ".join(f"{label} {v:8.3f} ({v / t['unarmed']:5.3f}x)" for label, v in t.items())
              + f"  [resident {'yes' if eng.info()['resident_steps'] else 'no'}]", flush=True)
    for name in ("128x128", "1024x1024"):
        p, ob = conftest.dataset(name)
        n = steps // 2
        p.max_iters = 4 * n
        cells = cells_for(p, 16)
        with lbm.Engine(p, ob) as eng:
            loop = loop_series(eng, cells, n)
            probes(p, 16, 1, n)(eng)
            eng.sync()
            t0 = time.perf_counter()
            eng.run(n)
            got = eng.probes()[1]          # synchronises and drains the ring: part of obtaining the series
            armed = (time.perf_counter() - t0) / n * 1e6
            assert got.shape == (n, 16, 4)
            print(f"{name:>10}: the per-step series of 16 probes over {n} steps: run(1) + final_state() loop {loop:9.2f} us/step, "
                  f"probes (run + drain) {armed:7.3f} us/step, ratio {loop / armed:7.1f}x", flush=True)


if __name__ == "__main__":
    main()
