"""us per timestep with the obstacle forces armed (Engine.set_forces) against the same engine unarmed, and against the
only other way to the same series: the loop of run(every) + cells() + the host's sum over the boundary links; same process.
python tools/forces_bench.py [--steps N]

The reference's 128^2 and 1024^2 data sets with their own obstacles (all blocked cells one body): calls of N timesteps
(default 4000), median of 5 timed calls (run + sync) each after one warm-up call; the recorder is re-armed outside the
timed region before every call (which also rebuilds the link list there), so the ring is never drained inside it.  Columns,
each at every = 100 and every = 1: unarmed (twice, back to back: their spread is the noise of the box), forces, and the
host loop, timed over N steps at every = 100 and over N / 20 steps at every = 1 (one call of each).  The host loop gathers
the populations on the links with one numpy index (the list is built once, outside the timed region) and sums them with
math.fsum, the value the engine gives."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import conftest  # noqa: E402
import forces_model  # noqa: E402


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
    eng.set_forces(0)


def forces(every, steps):
    def arm(eng):
        eng.set_forces(every, -(-steps // every))
    return arm


def loop(eng, steps, every, index, wx, wy):
    unarmed(eng)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(steps // every):
        eng.run(every)
        f = eng.cells().reshape(-1)[index].astype(np.float64)
        math.fsum(wx * f), math.fsum(wy * f)
    return (time.perf_counter() - t0) / (steps // every * every) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    args = ap.parse_args()
    lbm = conftest.load_package()
    steps = args.steps
    for name in ("128x128", "1024x1024"):
        p, ob = conftest.dataset(name)
        p.max_iters = 80 * steps
        ob2 = np.asarray(ob).reshape(p.ny, p.nx)
        links = forces_model.links(ob2)
        index = np.array([(y * p.nx + x) * 9 + k for _, y, x, k in links], dtype=np.int64)
        wx = np.array([-2.0 * forces_model.CX[k] for _, _, _, k in links])
        wy = np.array([-2.0 * forces_model.CY[k] for _, _, _, k in links])
        with lbm.Engine(p, ob) as eng:
            resident = "yes" if eng.info()["resident_steps"] else "no"
            eng.set_forces(100, 1)
            assert int(eng.force_links()[0]) == len(links)
            for every in (100, 1):
                cols = [("unarmed", unarmed), ("unarmed again", unarmed), ("forces", forces(every, steps))]
                t = {label: timed(eng, steps, arm) for label, arm in cols}
                t["run+cells+host sum loop"] = loop(eng, steps if every > 1 else max(every, steps // 20), every, index, wx, wy)
                base = t["unarmed"]
                print(f"{name:>10} every {every:>3} ({steps} steps per call, {len(links)} links): us/step  "
                      + "  ".join(f"{label} {v:8.3f} ({v / base:6.3f}x)" for label, v in t.items())
                      + f"  [resident {resident}]", flush=True)


if __name__ == "__main__":
    main()
