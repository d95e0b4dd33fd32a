"""us per batched timestep with the obstacle forces armed on a batch (Batch.set_forces) against the same batch unarmed, and
against what gives the same series without it: B single engines armed with Engine.set_forces, run one after the other;
same process.
python tools/forces_batch_bench.py [--steps N]

8 x 128^2 and 2 x 1024^2, every member the reference's data set with its own obstacles (all blocked cells one body):
calls of N timesteps (default 4000), median of 5 timed calls (run + sync) each after one warm-up call; the recorder is
re-armed outside the timed region before every call, so the ring is never drained inside it.  Columns, each at every = 100
and every = 1, in us per batched step (one step of all B members): (a) the batch unarmed, (b) the batch armed, (c) the B
single engines armed, the sum of their calls; then (c) / (b).  The second line gives the cost of one sample, (armed -
unarmed) * every: the batch's for all B series, ONE single engine's for its one, and their ratio -- at 8 x 128^2 and
every = 100 the figure the batch forces were built to keep at or below 1.25."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import conftest  # noqa: E402
import forces_model  # noqa: E402


def timed(engines, steps, every, repeats=5):
    """median over the timed calls of the summed run + sync time of `engines` (a batch, or single engines in turn), us per step"""
    samples = []
    for i in range(repeats + 1):
        for eng in engines:
            eng.set_forces(every, -(-steps // every) if every else 4096)    # (every == 0 disarms)
            eng.sync()
        total = 0.0
        for eng in engines:
            t0 = time.perf_counter()
            eng.run(steps)
            eng.sync()
            total += time.perf_counter() - t0
        if i:
            samples.append(total)
    return statistics.median(samples) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    args = ap.parse_args()
    lbm = conftest.load_package()
    steps = args.steps
    for name, members in (("128x128", 8), ("1024x1024", 2)):
        p, ob = conftest.dataset(name)
        p.max_iters = 40 * steps
        n_links = len(forces_model.links(np.asarray(ob).reshape(p.ny, p.nx)))
        with lbm.Batch([p] * members, [ob] * members) as batch:
            engines = [lbm.Engine(p, ob) for _ in range(members)]
            try:
                batch.set_forces(100, 1)
                assert batch.force_links().tolist() == [[n_links]] * members
                info = batch.info()
                for every in (100, 1):
                    a = timed([batch], steps, 0)
                    b = timed([batch], steps, every)
                    c = timed(engines, steps, every)
                    one_unarmed = timed(engines[:1], steps, 0)
                    one_armed = timed(engines[:1], steps, every)
                    batch_sample, one_sample = (b - a) * every, (one_armed - one_unarmed) * every
                    print(f"{members} x {name:>9} every {every:>3} ({steps} steps per call, {n_links} links per member, "
                          f"{info['members_per_launch']} members per launch): us per batched step  (a) batch unarmed {a:8.3f}  "
                          f"(b) batch armed {b:8.3f}  (c) {members} single engines armed, in turn {c:8.3f}  (c)/(b) {c / b:6.2f}x", flush=True)
                    print(f"{'':>15} us per sample: batch (b - a) * {every} = {batch_sample:8.2f} for {members} series;  one single engine "
                          f"({one_armed:.3f} - {one_unarmed:.3f}) * {every} = {one_sample:8.2f} for one;  batch / single {batch_sample / one_sample:5.2f}",
                          flush=True)
            finally:
                for eng in engines:
                    eng.close()


if __name__ == "__main__":
    main()
