"""us per timestep of a batch (lbm.Batch: B lattices advanced together) against ONE member run alone, same process.
python tools/batch_bench.py [--steps N] [--case BxNXxNY ...]

Per case: median of 5 timed repeats, after one warm-up call, of batch.run(N) + sync (and of Engine.run(N) + sync for
the single member); aggregate MLUPS = B * nx * ny / us per batched step; speed-up = B x single us / batched us, i.e. the
throughput of the batch over that of sequential single runs.  Members differ in omega and accel; the obstacle map is
the reference's where it has a data set of that size, else walls on all four sides."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import conftest  # noqa: E402

CASES = ("8x128x128", "16x128x128", "8x64x64", "2x256x256", "4x128x256", "8x1024x64", "2x1024x1024")


def obstacles(nx, ny):
    try:
        _, ob = conftest.dataset(f"{nx}x{ny}")
        return ob
    except OSError:
        ob = np.zeros((ny, nx), dtype=np.int32)
        ob[0, :] = ob[-1, :] = ob[:, 0] = ob[:, -1] = 1
        return ob


def timed(run, sync, steps, repeats=5):
    run(steps)
    sync()
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(steps)
        sync()
        samples.append(time.perf_counter() - t0)
    return statistics.median(samples) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--case", action="append", help="BxNXxNY (default: all of %s)" % ", ".join(CASES))
    args = ap.parse_args()
    lbm = conftest.load_package()
    for case in args.case or CASES:
        b, nx, ny = (int(v) for v in case.split("x"))
        ob = obstacles(nx, ny)
        params = [lbm.Params(nx, ny, 7 * args.steps, nx, 0.1, float(np.float32(0.005 + 0.001 * (i % 8))),
                             float(np.float32(1.7 + 0.02 * (i % 8)))) for i in range(b)]
        with lbm.Engine(params[0], ob) as eng:
            single = timed(eng.run, eng.sync, args.steps)
        with lbm.Batch(params, [ob] * b) as batch:
            info = batch.info()
            batched = timed(batch.run, batch.sync, args.steps)
        mlups = b * nx * ny / batched
        print(f"{case:>12}: batch {batched:8.3f} us/step  single {single:8.3f} us/step  aggregate {mlups:9.0f} MLUPS "
              f"(single {nx * ny / single:8.0f})  speed-up x{b * single / batched:5.2f}  "
              f"[{info['members_per_launch']} members per launch, {info['launches_per_chunk']} launches per chunk, "
              f"resident {'yes' if info['resident_steps'] else 'no'}]", flush=True)


if __name__ == "__main__":
    main()
