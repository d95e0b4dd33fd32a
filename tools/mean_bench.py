"""us per timestep with the mean fields armed (Engine.set_mean) against the same engine unarmed and against animation
frames at the same interval, same process.
python tools/mean_bench.py [--steps N]

Resident shapes (the reference's 128^2, 256^2, 1024^2 data sets): calls of N timesteps (default 4000), median of 5 timed
calls (run + sync) each after one warm-up call; the recorder is re-armed outside the timed region before every call.
Columns: unarmed (twice, back to back: their spread is the noise of the box), mean at every = 100, 10 and 1, the same at
order 2 (set_mean_order: the second moments, "mean2"), frames at every = 100 and 1.  Then 4096^2 (the 1024^2 map tiled) on
the per-pass kernels, N / 4 timesteps per call: unarmed, mean and mean2 at every = 100 and every = 4."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
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
    eng.set_mean(0)
    eng.set_frames(0)


def mean(every, order=1):
    def arm(eng):
        eng.set_frames(0)
        eng.set_mean_order(every, order)
    return arm


def frames(every, steps):
    def arm(eng):
        eng.set_mean(0)
        eng.set_frames(every, -(-steps // every))
    return arm


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
            cols = [("unarmed", unarmed), ("unarmed again", unarmed), ("mean /100", mean(100)), ("mean /10", mean(10)),
                    ("mean /1", mean(1)), ("mean2 /100", mean(100, 2)), ("mean2 /10", mean(10, 2)), ("mean2 /1", mean(1, 2)),
                    ("frames /100", frames(100, steps)), ("frames /1", frames(1, steps))]
            t = {label: timed(eng, steps, arm) for label, arm in cols}
            base = t["unarmed"]
            print(f"{name:>10}: us/step  " + "  ".join(f"{label} {v:7.3f} ({v / base:5.3f}x)" for label, v in t.items())
                  + f"  [resident {'yes' if eng.info()['resident_steps'] else 'no'}]", flush=True)
            spread = abs(t["unarmed again"] - t["unarmed"])
            a, b = t["mean /100"] - base, t["frames /100"] - base
            print(f"{'':>10}  over unarmed at every 100: mean {a:+7.3f}, frames {b:+7.3f}, spread of unarmed {spread:5.3f}: "
                  f"{'mean costs no more than frames' if a <= b + spread else 'MEAN COSTS MORE by %.3f us' % (a - b)}", flush=True)
    p, ob = conftest.dataset("1024x1024")
    big_steps = steps // 4
    big = lbm.Params(4096, 4096, 40 * big_steps, p.reynolds_dim, p.density, p.accel, p.omega)
    with lbm.Engine(big, lbm.tile_obstacles(ob, 4096, 4096)) as eng:
        t = {label: timed(eng, big_steps, arm) for label, arm in
             (("unarmed", unarmed), ("mean /100", mean(100)), ("mean /4", mean(4)), ("mean2 /100", mean(100, 2)),
              ("mean2 /4", mean(4, 2)))}
        print(f"{'4096x4096':>10}: us/step  " + "  ".join(f"{label} {v:8.3f} ({v / t['unarmed']:5.3f}x)" for label, v in t.items())
              + f"  [resident {'yes' if eng.info()['resident_steps'] else 'no'}]", flush=True)


if __name__ == "__main__":
    main()
