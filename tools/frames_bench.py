"""us per timestep with animation frames armed (Engine.set_frames) against the same engine unarmed, same process.
python tools/frames_bench.py [--steps N]

Resident shapes (the reference's 128^2, 256^2, 1024^2 data sets): calls of N timesteps (default 4000), unarmed and
every = 100, 10, 1, median of 5 timed calls (run + sync) each after one warm-up call; the frame buffer is re-armed
(emptied) outside the timed region before every call.  Then 4096^2 (the 1024^2 map tiled) on the per-pass kernels,
unarmed and every = 100, N / 4 timesteps per call."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import conftest  # noqa: E402


def timed(eng, steps, every, repeats=5):
    samples = []
    for i in range(repeats + 1):
        eng.set_frames(every, -(-steps // every) if every else 0)
        eng.sync()
        t0 = time.perf_counter()
        eng.run(steps)
        eng.sync()
        if i:
            samples.append(time.perf_counter() - t0)
    return statistics.median(samples) / steps * 1e6


def row(eng, label, steps, everys):
    base = timed(eng, steps, 0)
    parts = [f"unarmed {base:8.3f}"]
    for e in everys:
        t = timed(eng, steps, e)
        parts.append(f"every {e:>3} {t:8.3f} ({t / base:5.3f}x)")
    info = eng.info()
    print(f"{label:>10}: us/step  " + "  ".join(parts) + f"  [resident {'yes' if info['resident_steps'] else 'no'}]",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    args = ap.parse_args()
    lbm = conftest.load_package()
    for name in ("128x128", "256x256", "1024x1024"):
        p, ob = conftest.dataset(name)
        p.max_iters = 30 * args.steps
        with lbm.Engine(p, ob) as eng:
            row(eng, name, args.steps, (100, 10, 1))
    p, ob = conftest.dataset("1024x1024")
    steps = args.steps // 4
    big = lbm.Params(4096, 4096, 20 * steps, p.reynolds_dim, p.density, p.accel, p.omega)
    with lbm.Engine(big, lbm.tile_obstacles(ob, 4096, 4096)) as eng:
        row(eng, "4096x4096", steps, (100,))


if __name__ == "__main__":
    main()
