"""us per timestep with field frames armed (Engine.set_field_frames) against the same engine unarmed, against animation
frames at the same interval, and against the loop of run(every) + final_state() that field frames replace; same process.
python tools/fields_bench.py [--steps N]

Resident shapes (the reference's 128^2, 256^2, 1024^2 data sets): calls of N timesteps (default 4000), median of 5 timed
calls (run + sync) each after one warm-up call; the recorder is re-armed outside the timed region before every call, so
the ring (one slot per sample of a call) is never drained inside it.  Columns, each at every = 100 and every = 1: unarmed
(twice, back to back: their spread is the noise of the box), frames (lbm_set_frames), field frames with |u| only on the whole
grid, all four fields on the whole grid, all four fields on a one-column window (the vertical centreline).  The loop
run(every) + final_state() is timed over N steps at every = 100 and over N / 20 steps at every = 1 (one call of each)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import conftest  # noqa: E402

ALL = ("u_x", "u_y", "u", "pressure")


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
    eng.set_frames(0)
    eng.set_field_frames(0)


def frames(every, steps):
    def arm(eng):
        eng.set_field_frames(0)
        eng.set_frames(every, -(-steps // every))
    return arm


def fields(every, steps, names, window):
    def arm(eng):
        eng.set_frames(0)
        eng.set_field_frames(every, -(-steps // every), names, window)
    return arm


def loop(eng, steps, every):
    unarmed(eng)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(steps // every):
        eng.run(every)
        eng.final_state()
    return (time.perf_counter() - t0) / (steps // every * every) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    args = ap.parse_args()
    lbm = conftest.load_package()
    steps = args.steps
    for name in ("128x128", "256x256", "1024x1024"):
        p, ob = conftest.dataset(name)
        p.max_iters = 80 * steps
        column = (p.nx // 2, 0, 1, p.ny)
        with lbm.Engine(p, ob) as eng:
            resident = "yes" if eng.info()["resident_steps"] else "no"
            for every in (100, 1):
                # a whole-grid ring of four fields at every = 1 holds one frame per step: fewer steps per call where
                # 4000 of them would not fit 4 GiB
                n = steps if every > 1 else min(steps, (4 << 30) // (16 * p.nx * p.ny))
                cols = [("unarmed", unarmed), ("unarmed again", unarmed), ("frames", frames(every, n)),
                        ("fields |u|", fields(every, n, ("u",), None)), ("fields all", fields(every, n, ALL, None)),
                        ("fields all, column", fields(every, n, ALL, column))]
                t = {label: timed(eng, n, arm) for label, arm in cols}
                loop_steps = n if every > 1 else max(every, n // 20)
                t["run+final_state loop"] = loop(eng, loop_steps, every)
                base = t["unarmed"]
                print(f"{name:>10} every {every:>3} ({n} steps per call): us/step  "
                      + "  ".join(f"{label} {v:8.3f} ({v / base:6.3f}x)" for label, v in t.items())
                      + f"  [resident {resident}]", flush=True)


if __name__ == "__main__":
    main()
