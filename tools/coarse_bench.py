"""us per timestep with the coarse frames armed (Engine.set_coarse_frames) against the same engine unarmed, the time of
one sample next to a columns-only sample of the line profiles and to the compulsory bytes, and the bytes of a frame that
cross the host link; same process.
python tools/coarse_bench.py [--sizes 128,1024,8192]

The reference's 128^2 and 1024^2 data sets and the benchmark's 8192^2 grid (the 1024^2 obstacle map tiled 8 x 8): calls
of N timesteps (4000, 1000, 100), median of 5 timed calls (run + sync) each after one warm-up call; the recorder is
re-armed outside the timed region before every call, so the ring is never drained inside it.  Columns at every = 100:
unarmed (twice, back to back: their spread is the noise of the box), then the boxes 4x4, 16x16, 33x16 (31 of a wave's 64
lanes idle in x: one box of 33 columns per wave) and 128x128 (a workgroup per box, the waves meet in LDS).
One sample: 50 calls of run(1) armed at every = 1 (fewer where 50 frames would not fit the ring: 10 at 8192^2 with 4x4
boxes) against 50 unarmed, the difference per call (one memset of the slot and one launch), for each box; the yardstick
is the same difference with the line profiles armed on their columns alone (profile_columns, a kernel this tree does
not change): the same bytes read with the same access pattern and the same per-cell arithmetic.  Beside them the compulsory bytes, 37 B per cell (nine populations and the mask byte), at the copy
rate the statistics' bench measured on this device with one device-to-device copy of 1 GiB (4.733 TB/s, read + write
counted).  Host link: the bytes lbm_read_coarse_frames copies per frame (48 per box on one slab) and the time of
draining one frame, next to the bytes of a four-field lbm_set_field_frames frame of the whole grid (16 per cell)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402

COPY_RATE = 4.733e12          # bytes per second, profiles/stats_bench.log
BOXES = ((4, 4), (16, 16), (33, 16), (128, 128))


def label(box):
    return "%dx%d" % box


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
    eng.set_coarse_frames(0)
    eng.set_profiles(0)


def coarse(every, steps, box):
    def arm(eng):
        eng.set_profiles(0)
        eng.set_coarse_frames(every, -(-steps // every), box)
    return arm


def columns(every, steps):
    def arm(eng):
        eng.set_coarse_frames(0)
        eng.set_profiles(every, -(-steps // every), ("columns",))
    return arm


def idle_fraction(nx, box):
    """lanes of coarse_gather that own no column, of all its lanes: a wave takes floor(64 / bx) boxes of bx <= 64 columns,
    a workgroup of 256 lanes one box of more"""
    bx = box[0]
    cx = -(-nx // bx)
    if bx > 64:
        return 1.0 - nx / (cx * 256.0)
    spans = -(-cx // (64 // bx))
    return 1.0 - nx / (spans * 64.0)


def one_sample_us(eng, boxes, calls=50):
    """(a box's ring holds a frame per call: fewer calls where 50 frames would reach the ring's 2 GiB)"""
    nx, ny = eng.params.nx, eng.params.ny
    fit = lambda b: max(1, min(calls, (2 ** 31 - 1) // (48 * -(-nx // b[0]) * -(-ny // b[1]))))  # noqa: E731
    t = {}
    for name, arm, n in [("unarmed", unarmed, calls), ("columns", columns(1, calls), calls)] + [(label(b), coarse(1, fit(b), b), fit(b)) for b in boxes]:
        samples = []
        for i in range(4):
            arm(eng)
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                eng.run(1)
            eng.sync()
            if i:
                samples.append(time.perf_counter() - t0)
        t[name] = statistics.median(samples) / n * 1e6
    return {name: v - t["unarmed"] for name, v in t.items() if name != "unarmed"}, t["unarmed"]


def drain_us(eng, box):
    """the time of lbm_read_coarse_frames for one waiting frame: the copy over the host link and words -> frame"""
    samples = []
    for _ in range(4):
        eng.set_coarse_frames(1, 1, box)
        eng.run(1)
        eng.sync()
        t0 = time.perf_counter()
        steps, frames = eng.coarse_frames()
        samples.append(time.perf_counter() - t0)
        assert len(steps) == 1
    eng.set_coarse_frames(0)
    return statistics.median(samples[1:]) * 1e6, frames[0].nbytes


def case(lbm, n, calls):
    if n == 8192:
        tile = lbm.read_obstacles(os.path.join(conftest.GOLDEN, "inputs", "obstacles_1024x1024.dat"), 1024, 1024)
        p = lbm.Params(n, n, 200 * calls, 10, 0.1, 0.01, 1.85)
        return p, tile, True
    p, ob = conftest.dataset(f"{n}x{n}")
    p.max_iters = 200 * calls
    return p, ob, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,1024,8192")
    args = ap.parse_args()
    lbm = conftest.load_package()
    every = 100
    for n in [int(v) for v in args.sizes.split(",")]:
        steps = {128: 4000, 1024: 1000}.get(n, 100)
        p, ob, tiled = case(lbm, n, steps)
        boxes = [b for b in BOXES if b[0] <= n and b[1] <= n]
        with lbm.Engine(p, ob, tiled=tiled) as eng:
            resident = "yes" if eng.info()["resident_steps"] else "no"
            cols = [("unarmed", unarmed), ("unarmed again", unarmed)] + [(label(b), coarse(every, steps, b)) for b in boxes]
            t = {name: timed(eng, steps, arm) for name, arm in cols}
            base = t["unarmed"]
            print(f"{n:>5}^2 every {every:>3} ({steps} steps per call): us/step  "
                  + "  ".join(f"{name} {v:10.3f} ({v / base:7.3f}x)" for name, v in t.items())
                  + f"  [resident {resident}]", flush=True)
            sample, step1 = one_sample_us(eng, boxes)
            bytes_us = 37.0 * n * n / COPY_RATE * 1e6
            yard = sample["columns"]
            print(f"{n:>5}^2 one sample (memset + launch): profile columns alone {yard:9.2f} us ({yard / bytes_us:6.2f}x its bytes)  "
                  + "  ".join(f"{label(b)} {sample[label(b)]:9.2f} us ({sample[label(b)] / yard:6.3f}x columns, {sample[label(b)] / bytes_us:6.2f}x its bytes, "
                              f"idle lanes {100 * idle_fraction(n, b):4.1f} %)" for b in boxes)
                  + f"  (run(1) unarmed {step1:9.2f} us)   37 B/cell at the copy rate: {bytes_us:9.2f} us", flush=True)
            field_frame = 16 * n * n
            for b in boxes:
                us, nbytes = drain_us(eng, b)
                print(f"{n:>5}^2 host link, box {label(b):>7}: {nbytes:>12} B per frame ({field_frame / nbytes:9.1f}x fewer than the {field_frame} B of a "
                      f"four-field lbm_set_field_frames frame), one frame drained in {us:10.1f} us", flush=True)


if __name__ == "__main__":
    main()
