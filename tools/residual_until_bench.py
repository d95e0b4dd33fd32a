"""What a residual-steady run costs over a plain run, next to the average-velocity check and to one armed residual sample.
python tools/residual_until_bench.py [--steps N] [--every E] [--sizes 128,1024] [--kernels-only]

For the reference's 128^2 and 1024^2 data sets, in one process and on one engine: wall time per timestep of
  run_until_residual(N, E, tol=0)   -- a tol the run does not meet, so all N (default 32768) steps run, in N / E segments
                                       (E default 1024) with one sample and one check behind each;
  run(N) + sync();
  run_until(N, E, tol=0)            -- the check on the mean of av_vels;
  run(N) + sync() with the residual recorder armed at every = E (re-armed outside the timed region);
median of 5 timed calls each after one warm-up call of each kind (tools/steady_bench.py's repeats), the overhead over
run(N) in per cent, and what one check costs (the difference to run(N), divided by N / E).
One armed sample (tools/residual_bench.py's figure): 50 calls of run(1) armed at every = 1 against 50 unarmed, the
difference per call: one memset and one residual_gather.
--kernels-only: one short run_until_residual per size and nothing else, for a kernel trace of residual_gather_unless and
residual_check (whose duration is the device rounding of the two sums, on one lane each, plus the verdict)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import conftest  # noqa: E402


def timed(call, repeats=5, before=None):
    samples = []
    for i in range(repeats + 1):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        if i:
            samples.append(time.perf_counter() - t0)
    return statistics.median(samples)


def one_sample_us(eng, calls=50):
    t = {}
    for label, every in (("unarmed", 0), ("armed", 1)):
        samples = []
        for i in range(4):
            eng.set_residual(every, calls if every else 0)
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                eng.run(1)
            eng.sync()
            if i:
                samples.append(time.perf_counter() - t0)
        t[label] = statistics.median(samples) / calls * 1e6
    eng.set_residual(0)
    return t["armed"] - t["unarmed"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32768)
    ap.add_argument("--every", type=int, default=1024)
    ap.add_argument("--sizes", default="128,1024")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    lbm = conftest.load_package()
    n, every = args.steps, args.every
    checks = n // every
    if not args.kernels_only:
        print(f"per timestep, {n} steps per call, check_every = {every} ({checks} checks), tol = 0 (never met), median of 5", flush=True)
    for size in [int(v) for v in args.sizes.split(",")]:
        p, ob = conftest.dataset(f"{size}x{size}")
        p.max_iters = 30 * n + 1000
        with lbm.Engine(p, ob) as eng:
            if args.kernels_only:
                res = eng.run_until_residual(8 * every, every, 0.0, 2)
                assert res["checks"] == 8 and not res["steady"], res
                continue

            def plain():
                eng.run(n)
                eng.sync()

            def residual():
                res = eng.run_until_residual(n, every, 0.0, 2, history=0)
                assert not res["steady"] and not res["diverged"] and res["steps_run"] == n and res["checks"] == checks, res

            def mean():
                res = eng.run_until(n, every, 0.0, 2)
                assert not res["steady"] and res["steps_run"] == n, res

            def arm():
                eng.set_residual(0)
                # the recorder samples after the steps tt with tt % every == 0
                eng.set_residual(every, checks + 1)
                eng.sync()

            t = {"run": timed(plain), "run again": timed(plain), "run_until_residual": timed(residual), "run_until": timed(mean),
                 "run, recorder armed": timed(plain, before=arm)}
            eng.set_residual(0)
            base = t["run"]
            resident = "yes" if eng.info()["resident_steps"] else "no"
            print(f"{size:>5}^2 [resident {resident}]: " + "   ".join(f"{k} {v / n * 1e6:8.3f} us/step ({(v / base - 1) * 100:+6.2f} %)" for k, v in t.items()),
                  flush=True)
            sample = one_sample_us(eng)
            print(f"{size:>5}^2 one check: run_until_residual {(t['run_until_residual'] - base) / checks * 1e6:8.2f} us   "
                  f"run_until {(t['run_until'] - base) / checks * 1e6:8.2f} us   recorder armed {(t['run, recorder armed'] - base) / checks * 1e6:8.2f} us   "
                  f"one armed sample (run(1) armed - unarmed, memset + gather) {sample:8.2f} us   "
                  f"noise: the two plain runs differ by {abs(t['run again'] - base) / checks * 1e6:8.2f} us per check", flush=True)


if __name__ == "__main__":
    main()
