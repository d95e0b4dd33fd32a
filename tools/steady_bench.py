"""What the steady-state check costs, and where the reference's data sets become steady.
python tools/steady_bench.py [--steps N] [--cap N]

Overhead: for 128^2 and 1024^2, wall time of Engine.run_until(N, check_every=1024, tol=0) -- a tol the run does not meet,
so all N (default 32768) steps run, in N / 1024 segments with a check behind each -- against run(N) + sync() on the same
engine, median of 5 timed calls each after one warm-up call of each kind.
Steady state: the four data sets with maxIters raised to --cap (default 2000000): after how many steps run_until(cap,
1024, 1e-5, 2) stops, how long that takes, and the Reynolds number there."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import conftest  # noqa: E402


def timed(call, repeats=5):
    samples = []
    for i in range(repeats + 1):
        t0 = time.perf_counter()
        call()
        if i:
            samples.append(time.perf_counter() - t0)
    return statistics.median(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32768)
    ap.add_argument("--cap", type=int, default=2000000)
    args = ap.parse_args()
    lbm = conftest.load_package()
    n = args.steps
    print(f"overhead: run_until({n}, check_every=1024, tol=0) against run({n}) + sync(), median of 5", flush=True)
    for name in ("128x128", "1024x1024"):
        p, ob = conftest.dataset(name)
        p.max_iters = 12 * n
        with lbm.Engine(p, ob) as eng:
            def plain():
                eng.run(n)
                eng.sync()

            def until():
                res = eng.run_until(n, 1024, 0.0, 2)
                assert not res["steady"] and res["steps_run"] == n, res

            base = timed(plain)
            checked = timed(until)
            print(f"{name:>10}: run {base / n * 1e6:7.3f} us/step   run_until {checked / n * 1e6:7.3f} us/step   "
                  f"ratio {checked / base:6.4f}  [resident {'yes' if eng.info()['resident_steps'] else 'no'}]", flush=True)
    print(f"steady state: run_until({args.cap}, check_every=1024, tol=1e-5, patience=2)", flush=True)
    for name in ("128x128", "128x256", "256x256", "1024x1024"):
        p, ob = conftest.dataset(name)
        iters = p.max_iters
        p.max_iters = args.cap
        with lbm.Engine(p, ob) as eng:
            eng.sync()
            t0 = time.perf_counter()
            res = eng.run_until(args.cap, 1024, 1e-5, 2)
            dt = time.perf_counter() - t0
            print(f"{name:>10}: {'steady' if res['steady'] else 'NOT steady'} after {res['steps_run']:>8} steps "
                  f"(the data set's maxIters: {iters}), {dt:7.3f} s, rel. change {res['last_rel']:.3e}, "
                  f"Reynolds {eng.reynolds():.6e}", flush=True)


if __name__ == "__main__":
    main()
