"""ms per timestep and MLUPS of the double engine (DoubleEngine, step_double) against the fp32 one-step kernel
(LBM_FUSE2=0 LBM_RESIDENT=0: step_vec4, the kernel step_double is the twin of), same process, same session.
python tools/double_bench.py [--log FILE]

128x128 and 1024x1024 (the reference's data sets) and 8192x8192 (the 1024x1024 map tiled, bench.py's workload:
`8192 8192 iters 10 0.1 0.01 1.85`).  Each figure is the median of 5 timed calls (HIP events around the call's launches,
run_timed) after one warm-up call.  The expectation at 8192x8192, where both kernels stream from HBM: step_double moves
144 bytes per lattice update against 72, so at least 0.45 x the fp32 kernel's MLUPS (0.5 less a 10 % margin for the
fp64 divides).  The lines are printed and written to FILE (default profiles/double_bench.log)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402

CASES = ((128, 128, 4000), (1024, 1024, 400), (8192, 8192, 40))   # nx, ny, timesteps per timed call
REPEATS = 5


def median_ms(eng, steps):
    eng.run_timed(steps)   # warm-up
    return statistics.median(eng.run_timed(steps) for _ in range(REPEATS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "double_bench.log"))
    args = ap.parse_args()
    os.environ["LBM_FUSE2"] = "0"      # the fp32 yardstick: one timestep per pass ...
    os.environ["LBM_RESIDENT"] = "0"   # ... also where long calls would run the resident kernel
    lbm = conftest.load_package()
    inputs = os.path.join(ROOT, "tests", "golden", "inputs")
    tile = lbm.read_obstacles(os.path.join(inputs, "obstacles_1024x1024.dat"), 1024, 1024)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/double_bench.py: median of {REPEATS} run_timed calls after one warm-up; fp32 = step_vec4 (LBM_FUSE2=0 LBM_RESIDENT=0)")
    for nx, ny, steps in CASES:
        own = os.path.join(inputs, f"input_{nx}x{ny}.params")
        if os.path.exists(own):
            p64 = lbm.read_params_double(own)
            ob = lbm.read_obstacles(os.path.join(inputs, f"obstacles_{nx}x{ny}.dat"), nx, ny)
        else:
            p64 = lbm.ParamsDouble(nx, ny, 0, 10, 0.1, 0.01, 1.85)
            ob = lbm.tile_obstacles(tile, nx, ny)
        p64.max_iters = (REPEATS + 1) * steps
        p32 = lbm.Params(nx, ny, p64.max_iters, p64.reynolds_dim, p64.density, p64.accel, p64.omega)
        with lbm.Engine(p32, ob, None, n_gpus=1, math="exact") as eng:
            info = eng.info()
            assert info["steps_per_launch"] == 1 and info["resident_steps"] == 0, info
            ms32 = median_ms(eng, steps)
            nts32 = info["nontemporal"]
        with lbm.DoubleEngine(p64, ob) as eng:
            info = eng.info()
            ms64 = median_ms(eng, steps)
        cells = nx * ny
        mlups32, mlups64 = cells / ms32 / 1e3, cells / ms64 / 1e3
        say(f"{nx}x{ny}: {steps} steps per call | fp32 step_vec4 {ms32:9.5f} ms/step {mlups32:9.1f} MLUPS (nts {nts32}) | "
            f"double step_double {ms64:9.5f} ms/step {mlups64:9.1f} MLUPS (lane_cells {info['lane_cells']}, nts {info['nontemporal']}) | "
            f"double / fp32 MLUPS {mlups64 / mlups32:5.3f} | double {144.0 * cells / ms64 / 1e9:6.2f} TB/s, fp32 {72.0 * cells / ms32 / 1e9:6.2f} TB/s of compulsory traffic")
        if (nx, ny) == (8192, 8192):
            ratio = mlups64 / mlups32
            say(f"8192x8192 expectation double >= 0.45 x fp32: {'MET' if ratio >= 0.45 else 'MISSED'} ({ratio:5.3f})")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
