"""tests/plan_dump.cpp as a stand-alone checked binary: what lbm_plan.h (plan_kernels, slab_rows) decides for one
context, asked from Python.  Host arithmetic only -- shared by the CPU test that pins the plans
(test_kernel_plan.py), the CPU test that ties every exact stream-kernel row to a GPU case (test_stream_rows.py) and the GPU test that compares them with what a created context reports (test_gpu_plan.py).
"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "plan_dump.cpp")

HALO = {"none": 0, "memcpy": 1, "rccl": 2, "host": 3}       # lbm_plan::HaloKind


def build(directory) -> str:
    """Compiles plan_dump with AddressSanitizer and UBSan into `directory`.  The runtimes are linked statically: the
    binary checks itself wherever it runs, and nothing has to be preloaded into it."""
    exe = os.path.join(str(directory), "plan_dump")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", SOURCE, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    return exe


def run(exe, *, nx, ny, world=1, rank=0, n_slabs=1, halo=0, cus, n_devices=1, distinct_devices=0, env=None) -> dict:
    """One plan, in a child process whose only LBM_* variables are `env`.  Returns {"plan": {...}, "slabs": [...],
    "stream_rows": [...], "resident_form": n}."""
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("LBM_")}
    child_env.update(env or {})
    args = [nx, ny, world, rank, n_slabs, halo, cus, n_devices, int(distinct_devices)]
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=child_env)
    assert out.returncode == 0, f"plan_dump {args} {env}: exit status {out.returncode}\n{out.stderr}"
    return json.loads(out.stdout)
