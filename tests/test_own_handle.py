"""The owning handle every device resource of the engine sits in (lbm-asynchronous_amd/csrc/lbm_own.h), checked without
a GPU: tests/own_check.cpp instantiates it with a counting release function and exits non-zero unless an empty handle
releases nothing, a full one releases exactly once (scope end, reset, move, move assignment, not on self-move, not after
release()), and a struct's members are released in reverse declaration order behind its destructor's body -- the order
Slab's teardown relies on.  Built as a stand-alone program under AddressSanitizer and UBSan, as plan_tool builds
plan_dump: the runtimes are linked statically, nothing is preloaded and nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "own_check.cpp")


def test_own_handle_releases_once_and_in_order(tmp_path):
    exe = str(tmp_path / "own_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", SOURCE, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"own_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
