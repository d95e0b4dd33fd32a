"""CPU check of the segment loop of the checked runs (csrc/lbm_segments.h: issue up to `depth` segments ahead, judge the
oldest, end at the first stop, break or failed issue), as a stand-alone program: nothing is loaded into Python.
Host-only: passes on a box without a GPU."""
import os
import subprocess

from conftest import ROOT
import makefile_rules

CSRC = os.path.join(ROOT, "lbm-asynchronous_amd", "csrc")


def test_segment_loop(tmp_path):
    """lbm_segments.h, built as a stand-alone program under AddressSanitizer and UBSan (as ring_check is): against a
    brute-force list of the issues and judges, exhaustively for 0 .. 6 segments, depth 1 and 2, a stop, a break and a
    failing issue at each index or never -- issues in index order, never more than `depth` in flight, nothing after the
    first stop, break or failure, nothing left in flight at depth 1 and at most one segment at depth 2, nothing at all
    for no segment"""
    exe = str(tmp_path / "segments_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "segments_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"segments_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    # n_seg 0 .. 6, two depths; the stop, the break and the failing issue each at one of n_seg indices or never
    assert run.stdout == "%d cases, 0 failed\n" % sum(2 * (n + 1) ** 3 for n in range(7))


def test_the_engine_loops_over_segments_nowhere_else():
    """the header is the one place: the engine's source includes it, calls it, and keeps no look-ahead count of its own;
    the Makefile rebuilds the library when the header changes"""
    src = open(os.path.join(CSRC, "lbm_hip.hip")).read()
    assert '#include "lbm_segments.h"' in src and "lbm_segments::run(" in src
    assert "issued - judged" not in src
    makefile = open(os.path.join(ROOT, "lbm-asynchronous_amd", "Makefile")).read()
    for target in ("liblbm_hip.so:", "asm:", "profile-lib:"):
        line = makefile_rules.rule_line(target)
        assert "csrc/lbm_segments.h" in line, target
