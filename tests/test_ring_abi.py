"""CPU check of the recorders' ring arithmetic (csrc/lbm_ring.h: where the n oldest waiting records lie), as a stand-alone
program: nothing is loaded into Python.  Host-only: passes on a box without a GPU."""
import os
import subprocess

from conftest import ROOT
import makefile_rules

CSRC = os.path.join(ROOT, "lbm-asynchronous_amd", "csrc")


def test_oldest_runs(tmp_path):
    """lbm_ring.h, built as a stand-alone program under AddressSanitizer and UBSan (as stats_row_check is): against the
    brute-force list of (read + i) % slots, exhaustively for 1 .. 5 slots, every read % slots and n from 0 to slots, with
    `read` beyond 2^31 too -- the runs cover exactly the n oldest slots in order, never more than two, the second from slot
    0, none for n = 0 -- and the copy of records of 0 .. 3 words along them"""
    exe = str(tmp_path / "ring_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "ring_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"ring_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    # slots 1 .. 5: sum of slots * (slots + 1) pairs (read % slots, n), four record sizes, four reads; and the one by hand
    assert run.stdout == "%d cases, 0 failed\n" % (sum(s * (s + 1) for s in range(1, 6)) * 4 * 4 + 1)


def test_the_engine_splits_a_ring_nowhere_else():
    """the header is the one place: the engine's source has no ring split of its own, includes the header, and the
    Makefile rebuilds the library when the header changes"""
    src = open(os.path.join(CSRC, "lbm_hip.hip")).read()
    assert '#include "lbm_ring.h"' in src and "lbm_ring::oldest_runs" in src
    assert "slots - slot" not in src
    makefile = open(os.path.join(ROOT, "lbm-asynchronous_amd", "Makefile")).read()
    for target in ("liblbm_hip.so:", "asm:", "profile-lib:"):
        line = makefile_rules.rule_line(target)
        assert "csrc/lbm_ring.h" in line, target
