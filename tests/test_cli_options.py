"""The option parser of the command line (lbm-asynchronous_amd/host/lbm_options.c), checked without a GPU.

tests/options_check.c calls lbm_parse_options over its NAME=VALUE arguments and prints the parsed options on one line.  It is
built from lbm_options.c and lbm_io.c alone as a stand-alone program under AddressSanitizer and UBSan, as test_own_handle
builds own_check: the runtimes are linked statically, nothing is preloaded and nothing of it is loaded into Python.  Every
malformed value of the corpus (tests/cli_case.py) must end it with status 1 and its "could not read" message, every valid
one must print the expected line, and a sanitizer report fails either (it ends the program with another status and text).

The 21 pairs of the option table then go through d2q9-bgk itself: each is refused with its one message and nothing is
written -- on a box without a device too, which is what "before any device is touched" means."""
import os
import re
import subprocess

import pytest

from cli_case import VALID, malformed_cases, pair_cases, printed, run_cli
from conftest import ROOT

HOST = os.path.join(ROOT, "lbm-asynchronous_amd", "host")


@pytest.fixture(scope="module")
def options_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("options_check") / "options_check")
    cmd = ["gcc", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "options_check.c"), os.path.join(HOST, "lbm_options.c"), os.path.join(HOST, "lbm_io.c"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    return exe


def check(exe, env):
    return subprocess.run([exe] + ["%s=%s" % kv for kv in env.items()], capture_output=True, text=True)


def test_malformed_values_are_refused(options_check):
    cases = malformed_cases()
    assert len(cases) >= 50
    for env, name in cases:
        out = check(options_check, env)
        assert out.returncode == 1, (env, out.stderr)
        assert re.fullmatch(r"Error at line \d+ of file .*lbm_options\.c:\ncould not read %s: expected .*\n" % name, out.stderr), (env, out.stderr)
        assert out.stdout == ""


def test_valid_values_parse_to_the_expected_options(options_check):
    for env, expect in VALID:
        out = check(options_check, env)
        assert (out.returncode, out.stderr) == (0, ""), (env, out.stderr)
        assert out.stdout == printed(expect) + "\n", env


def test_mean_order_needs_mean(options_check):
    out = check(options_check, {"LBM_MEAN_ORDER": "2", "LBM_STATES": "10", "LBM_FORCES": "5"})
    assert out.returncode == 1 and out.stderr.endswith(":\nLBM_MEAN_ORDER needs LBM_MEAN\n")


@pytest.mark.parametrize("env,message", pair_cases(), ids=lambda v: "+".join(v) if isinstance(v, dict) else None)
def test_cli_refuses_each_pair_before_any_device_is_touched(lbm, tmp_path, env, message):
    out = run_cli(lbm, tmp_path, **env)
    assert out.returncode == 1
    assert re.fullmatch(r"Error at line \d+ of file .*:\n%s\n" % re.escape(message), out.stderr), out.stderr
    assert "no HIP device" not in out.stderr
    assert sorted(os.listdir(tmp_path)) == ["input.params", "obstacles.dat"]
    for name in ("av_vels.dat", "animation_data", "state_data", "probes.dat", "forces.dat"):
        assert not (tmp_path / name).exists()
