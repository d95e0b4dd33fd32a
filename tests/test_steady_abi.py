"""CPU checks of the steady-state entry points (lbm_run_until, lbm_batch_run_until): exported, declared, their result
struct laid out as the header says, and every argument check that needs no device made before any device call.
Host-only: passes on a box without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from cli_case import MALFORMED, run_cli
from conftest import ROOT


def test_steady_symbols_are_exported_and_declared(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in ("lbm_run_until", "lbm_batch_run_until"):
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)


def test_result_struct_matches_the_header(lbm):
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} lbm_steady_result;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"\b(int|double)\s+(\w+)\s*;", body)]
    ctype = {"int": ctypes.c_int, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(lbm._CSteadyResult._fields_)
    assert ctypes.sizeof(lbm._CSteadyResult) == 32
    # lbm_info / lbm_batch_info keep their layout
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4


def test_null_arguments_are_refused(lbm):
    lib = lbm.load_library()
    res = lbm._CSteadyResult()
    steps = ctypes.c_int()
    assert lib.lbm_run_until(None, 10, 1, 1e-3, 1, ctypes.byref(res)) != 0
    assert b"lbm_run_until" in lib.lbm_last_error()
    assert lib.lbm_batch_run_until(None, 10, 1, 1e-3, 1, ctypes.byref(res), ctypes.byref(steps)) != 0
    assert b"lbm_batch_run_until" in lib.lbm_last_error()


@pytest.mark.parametrize("kwargs,match", [
    ({"max_steps": -1}, "max_steps"), ({"max_steps": 1.5}, "max_steps must be an integer"),
    ({"max_steps": True}, "max_steps must be an integer"), ({"max_steps": 2 ** 31}, "max_steps"),
    ({"check_every": 0}, "check_every"), ({"check_every": "8"}, "check_every must be an integer"),
    ({"patience": 0}, "patience"), ({"patience": None}, "patience must be an integer"),
    ({"tol": -1e-9}, "tol must be a non-negative"), ({"tol": float("nan")}, "tol must be a non-negative"),
    ({"tol": "1e-3"}, "tol must be a number"), ({"tol": None}, "tol must be a number")])
def test_python_argument_checks_need_no_device(lbm, kwargs, match):
    args = {"max_steps": 100, "check_every": 10, "tol": 1e-6, "patience": 2}
    args.update(kwargs)
    with pytest.raises(lbm.LbmError, match=match):
        lbm._steady_args(**args)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._steady_args(np.int64(100), 10, 0, np.int32(3)) == (100, 10, 0.0, 3)
    assert lbm._steady_args(0, 1, np.float32(0.5), 1) == (0, 1, 0.5, 1)
    assert lbm._steady_args(5, 1, float("inf"), 1)[2] == float("inf")


def test_engine_classes_have_run_until(lbm):
    import inspect
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.run_until)
        assert list(sig.parameters)[1:] == ["max_steps", "check_every", "tol", "patience"]
        assert (sig.parameters["check_every"].default, sig.parameters["tol"].default,
                sig.parameters["patience"].default) == (1024, 1e-6, 2)
    member = lbm.BatchMember.__new__(lbm.BatchMember)
    with pytest.raises(lbm.LbmError, match="member of a batch"):
        member.run_until(10)


@pytest.mark.parametrize("value", [""] + MALFORMED["LBM_STEADY"])
def test_cli_dies_on_a_malformed_lbm_steady(lbm, tmp_path, value):
    """As for a malformed params file: a message and exit(EXIT_FAILURE), before any device is touched.  (An empty value
    counts as unset, so the run goes on to its usual end: on a box without a device that is lbm_create's error.)"""
    out = run_cli(lbm, tmp_path, LBM_STEADY=value)
    if value == "":
        assert "LBM_STEADY" not in out.stderr
        return
    assert out.returncode == 1
    assert "could not read LBM_STEADY" in out.stderr
    assert not (tmp_path / "av_vels.dat").exists()
