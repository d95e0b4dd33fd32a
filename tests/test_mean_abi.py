"""CPU checks of the mean-field entry points (lbm_set_mean, lbm_read_mean): exported, declared, the argument checks that
need no device made before any device call, the mean_state.dat writer, the command line's LBM_MEAN parser and its
forbidden combinations, and the CPU model the GPU tests compare against.  Host-only: passes on a box without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import mean_model
from cli_case import MALFORMED, run_cli
from conftest import ROOT


def test_mean_symbols_are_exported_and_declared(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in ("lbm_set_mean", "lbm_read_mean"):
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
    assert re.search(r"lbm_read_mean\(lbm_ctx\* ctx, double\* sum_u_x, double\* sum_u_y, double\* sum_u_mag, "
                     r"double\* sum_pressure,\s*long long\* n_samples\)", header)
    # lbm_info / lbm_batch_info keep their layout: what a host needs it gets from lbm_read_mean
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4


def test_null_context_is_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_longlong(-1)
    assert lib.lbm_set_mean(None, 10) != 0
    assert b"lbm_set_mean" in lib.lbm_last_error()
    assert lib.lbm_read_mean(None, None, None, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_mean" in lib.lbm_last_error()


@pytest.mark.parametrize("every,match", [
    (1.5, "every must be an integer"), (True, "every must be an integer"), ("1", "every must be an integer"),
    (None, "every must be an integer"), (-1, r"every must lie in \[0, 2\^31\)"), (2 ** 31, r"every must lie in \[0, 2\^31\)")])
def test_python_argument_checks_need_no_device(lbm, every, match):
    with pytest.raises(lbm.LbmError, match=match):
        lbm._mean_args(every)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._mean_args(0) == 0 and lbm._mean_args(1) == 1 and lbm._mean_args(2 ** 31 - 1) == 2 ** 31 - 1
    out = lbm._mean_args(np.int64(7))
    assert out == 7 and type(out) is int


def test_engine_signatures(lbm):
    assert list(inspect.signature(lbm.Engine.set_mean).parameters) == ["self", "every"]
    assert list(inspect.signature(lbm.Engine.mean_sums).parameters) == ["self"]
    assert list(inspect.signature(lbm.Engine.mean).parameters) == ["self"]
    for name in ("set_mean", "mean_sums", "mean"):
        assert getattr(lbm.BatchMember, name) is getattr(lbm.Engine, name)
    assert list(inspect.signature(lbm.write_mean_state).parameters) == ["path", "mean", "obstacles"]


def test_write_mean_state_matches_the_format(lbm, tmp_path):
    """final_state.dat's line format from float64 means rounded to float (1/3 and 0.1/3 are not floats: the file shows
    the rounded values)."""
    mean = {"u_x": np.array([[1.5e-3, 0.0], [0.123456789, 1.0]]), "u_y": np.array([[-2.5e-4, -0.0], [1.0, 2.0]]),
            "u": np.array([[1e-40, 0.0], [1.0, 3.0]]), "pressure": np.array([[1.0 / 3.0, 0.1 / 3.0], [2.0, 4.0]]),
            "samples": 3}
    ob = np.array([[0, 1], [0, 0]], dtype=np.int32)
    path = tmp_path / "mean_state.dat"
    lbm.write_mean_state(str(path), mean, ob)
    want = ("0 0 1.500000013039E-03 -2.500000118744E-04 9.999946101115E-41 3.333333432674E-01 0\n"
            "1 0 0.000000000000E+00 -0.000000000000E+00 0.000000000000E+00 3.333333507180E-02 1\n"
            "0 1 1.234567910433E-01 1.000000000000E+00 1.000000000000E+00 2.000000000000E+00 0\n"
            "1 1 1.000000000000E+00 2.000000000000E+00 3.000000000000E+00 4.000000000000E+00 0\n")
    assert path.read_text() == want


@pytest.mark.parametrize("value", [""] + MALFORMED["LBM_MEAN"])
def test_cli_dies_on_a_malformed_lbm_mean(lbm, tmp_path, value):
    """As for a malformed LBM_PROBES: a message and exit(EXIT_FAILURE), before any device is touched.  (An empty value
    counts as unset, so the run goes on to its usual end: on a box without a device that is lbm_create's error.)"""
    out = run_cli(lbm, tmp_path, LBM_MEAN=value)
    if value == "":
        assert "LBM_MEAN" not in out.stderr
        return
    assert out.returncode == 1
    assert "could not read LBM_MEAN" in out.stderr
    assert not (tmp_path / "av_vels.dat").exists()
    assert not (tmp_path / "mean_state.dat").exists()


@pytest.mark.parametrize("other,value", [("LBM_ANIMATION", "100"), ("LBM_PROBES", "1,2"), ("LBM_STEADY", "1e-6")])
def test_cli_dies_on_forbidden_combinations(lbm, tmp_path, other, value):
    out = run_cli(lbm, tmp_path, LBM_MEAN="10:2", **{other: value})
    assert out.returncode == 1
    assert "%s and LBM_MEAN cannot be combined" % other in out.stderr
    assert not (tmp_path / "av_vels.dat").exists()
    assert not (tmp_path / "mean_state.dat").exists()


def test_mean_model_against_brute_force(lbm, oracle):
    """oracle_sums steps from sample to sample; the brute force takes every step on its own and adds where
    tt % every == 0.  A 16 x 8 lattice with an obstacle, armed at step 5."""
    p = lbm.Params(16, 8, 40, 8, 0.1, 0.005, 1.7)
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[3, 4:7] = 1
    start = oracle.init_cells(p)
    oracle.run(p, start, ob, 5)
    for every, total in ((1, 23), (4, 23), (7, 36), (50, 36)):
        ref, sums, n = mean_model.oracle_sums(oracle, p, ob, start, 5, total, every)
        cells = start.copy()
        brute = {k: np.zeros((8, 16), dtype=np.float64) for k in mean_model.FIELDS}
        count = 0
        for tt in range(5, total):
            oracle.run(p, cells, ob, 1)
            if tt % every == 0:
                state = oracle.final_state(p, cells, ob)
                for k in mean_model.FIELDS:
                    brute[k] += state[k].astype(np.float64)
                count += 1
        assert n == count == len([tt for tt in range(5, total) if tt % every == 0])
        assert np.array_equal(ref.view(np.uint32), cells.view(np.uint32))
        for k in mean_model.FIELDS:
            assert np.array_equal(sums[k].view(np.uint64), brute[k].view(np.uint64)), (every, k)
        if n:
            assert brute["pressure"][3, 5] == n * np.float64(np.float32(p.density) * np.float32(1.0 / 3.0))
            assert brute["u"][3, 5] == 0.0 and mean_model.means_of(sums, n)["samples"] == n
