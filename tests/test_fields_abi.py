"""CPU checks of the field-frame entry points (lbm_set_field_frames, lbm_read_field_frames): exported, declared, the
argument checks that need no device made before any device call, the state-frame writer, the command line's LBM_STATES
parser and its forbidden combinations, and the CPU model the GPU tests compare against.  Host-only: passes on a box
without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fields_model
from cli_case import MALFORMED, run_cli
from conftest import ROOT


def test_field_frame_symbols_are_exported_and_declared(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in ("lbm_set_field_frames", "lbm_read_field_frames"):
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
    assert re.search(r"int lbm_set_field_frames\(lbm_ctx\* ctx, int every, int capacity, int fields, const lbm_window\* window\b", header)
    assert re.search(r"int lbm_read_field_frames\(lbm_ctx\* ctx, int max_frames, float\* out, int\* steps, int\* n_read\);", header)
    assert re.search(r"typedef struct \{ int x0, y0, nx, ny; \} lbm_window;", header)
    for name, value in (("UX", 1), ("UY", 2), ("UMAG", 4), ("PRESSURE", 8), ("ALL", 15)):
        assert re.search(r"#define LBM_FIELD_%s\s+%d\b" % (name, value), header)
    assert lbm.FIELD_BITS == {"u_x": 1, "u_y": 2, "u": 4, "pressure": 8}
    # lbm_info / lbm_batch_info keep their layout
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4
    assert ctypes.sizeof(lbm._CWindow) == 16


def test_null_context_is_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    assert lib.lbm_set_field_frames(None, 10, 4, 15, None) != 0
    assert b"lbm_set_field_frames" in lib.lbm_last_error()
    assert lib.lbm_read_field_frames(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_field_frames" in lib.lbm_last_error()


ALL = ("u_x", "u_y", "u", "pressure")


@pytest.mark.parametrize("every,capacity,fields,window,match", [
    (1.5, 4, ALL, None, "every must be an integer"), (True, 4, ALL, None, "every must be an integer"),
    ("1", 4, ALL, None, "every must be an integer"), (None, 4, ALL, None, "every must be an integer"),
    (10, 2.0, ALL, None, "capacity must be an integer"), (10, None, ALL, None, "capacity must be an integer"),
    (-1, 4, ALL, None, r"every must lie in \[0, 2\^31\)"), (2 ** 31, 4, ALL, None, r"every must lie in \[0, 2\^31\)"),
    (10, -3, ALL, None, r"capacity must lie in \[0, 2\^31\)"), (10, 2 ** 31, ALL, None, r"capacity must lie in \[0, 2\^31\)"),
    (10, 0, ALL, None, "at least one frame slot"),
    (10, 4, (), None, "no fields"), (10, 4, [], None, "no fields"), (10, 4, 15, None, "sequence of names"),
    (10, 4, ("u_x", "speed"), None, "unknown field 'speed'"), (10, 4, ("u_mag",), None, "unknown field"),
    (10, 4, (1,), None, "unknown field"), (10, 4, ("u_x", "u", "u_x"), None, "named twice"),
    (10, 4, ALL, (1, 2, 3), "four integers"), (10, 4, ALL, (1, 2, 3, 4, 5), "four integers"), (10, 4, ALL, 7, "four integers"),
    (10, 4, ALL, (1, 2, 3.0, 4), "four integers"), (10, 4, ALL, (1, 2, True, 4), "four integers"),
    (10, 4, ALL, (-1, 2, 3, 4), r"lie in \[0, 2\^31\)"), (10, 4, ALL, (1, 2, 3, 2 ** 31), r"lie in \[0, 2\^31\)"),
    (10, 4, ALL, (1, 2, 0, 4), "at least 1 x 1"), (10, 4, ALL, (1, 2, 3, 0), "at least 1 x 1")])
def test_python_argument_checks_need_no_device(lbm, every, capacity, fields, window, match):
    with pytest.raises(lbm.LbmError, match=match):
        lbm._field_frame_args(every, capacity, fields, window)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._field_frame_args(0, 0, ALL, None) == (0, 0, 15, None)
    assert lbm._field_frame_args(3, 2 ** 31 - 1, ["pressure", "u_x"], [0, 0, 1, 1]) == (3, 2 ** 31 - 1, 9, (0, 0, 1, 1))
    assert lbm._field_frame_args(3, 5, "u", None) == (3, 5, 4, None)
    out = lbm._field_frame_args(np.int64(7), np.int32(2), ("u_y",), np.array([1, 2, 3, 4]))
    assert out == (7, 2, 2, (1, 2, 3, 4))
    assert type(out[0]) is int and type(out[1]) is int and all(type(v) is int for v in out[3])


def test_engine_signatures(lbm):
    sig = inspect.signature(lbm.Engine.set_field_frames)
    assert list(sig.parameters) == ["self", "every", "capacity", "fields", "window"]
    assert sig.parameters["fields"].default == ALL and sig.parameters["window"].default is None
    assert sig.parameters["capacity"].default == inspect.signature(lbm.Engine.set_frames).parameters["capacity"].default
    sig = inspect.signature(lbm.Engine.field_frames)
    assert list(sig.parameters) == ["self", "max_frames"] and sig.parameters["max_frames"].default is None
    for name in ("set_field_frames", "field_frames"):
        assert getattr(lbm.BatchMember, name) is getattr(lbm.Engine, name)
    assert list(inspect.signature(lbm.write_state_frame).parameters) == ["path", "fields", "obstacles", "window"]
    assert list(inspect.signature(lbm._field_frame_args).parameters) == ["every", "capacity", "fields", "window"]


def test_write_state_frame_matches_the_format(lbm, tmp_path):
    """final_state.dat's line format for a 2 x 2 window at (1, 1) of a 3 x 3 grid: global ii jj, jj outer."""
    f32 = np.float32
    fields = {"u_x": np.array([[1.5e-3, 0.0], [0.123456789, 1.0]], dtype=f32), "u_y": np.array([[-2.5e-4, -0.0], [1.0, 2.0]], dtype=f32),
              "u": np.array([[1e-40, 0.0], [1.0, 3.0]], dtype=f32), "pressure": np.array([[1.0 / 3.0, 0.1 / 3.0], [2.0, 4.0]], dtype=f32)}
    ob = np.array([[1, 1, 1], [1, 0, 1], [1, 0, 0]], dtype=np.int32)
    path = tmp_path / "final_state_000100.dat"
    lbm.write_state_frame(str(path), fields, ob, (1, 1, 2, 2))
    want = ("1 1 1.500000013039E-03 -2.500000118744E-04 9.999946101115E-41 3.333333432674E-01 0\n"
            "2 1 0.000000000000E+00 -0.000000000000E+00 0.000000000000E+00 3.333333507180E-02 1\n"
            "1 2 1.234567910433E-01 1.000000000000E+00 1.000000000000E+00 2.000000000000E+00 0\n"
            "2 2 1.000000000000E+00 2.000000000000E+00 3.000000000000E+00 4.000000000000E+00 0\n")
    assert path.read_text() == want
    with pytest.raises(lbm.LbmError, match="leaves"):
        lbm.write_state_frame(str(path), fields, ob, (2, 1, 2, 2))
    with pytest.raises(lbm.LbmError, match="every field must be"):
        lbm.write_state_frame(str(path), fields, ob, (0, 0, 3, 2))


def test_write_state_frame_of_the_whole_grid_is_write_final_state(lbm, tmp_path):
    rng = np.random.default_rng(5)
    ny, nx = 5, 7
    fields = {k: rng.standard_normal((ny, nx)).astype(np.float32) for k in ALL}
    ob = (rng.random((ny, nx)) < 0.3).astype(np.int32)
    lbm.write_final_state(str(tmp_path / "a.dat"), fields, ob)
    lbm.write_state_frame(str(tmp_path / "b.dat"), fields, ob, (0, 0, nx, ny))
    assert (tmp_path / "a.dat").read_bytes() == (tmp_path / "b.dat").read_bytes()


@pytest.mark.parametrize("value", [""] + MALFORMED["LBM_STATES"])
def test_cli_dies_on_a_malformed_lbm_states(lbm, tmp_path, value):
    """As for a malformed LBM_MEAN: a message and exit(EXIT_FAILURE), before any device is touched.  (An empty value
    counts as unset, so the run goes on to its usual end: on a box without a device that is lbm_create's error.)"""
    out = run_cli(lbm, tmp_path, LBM_STATES=value)
    if value == "":
        assert "LBM_STATES" not in out.stderr
        return
    assert out.returncode == 1
    assert "could not read LBM_STATES" in out.stderr
    assert not (tmp_path / "av_vels.dat").exists()
    assert not (tmp_path / "state_data").exists()


@pytest.mark.parametrize("states", ["10", "10:1,2,3,4"])
@pytest.mark.parametrize("other,value,named", [("LBM_ANIMATION", "100", "LBM_ANIMATION"), ("LBM_PROBES", "1,2", "LBM_PROBES"),
                                               ("LBM_MEAN", "10:2", "LBM_MEAN"), ("LBM_STEADY", "1e-6", "LBM_STEADY"),
                                               ("LBM_PRECISION", "double", "LBM_PRECISION=double")])
def test_cli_dies_on_forbidden_combinations(lbm, tmp_path, states, other, value, named):
    out = run_cli(lbm, tmp_path, LBM_STATES=states, **{other: value})
    assert out.returncode == 1
    assert "%s and LBM_STATES cannot be combined" % named in out.stderr
    assert not (tmp_path / "av_vels.dat").exists()
    assert not (tmp_path / "state_data").exists()


def test_fields_model_against_brute_force(lbm, oracle):
    """oracle_field_frames steps from sample to sample; the brute force takes every step on its own and cuts the window
    out where tt % every == 0.  A 16 x 8 lattice with an obstacle, armed at step 5."""
    p = lbm.Params(16, 8, 40, 8, 0.1, 0.005, 1.7)
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[3, 4:7] = 1
    start = oracle.init_cells(p)
    oracle.run(p, start, ob, 5)
    for every, total, fields, window in ((1, 23, ALL, None), (4, 23, ("u_x", "pressure"), (3, 2, 5, 3)),
                                         (7, 36, ("u",), (15, 0, 1, 8)), (50, 36, ALL, (0, 7, 16, 1))):
        ref, frames = fields_model.oracle_field_frames(oracle, p, ob, start, 5, total, every, fields, window)
        x0, y0, wnx, wny = window or (0, 0, 16, 8)
        cells = start.copy()
        brute = {}
        for tt in range(5, total):
            oracle.run(p, cells, ob, 1)
            if tt % every == 0:
                state = oracle.final_state(p, cells, ob)
                brute[tt] = {k: state[k][y0:y0 + wny, x0:x0 + wnx] for k in fields}
        assert sorted(frames) == sorted(brute) == [tt for tt in range(5, total) if tt % every == 0]
        assert np.array_equal(ref.view(np.uint32), cells.view(np.uint32))
        for tt in brute:
            assert list(frames[tt]) == [k for k in ALL if k in fields]
            for k in fields:
                assert frames[tt][k].shape == (wny, wnx)
                assert np.array_equal(frames[tt][k].view(np.uint32), brute[tt][k].view(np.uint32)), (every, tt, k)
        if window == (3, 2, 5, 3) and frames:
            tt = sorted(frames)[0]
            assert frames[tt]["pressure"][1, 2] == np.float32(p.density) * np.float32(1.0 / 3.0)   # the blocked cell (5, 3)
            assert frames[tt]["u_x"][1, 2] == 0.0
