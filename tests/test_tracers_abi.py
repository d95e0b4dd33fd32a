"""CPU checks of the tracer particles (lbm_set_tracers, lbm_read_tracers, lbm_tracers_now and the batch twins): exported
and declared, lbm_tracer's layout, what the header states, the Python-side refusals of shape and dtype, tracer_seeds
against a hand-written case and the text writer's round trip.  Host-only: passes on a box without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("lbm_set_tracers", "lbm_read_tracers", "lbm_tracers_now", "lbm_batch_set_tracers", "lbm_batch_read_tracers", "lbm_batch_tracers_now")


def test_tracer_symbols_are_exported_declared_and_listed(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
    assert re.search(r"int lbm_set_tracers\(lbm_ctx\* ctx, int n, const lbm_tracer\* start[^,]*, int every, int capacity\);", header)
    assert re.search(r"int lbm_read_tracers\(lbm_ctx\* ctx, int max_rows, lbm_tracer\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_tracers_now\(lbm_ctx\* ctx, lbm_tracer\* out[^,)]*\);", header)
    assert re.search(r"int lbm_batch_set_tracers\(lbm_batch\* batch, int n, const lbm_tracer\* start[^,]*, int every, int capacity\);", header)
    assert re.search(r"int lbm_batch_read_tracers\(lbm_batch\* batch, int max_rows, lbm_tracer\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_batch_tracers_now\(lbm_batch\* batch, lbm_tracer\* out[^,)]*\);", header)
    assert re.search(r"#define LBM_MAX_TRACERS \(1 << 24\)", header) and lbm.MAX_TRACERS == 1 << 24


def test_tracer_layout(tmp_path):
    """sizeof(lbm_tracer) == 16 with x at 0 and y at 8, by the C compiler"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu %%zu %%zu %%d\\n", sizeof(lbm_tracer), offsetof(lbm_tracer, x), offsetof(lbm_tracer, y), LBM_MAX_TRACERS);\n'
                   "  return 0;\n}\n" % os.path.join(ROOT, "include", "lbm_hip.h"))
    exe = str(tmp_path / "layout")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", str(src), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert subprocess.run([exe], capture_output=True, text=True).stdout.split() == ["16", "0", "8", str(1 << 24)]


def test_the_header_states_the_definition_and_what_is_not_offered():
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    text = header[header.index("---- tracer particles"):header.index("} lbm_tracer;")]
    flat = " ".join(text.replace("*", " ").split())
    for line in ("the centre of cell (i, j) lies at (i, j)", "i0 = floor(x), fx = x - i0, i1 = i0 + 1, or 0 when that equals nx",
                 "a = u[j0][i0] + fx (u[j0][i1] - u[j0][i0])", "b = u[j1][i0] + fx (u[j1][i1] - u[j1][i0])", "v = a + fy (b - a)",
                 "W(z, n) = z - n floor(z / n)", "becomes 0.0", "xm = W(x + (0.5 H) v1x, nx)", "x' = W(x + H v2x, nx)",
                 "(NaN, NaN) and stays so", "since the previous sample, or since arming for the first sample",
                 "capacity == 0 arms WITHOUT a ring", "a tracer's four cells can straddle two slabs"):
        assert line in flat, line
    for word in ("several slabs", "rank contexts", "the double engine", "finite-size or inertial particles", "unwrapped coordinates",
                 "seeding during a run"):
        assert word in flat[flat.index("Not offered"):], word


def test_null_handles_are_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    xy = np.zeros((4, 2))
    for call, args in ((lib.lbm_set_tracers, (None, 4, xy.ctypes.data, 10, 4)), (lib.lbm_read_tracers, (None, 0, None, None, ctypes.byref(n))),
                       (lib.lbm_tracers_now, (None, xy.ctypes.data)), (lib.lbm_batch_set_tracers, (None, 4, xy.ctypes.data, 10, 4)),
                       (lib.lbm_batch_read_tracers, (None, 0, None, None, ctypes.byref(n))), (lib.lbm_batch_tracers_now, (None, xy.ctypes.data))):
        assert call(*args) != 0
        assert call.__name__.encode() in lib.lbm_last_error()
    assert lib.lbm_set_tracers(None, 4, xy.ctypes.data, -1, 4) != 0    # (a null context before everything else)
    assert lib.lbm_last_error() == b"lbm_set_tracers: null context"


def test_method_signatures(lbm):
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.set_tracers)
        assert list(sig.parameters) == ["self", "xy", "every", "capacity"] and sig.parameters["capacity"].default == 0
        assert list(inspect.signature(cls.tracer_rows).parameters) == ["self", "max_rows"]
        assert inspect.signature(cls.tracer_rows).parameters["max_rows"].default is None
        assert list(inspect.signature(cls.tracers).parameters) == ["self"]
    assert lbm.BatchMember.set_tracers is lbm.Engine.set_tracers      # a member raises the engine's refusal
    assert list(inspect.signature(lbm.write_tracers).parameters) == ["path", "steps", "rows"]
    assert list(inspect.signature(lbm.tracer_seeds).parameters) == ["obstacles", "spacing"]


def test_shape_and_dtype_refusals(lbm):
    ok = np.zeros((5, 2))
    xy, every, capacity = lbm._tracer_args("set_tracers", ok, (), 4, 0)            # no ring: allowed
    assert xy.dtype == np.float64 and xy.flags.c_contiguous and (every, capacity) == (4, 0)
    xy, _, _ = lbm._tracer_args("set_tracers", np.arange(12, dtype=np.float32).reshape(6, 2)[::2], (), np.int64(1), np.int32(7))
    assert xy.dtype == np.float64 and xy.flags.c_contiguous and xy.tolist() == [[0.0, 1.0], [4.0, 5.0], [8.0, 9.0]]
    assert lbm._tracer_args("set_tracers", [[1, 2]], (), 1, 1)[0].tolist() == [[1.0, 2.0]]
    assert lbm._tracer_args("set_tracers", np.zeros((0, 2)), (), 1, 1)[0].shape == (0, 2)
    assert lbm._tracer_args("set_tracers", np.zeros((3, 5, 2)), (3,), 1, 1)[0].shape == (3, 5, 2)
    for bad in (np.zeros(5), np.zeros((5, 3)), np.zeros((2, 5, 2)), np.zeros((5, 2, 1)), 1.0):
        with pytest.raises(lbm.LbmError, match=r"set_tracers: xy must have shape \(n, 2\)"):
            lbm._tracer_args("set_tracers", bad, (), 1, 1)
    for bad in (np.zeros((5, 2)), np.zeros((2, 5, 2)), np.zeros((3, 5, 3))):
        with pytest.raises(lbm.LbmError, match=r"set_tracers: xy must have shape \(3, n, 2\)"):
            lbm._tracer_args("set_tracers", bad, (3,), 1, 1)
    for bad in (np.zeros((5, 2), dtype=complex), np.zeros((5, 2), dtype=bool), np.array([["a", "b"]]), np.array([[None, 1.0]], dtype=object)):
        with pytest.raises(lbm.LbmError, match="set_tracers: xy must hold real numbers"):
            lbm._tracer_args("set_tracers", bad, (), 1, 1)
    for every, capacity, word in ((-1, 4, "every"), (1.5, 4, "every"), (True, 4, "every"), (1, -1, "capacity"), (1, 2 ** 31, "capacity"),
                                  (1, "4", "capacity")):
        with pytest.raises(lbm.LbmError, match="set_tracers: %s must" % word):
            lbm._tracer_args("set_tracers", ok, (), every, capacity)


def test_tracer_seeds_by_hand(lbm):
    ob = np.zeros((5, 7), dtype=np.int32)
    ob[0, 2] = ob[2, 0] = ob[4, 6] = ob[1, 1] = 1                     # (1, 1) is on no sub-grid of spacing 2
    seeds = lbm.tracer_seeds(ob, 2)
    assert seeds.dtype == np.float64
    assert seeds.tolist() == [[0, 0], [4, 0], [6, 0], [2, 2], [4, 2], [6, 2], [0, 4], [2, 4], [4, 4]]    # (x, y), row-major
    assert lbm.tracer_seeds(ob, 1).shape == (31, 2) and lbm.tracer_seeds(ob, 7).tolist() == [[0, 0]]
    assert lbm.tracer_seeds(np.ones((3, 3)), 1).shape == (0, 2)
    for bad in (0, -1, 1.0, True):
        with pytest.raises(lbm.LbmError, match="tracer_seeds: spacing"):
            lbm.tracer_seeds(ob, bad)
    with pytest.raises(lbm.LbmError, match="tracer_seeds: obstacles"):
        lbm.tracer_seeds(np.zeros(5), 1)


def test_write_tracers_round_trip(lbm, tmp_path):
    path = str(tmp_path / "tracers.dat")
    rng = np.random.default_rng(3)
    rows = rng.random((3, 4, 2)) * 100
    rows[1, 2] = np.nan                                               # a lost tracer
    rows[2, 0] = (0.0, np.nextafter(13.0, 0))
    lbm.write_tracers(path, [0, 4, 8], rows)
    lines = open(path).read().splitlines()
    assert len(lines) == 3 and [line.split(":")[0] for line in lines] == ["0", "4", "8"]
    assert lines[0].startswith("0:\t%.17E\t%.17E\t" % (rows[0, 0, 0], rows[0, 0, 1]))
    back = np.array([[float(v) for v in line.split("\t")[1:]] for line in lines]).reshape(3, 4, 2)
    nan = np.isnan(rows)
    assert np.array_equal(nan, np.isnan(back)) and np.array_equal(back.view(np.uint64)[~nan], rows.view(np.uint64)[~nan])
    for steps, bad in (([0, 4], rows), ([0, 4, 8], rows.astype(np.float32)), ([0, 4, 8], rows[:, :, 0]), ([0, 4, 8], np.zeros((3, 4, 3)))):
        with pytest.raises(lbm.LbmError, match="write_tracers: rows must be"):
            lbm.write_tracers(path, steps, bad)
