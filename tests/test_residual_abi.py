"""CPU checks of the velocity residuals (lbm_set_residual, lbm_read_residual and their batch twins): exported and
declared, the row's layout, the argument checks that need no device, residual_l2 and the writer, "words -> row"
(csrc/lbm_residual_row.h, as a stand-alone program), and the numpy model the GPU tests compare against, checked on the
oracle alone.  Host-only: passes on a box without a GPU."""
import ctypes
import inspect
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import residual_model
from conftest import ROOT
from test_gpu_forces import small

NAMES = ("lbm_set_residual", "lbm_read_residual", "lbm_batch_set_residual", "lbm_batch_read_residual")
ROW_FIELDS = ("sum_du_sq", "sum_u_sq", "nonfinite", "max_du", "max_x", "max_y", "span")


def test_residual_symbols_are_exported_declared_and_listed(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert re.fullmatch(r"lbm_[a-z_]+", name)
    assert re.search(r"int lbm_set_residual\(lbm_ctx\* ctx, int every, int capacity\);", header)
    assert re.search(r"int lbm_read_residual\(lbm_ctx\* ctx, int max_rows, lbm_residual_row\* out, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_batch_set_residual\(lbm_batch\* batch, int every, int capacity\);", header)
    assert re.search(r"int lbm_batch_read_residual\(lbm_batch\* batch, int max_rows, lbm_residual_row\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout


def test_row_layout(lbm, tmp_path):
    """sizeof(lbm_residual_row) == 40 and its field offsets, by the C compiler, against RESIDUAL_DTYPE"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(lbm_residual_row), offsetof(lbm_residual_row, sum_du_sq),\n'
                   "         offsetof(lbm_residual_row, sum_u_sq), offsetof(lbm_residual_row, nonfinite), offsetof(lbm_residual_row, max_du),\n"
                   "         offsetof(lbm_residual_row, max_x), offsetof(lbm_residual_row, max_y), offsetof(lbm_residual_row, span),\n"
                   "         sizeof(lbm_info), sizeof(lbm_batch_info));\n  return 0;\n}\n"
                   % os.path.join(ROOT, "include", "lbm_hip.h"))
    exe = str(tmp_path / "layout")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", str(src), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [40, 0, 8, 16, 24, 28, 32, 36, 80, 24]
    d = lbm.RESIDUAL_DTYPE
    assert d.itemsize == 40 and d.names == ROW_FIELDS
    assert [d.fields[k][1] for k in ROW_FIELDS] == got[1:8]
    assert [d.fields[k][0] for k in ROW_FIELDS] == [np.dtype(t) for t in ("<f8", "<f8", "<i8", "<f4", "<i4", "<i4", "<i4")]


def test_null_handles_are_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    assert lib.lbm_set_residual(None, 10, 4) != 0
    assert b"lbm_set_residual" in lib.lbm_last_error()
    assert lib.lbm_read_residual(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_residual" in lib.lbm_last_error()
    assert lib.lbm_batch_set_residual(None, 10, 4) != 0
    assert b"lbm_batch_set_residual" in lib.lbm_last_error()
    assert lib.lbm_batch_read_residual(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_batch_read_residual" in lib.lbm_last_error()


@pytest.mark.parametrize("every,capacity,match", [
    (1.5, 4, "every must be an integer"), (True, 4, "every must be an integer"), ("1", 4, "every must be an integer"),
    (None, 4, "every must be an integer"), (10, 2.0, "capacity must be an integer"), (10, None, "capacity must be an integer"),
    (-1, 4, r"every must lie in \[0, 2\^31\)"), (2 ** 31, 4, r"every must lie in \[0, 2\^31\)"),
    (10, -3, r"capacity must lie in \[0, 2\^31\)"), (10, 2 ** 31, r"capacity must lie in \[0, 2\^31\)"), (10, 0, "at least one row")])
def test_python_argument_checks_need_no_device(lbm, every, capacity, match):
    with pytest.raises(lbm.LbmError, match="set_residual: .*" + match):
        lbm._residual_args(every, capacity)
    # ... and they are _stats_args' checks, message for message
    with pytest.raises(lbm.LbmError) as stats:
        lbm._stats_args(every, capacity)
    with pytest.raises(lbm.LbmError) as residual:
        lbm._residual_args(every, capacity)
    assert str(residual.value) == str(stats.value).replace("set_stats:", "set_residual:")


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._residual_args(0, 0) == (0, 0)
    assert lbm._residual_args(3, 2 ** 31 - 1) == (3, 2 ** 31 - 1)
    every, capacity = lbm._residual_args(np.int64(7), np.int32(2))
    assert (every, capacity) == (7, 2) and type(every) is int and type(capacity) is int


def test_method_signatures(lbm):
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.set_residual)
        assert list(sig.parameters) == ["self", "every", "capacity"] and sig.parameters["capacity"].default == 4096
        assert list(inspect.signature(cls.residuals).parameters) == ["self", "max_rows"]
        assert inspect.signature(cls.residuals).parameters["max_rows"].default is None
    assert lbm.BatchMember.set_residual is lbm.Engine.set_residual      # a member raises the engine's refusal
    assert list(inspect.signature(lbm.write_residuals).parameters) == ["path", "steps", "rows"]
    assert list(inspect.signature(lbm.residual_l2).parameters) == ["rows"]


def test_residual_l2_and_its_three_corners(lbm):
    rows = np.zeros(4, dtype=lbm.RESIDUAL_DTYPE)
    rows["sum_du_sq"] = [1.0, 0.0, 2.5, 0.0]
    rows["sum_u_sq"] = [4.0, 0.0, 0.0, 3.0]
    got = lbm.residual_l2(rows)
    assert got.dtype == np.float64 and got.tolist() == [0.5, 0.0, math.inf, 0.0]
    assert lbm.residual_l2(rows.reshape(2, 2)).shape == (2, 2)                   # a batch's [n, members]
    one = np.zeros(1, dtype=lbm.RESIDUAL_DTYPE)
    one["sum_du_sq"], one["sum_u_sq"] = 3e-7, 0.7
    assert lbm.residual_l2(one)[0] == math.sqrt(3e-7 / 0.7)


def test_write_residuals_format(lbm, tmp_path):
    path = str(tmp_path / "residuals.dat")
    rows = np.zeros(3, dtype=lbm.RESIDUAL_DTYPE)
    rows[0] = (0.25, 4.0, 0, 0.5, 3, 7, 1)
    rows[1] = (0.0, 0.0, 12, 0.0, -1, -1, 50)
    rows[2] = (1.0, 0.0, 0, 1.0, 0, 0, 50)
    lbm.write_residuals(path, [0, 50, 100], rows)
    assert open(path).read() == ("0:\t2.500000000000E-01\t2.500000000000E-01\t4.000000000000E+00\t5.000000000000E-01\t3\t7\t1\t0\n"
                                 "50:\t0.000000000000E+00\t0.000000000000E+00\t0.000000000000E+00\t0.000000000000E+00\t-1\t-1\t50\t12\n"
                                 "100:\tINF\t1.000000000000E+00\t0.000000000000E+00\t1.000000000000E+00\t0\t0\t50\t0\n")
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_residuals(path, [0], rows)
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_residuals(path, [0, 50, 100], np.zeros((3, 7)))


# ---- words -> row -------------------------------------------------------------------------------------------------------
def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def fbits(v):
    return int(np.float32(v).view(np.uint32))


def row_cases():
    """[(nx, span, [slab: ([dsq terms], [usq terms], bad, [(dmag, cell)])])]; what the row must be follows from all terms"""
    rng = np.random.default_rng(7)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                                               # noqa: E731
    wide = lambda n: f32(np.abs(np.ldexp(rng.standard_normal(n), rng.integers(-140, 120, n))))    # noqa: E731
    cases = []
    cases.append((16, 1, [(f32(rng.random(120) * 1e-6), f32(rng.random(120) * 1e-3), 0,
                           [(np.float32(0.001 * (i % 7)), i) for i in range(120)])]))              # one slab
    three = [(wide(290), f32(rng.random(290)), s, [(np.float32(0.02 + 0.001 * ((i * 7 + s) % 11)), s * 300 + i) for i in range(290)])
             for s in range(3)]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0)):                                    # slabs merged in any order
        cases.append((128, 4, [three[s] for s in order]))
    # carries across limbs: 2^16 terms of 0x1.fffffep+31 and of 0x1.fffffep+63 overflow limb boundaries many times over
    top = f32([np.ldexp(2.0 - 2.0 ** -23, 31)] * 40000 + [np.ldexp(2.0 - 2.0 ** -23, 63)] * 25536)
    tiny = f32([1e-45] * 70000 + [np.ldexp(1.0, -126)] * 3)
    cases.append((64, 7, [(top, tiny, 0, [(np.float32(1.0), 1)]), (top[::-1], tiny[:5], 0, [(np.float32(1.0), 0)])]))
    cases.append((64, 2, [([], [], 0, []), ([], [], 0, [])]))                                      # key 0: 0 at -1, -1
    cases.append((64, 2147483647, [([], [], 40, []), ([], [], 24, [])]))                           # nothing finite; the largest span
    tie = np.float32(0.0625)
    cases.append((64, 3, [([], [], 0, [(tie, 700), (np.float32(0.06), 3)]), ([], [], 0, [(tie, 130), (tie, 131)]),
                          ([], [], 0, [(tie, 4000)])]))                                            # a tie between slabs: cell 130
    cases.append((64, 1, [([], [], 0, [(np.float32(0.0), 0), (np.float32(0.0), 1)]), ([], [], 0, [(np.float32(0.0), 64)])]))  # cell 0, dmag = +0
    cases.append((65536, 9, [([], [], 0, [(np.float32(3e38), 2 ** 31 - 2)]), ([], [], 0, [(np.float32(1e-45), 2 ** 31 - 1)])]))
    return cases


def row_text(nx, span, slabs):
    lines = ["%d %d %d" % (len(slabs), nx, span)]
    total = [[], []]
    bad, best = 0, None
    for dsq, usq, n_bad, cells in slabs:
        for j, t in enumerate((dsq, usq)):
            t = np.asarray(t, dtype=np.float32)
            lines.append(" ".join(["%d" % len(t)] + ["%x" % b for b in t.view(np.uint32).tolist()]))
            total[j] += [float(v) for v in t]
        lines.append("%d %d" % (n_bad, len(cells)) + "".join(" %x %d" % (fbits(u), c) for u, c in cells))
        bad += n_bad
        for u, c in cells:
            if best is None or (float(u), -c) > (float(best[0]), -best[1]):
                best = (u, c)
    u, x, y = (np.float32(0.0), -1, -1) if best is None else (best[0], best[1] % nx, best[1] // nx)
    lines.append(" ".join("%x" % dbits(math.fsum(t)) for t in total) + " %d %x %d %d %d" % (bad, fbits(u), x, y, span))
    return "\n".join(lines) + "\n"


def test_words_to_row(tmp_path):
    """lbm_residual_row.h, built as a stand-alone program under AddressSanitizer and UBSan (as stats_row_check is): slabs
    merged in any order, key 0, ties between slabs, carries across limbs, the span passed through"""
    exe = str(tmp_path / "residual_row_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "residual_row_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    cases = row_cases()
    texts = [row_text(nx, span, slabs) for nx, span, slabs in cases]
    assert len({t.splitlines()[-1] for t in texts[1:5]}) == 1                                     # every order: one expected row
    assert "\n0 0 0 0 -1 -1 2\n" in texts[6] and texts[8].endswith(" 0 %x 2 2 3\n" % fbits(0.0625))  # key 0; the tie goes to cell 130
    run = subprocess.run([exe], input="".join(texts), capture_output=True, text=True)
    assert run.returncode == 0, f"residual_row_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert run.stdout == "%d cases, 0 failed\n" % len(cases)


# ---- the model, on the oracle alone ---------------------------------------------------------------------------------
def smallest(lbm):
    p, ob, cells = small(lbm, 16, 8)
    ob[3:5, 6:8] = 1
    return p, ob, cells


def test_model_field_is_the_oracles_final_state(lbm, oracle):
    p, ob, cells = smallest(lbm)
    oracle.run(p, cells, ob, 20)
    ux, uy = residual_model.field(cells, ob)
    want = oracle.final_state(p, cells, ob)
    for got, key in ((ux, "u_x"), (uy, "u_y")):
        assert np.array_equal(got.view(np.uint32), np.asarray(want[key], dtype=np.float32).view(np.uint32)), key
    assert np.all(ux[ob != 0] == 0.0) and np.all(uy[ob != 0] == 0.0)


def test_model_smallest_case_twelve_distinct_rows(lbm, oracle):
    p, ob, cells = smallest(lbm)
    _, rows = residual_model.oracle_rows(oracle, p, ob, cells, 0, 12, 1)
    assert sorted(rows) == list(range(12)) and all(r["span"] == 1 and r["nonfinite"] == 0 for r in rows.values())
    du = [rows[tt]["sum_du_sq"] for tt in range(12)]
    assert len(set(du)) == 12
    assert 3.2e-2 < du[0] < 3.4e-2 and 7.5e-3 < du[11] < 8.5e-3                # the random start relaxes
    assert all(0.0 < rows[tt]["max_du"] and 0 <= rows[tt]["max_x"] < 16 and 0 <= rows[tt]["max_y"] < 8 for tt in rows)


def test_model_armed_after_unarmed_steps(lbm, oracle):
    p, ob, cells = smallest(lbm)
    oracle.run(p, cells, ob, 6)
    _, rows = residual_model.oracle_rows(oracle, p, ob, cells, 6, 12, 4)
    assert [(tt, rows[tt]["span"]) for tt in sorted(rows)] == [(8, 3), (12, 4), (16, 4)]


def test_model_at_rest(lbm, oracle):
    """accel = 0 from the uniform equilibrium, with blocked cells: nothing ever moves"""
    p = lbm.Params(16, 8, 400, 10, 0.1, 0.0, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[0, :3] = ob[3:5, 6:8] = 1
    _, rows = residual_model.oracle_rows(oracle, p, ob, oracle.init_cells(p), 0, 4, 2)
    for r in rows.values():
        assert r["sum_du_sq"] == 0.0 and r["sum_u_sq"] == 0.0 and not np.signbit(r["sum_du_sq"]) and not np.signbit(r["sum_u_sq"])
        assert (float(r["max_du"]), r["max_x"], r["max_y"]) == (0.0, 3, 0)       # the first FLUID cell


def test_model_channel_ties_take_the_smallest_cell(lbm, oracle):
    p = lbm.Params(64, 16, 400, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((16, 64), dtype=np.int32)
    ob[0, :] = 1
    _, rows = residual_model.oracle_rows(oracle, p, ob, oracle.init_cells(p), 0, 12, 4)
    assert sorted(rows) == [0, 4, 8] and all(r["max_x"] == 0 and r["max_du"] > 0 for r in rows.values())


def test_model_counts_nonfinite_cells(lbm, oracle):
    p, ob, cells = smallest(lbm)
    _, rows = residual_model.oracle_rows(oracle, p, ob, residual_model.poisoned(cells), 0, 3, 1)
    assert tuple(rows[tt]["nonfinite"] for tt in range(3)) == residual_model.POISON_COUNTS == (4, 18, 48)
    assert all(math.isfinite(rows[tt]["sum_du_sq"]) and rows[tt]["sum_du_sq"] > 0.0 for tt in range(3))   # the sums are taken over the rest
