"""CPU checks of the residual-steady runs (lbm_run_until_residual and its batch twin): exported and declared, the result's
layout, the argument checks that need no device, the verdict function the check kernels call (csrc/lbm_residual_until.h,
as a stand-alone program), and the model the GPU tests compare against, run on the oracle alone for their cases.
Host-only: passes on a box without a GPU."""
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
import residual_until_model as rum
import steady_model as sm
from conftest import ROOT

NAMES = ("lbm_run_until_residual", "lbm_batch_run_until_residual")
RESULT_FIELDS = ("steps_run", "steady", "steady_step", "checks", "diverged", "reserved", "last_rel", "last")


def test_symbols_are_exported_declared_and_listed(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert re.fullmatch(r"lbm_[a-z_]+", name)
    assert re.search(r"int lbm_run_until_residual\(lbm_ctx\* ctx, int max_steps, int check_every, double tol, int patience,\s*"
                     r"lbm_residual_steady_result\* out,\s*lbm_residual_row\* history[^,]*, int history_capacity\);", header)
    assert re.search(r"int lbm_batch_run_until_residual\(lbm_batch\* batch, int max_steps, int check_every, double tol, int patience,\s*"
                     r"lbm_residual_steady_result\* out[^,]*, int\* steps_run,\s*lbm_residual_row\* history[^,]*, int history_capacity\);", header)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout
    assert ctypes.sizeof(lbm._CSteadyResult) == 32


def test_result_layout(lbm, tmp_path):
    """sizeof(lbm_residual_steady_result) == 72 and its field offsets, by the C compiler, against the binding's struct"""
    src = tmp_path / "layout.c"
    fields = ", ".join("offsetof(lbm_residual_steady_result, %s)" % f for f in RESULT_FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n'
                   "  size_t v[] = {sizeof(lbm_residual_steady_result), %s, sizeof(lbm_residual_row), sizeof(lbm_steady_result),\n"
                   "                sizeof(lbm_info), sizeof(lbm_batch_info)};\n"
                   '  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) printf("%%zu ", v[i]);\n  return 0;\n}\n'
                   % (os.path.join(ROOT, "include", "lbm_hip.h"), fields))
    exe = str(tmp_path / "layout")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", str(src), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [72, 0, 4, 8, 12, 16, 20, 24, 32, 40, 32, 80, 24]
    c = lbm._CResidualSteadyResult
    assert ctypes.sizeof(c) == 72 and tuple(n for n, _ in c._fields_) == RESULT_FIELDS
    assert [getattr(c, n).offset for n in RESULT_FIELDS] == got[1:9]
    row = lbm._CResidualRow
    assert ctypes.sizeof(row) == lbm.RESIDUAL_DTYPE.itemsize == 40
    assert [(n, getattr(row, n).offset) for n, _ in row._fields_] == [(n, lbm.RESIDUAL_DTYPE.fields[n][1]) for n in lbm.RESIDUAL_DTYPE.names]


def test_null_arguments_are_refused_by_name(lbm):
    lib = lbm.load_library()
    res = lbm._CResidualSteadyResult()
    steps = ctypes.c_int()
    assert lib.lbm_run_until_residual(None, 10, 4, 1e-4, 2, ctypes.byref(res), None, 0) != 0
    assert b"lbm_run_until_residual: NULL argument" in lib.lbm_last_error()
    assert lib.lbm_batch_run_until_residual(None, 10, 4, 1e-4, 2, res, ctypes.byref(steps), None, 0) != 0
    assert b"lbm_batch_run_until_residual: NULL argument" in lib.lbm_last_error()


@pytest.mark.parametrize("args,match", [
    ((1.5, 16, 1e-4, 2), "max_steps must be an integer"), ((100, True, 1e-4, 2), "check_every must be an integer"),
    ((100, 16, 1e-4, None), "patience must be an integer"), ((-1, 16, 1e-4, 2), r"max_steps must lie in \[0, 2\^31\)"),
    ((100, 0, 1e-4, 2), r"check_every must lie in \[1, 2\^31\)"), ((100, 16, 1e-4, 0), r"patience must lie in \[1, 2\^31\)"),
    ((100, 16, "1", 2), "tol must be a number"), ((100, 16, -1e-9, 2), "tol must be a non-negative number"),
    ((100, 16, float("nan"), 2), "tol must be a non-negative number")])
def test_python_argument_checks_are_run_untils(lbm, args, match):
    """without a device, through _steady_args, message for message"""
    with pytest.raises(lbm.LbmError, match="run_until: .*" + match) as steady:
        lbm._steady_args(*args)
    for cls in (lbm.Engine, lbm.Batch):
        with pytest.raises(lbm.LbmError) as got:
            cls.run_until_residual(None, *args)                      # refused before `self` is touched
        assert str(got.value) == str(steady.value)


@pytest.mark.parametrize("history,match", [(1.5, "history must be an integer or None"), (True, "history must be an integer or None"),
                                           ("3", "history must be an integer or None"), (-1, r"history must lie in \[0, 2\^31\)"),
                                           (2 ** 31, r"history must lie in \[0, 2\^31\)")])
def test_python_history_check(lbm, history, match):
    with pytest.raises(lbm.LbmError, match="run_until: " + match):
        lbm._until_history_arg(history, 4096, 512)
    for cls in (lbm.Engine, lbm.Batch):
        with pytest.raises(lbm.LbmError, match="run_until: " + match):
            cls.run_until_residual(None, 4096, 512, history=history)


def test_python_history_capacity(lbm):
    assert lbm._until_history_arg(None, 4096, 512) == 8 and lbm._until_history_arg(None, 1300, 512) == 2
    assert lbm._until_history_arg(None, 100, 512) == 0 and lbm._until_history_arg(0, 4096, 512) == 0
    assert lbm._until_history_arg(np.int64(3), 4096, 512) == 3 and type(lbm._until_history_arg(np.int64(3), 4096, 512)) is int
    assert lbm._until_history_arg(100, 4096, 512) == 8                 # never more rows than checks


def test_method_signatures(lbm):
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.run_until_residual)
        assert list(sig.parameters) == ["self", "max_steps", "check_every", "tol", "patience", "history"]
        assert [sig.parameters[k].default for k in ("check_every", "tol", "patience", "history")] == [1024, 1e-4, 2, None]
    assert lbm.BatchMember.run_until_residual is not lbm.Engine.run_until_residual
    with pytest.raises(lbm.LbmError, match="run_until_residual: this engine is a member of a batch"):
        lbm.BatchMember.run_until_residual(None, 100)


# ---- the model's own corners -------------------------------------------------------------------------------------------
def mrow(du, u, bad=0, span=8):
    return {"sum_du_sq": du, "sum_u_sq": u, "nonfinite": bad, "max_du": np.float32(0.0), "max_x": 0, "max_y": 0, "span": span}


def test_model_rel_and_its_corners(lbm):
    assert rum.rel(mrow(1.0, 4.0)) == 0.5 and rum.rel(mrow(0.0, 0.0)) == 0.0 and rum.rel(mrow(0.0, 3.0)) == 0.0
    assert math.isinf(rum.rel(mrow(2.5, 0.0)))
    assert rum.rel(mrow(3e-7, 0.7)) == math.sqrt(3e-7 / 0.7)
    rows = np.zeros(4, dtype=lbm.RESIDUAL_DTYPE)                          # ... which are residual_l2's
    rows["sum_du_sq"], rows["sum_u_sq"] = [1.0, 0.0, 2.5, 3e-7], [4.0, 0.0, 0.0, 0.7]
    assert lbm.residual_l2(rows).tolist() == [rum.rel(r) for r in rows]


def test_model_patience_streak_and_cap():
    E = 8
    rows = [mrow(r * r, 1.0) for r in (1.0, 0.5, 1e-3, 0.5, 1e-3, 1e-3, 1e-3)]
    r = rum.run_until(rows, 7 * E, E, 1e-2, 2)
    assert r["steady"] and r["steady_step"] == r["steps_run"] == r["end_step"] == 6 * E and r["checks"] == 6 and not r["diverged"]
    assert r["rels"][:3] == [1.0, 0.5, 1e-3] and r["last"] is rows[5]
    r = rum.run_until(rows, 7 * E, E, 1e-2, 1)                            # the first segment is already a check
    assert r["steady_step"] == 3 * E and r["checks"] == 3
    assert rum.run_until(rows, 7 * E, E, 1e30, 1)["steady_step"] == E
    r = rum.run_until(rows, 7 * E + 5, E, 1e-2, 4)                        # never four in a row; the rest is run unchecked
    assert not r["steady"] and r["steady_step"] == -1 and r["steps_run"] == 7 * E + 5 and r["checks"] == 7 and r["end_step"] == -1
    r = rum.run_until(rows, E - 1, E, 1e30, 1)
    assert r["steps_run"] == E - 1 and r["checks"] == 0 and math.isinf(r["last_rel"]) and r["last"] is None
    assert rum.run_until([mrow(0.0, 1.0)] * 2, 4 * E, E, 0.0, 2)["steady_step"] == 2 * E      # tol = 0: met by r = 0
    assert not rum.run_until(rows, 7 * E, E, 0.0, 1)["steady"]
    assert not rum.run_until([mrow(1.0, 0.0)] * 3, 3 * E, E, 1e300, 1)["steady"]               # r = +inf <= tol only for tol = +inf
    assert rum.run_until([mrow(1.0, 0.0)] * 3, 3 * E, E, math.inf, 1)["steady_step"] == E


def test_model_divergence_ends_the_call():
    E = 8
    rows = [mrow(1e-8, 1.0), mrow(1e-8, 1.0, bad=3), mrow(1e-8, 1.0)]
    r = rum.run_until(rows, 5 * E, E, 1e-2, 2)                            # the second check would have made it steady
    assert r["diverged"] and not r["steady"] and r["steady_step"] == -1 and r["steps_run"] == r["end_step"] == 2 * E and r["checks"] == 2
    assert r["last"] is rows[1] and r["last_rel"] == 1e-4


def test_model_batch_stops_with_its_last_member():
    E = 8
    a = [mrow(0.0, 1.0)] * 6
    b = [mrow(1.0, 1.0)] * 3 + [mrow(0.0, 1.0)] * 3
    c = [mrow(1.0, 1.0), mrow(1.0, 1.0, bad=1)] + [mrow(0.0, 1.0)] * 4
    steps, members = rum.batch_run_until([a, b, c], 6 * E, E, 1e-6, 2)
    assert steps == 5 * E and [m["end_step"] for m in members] == [2 * E, 5 * E, 2 * E]
    assert [m["steady"] for m in members] == [True, True, False] and [m["diverged"] for m in members] == [False, False, True]
    assert [m["checks"] for m in members] == [2, 5, 2] and all(m["steps_run"] == steps for m in members)
    steps, members = rum.batch_run_until([a, b], 4 * E, E, 1e-6, 2)
    assert steps == 4 * E and [m["steady"] for m in members] == [True, False]


# ---- the verdict function ----------------------------------------------------------------------------------------------
def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def verdict_runs():
    """[(tol, patience, E, [check: (dsq terms, usq terms, bad)])]"""
    rng = np.random.default_rng(11)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                                               # noqa: E731
    wide = lambda n: f32(np.abs(np.ldexp(rng.standard_normal(n), rng.integers(-140, 120, n))))    # noqa: E731
    small = lambda n, scale: f32(rng.random(n) * scale)                                           # noqa: E731
    # carries across limbs: many terms of 0x1.fffffep+31 and 0x1.fffffep+63, and of the smallest floats
    top = f32([np.ldexp(2.0 - 2.0 ** -23, 31)] * 40000 + [np.ldexp(2.0 - 2.0 ** -23, 63)] * 25536)
    tiny = f32([1e-45] * 70000 + [np.ldexp(1.0, -126)] * 3)
    falling = [(small(300, s * s), small(300, 1.0), 0) for s in (1.0, 1e-2, 1e-4, 1e-5, 1e-5, 1e-5, 1e-5)]
    runs = [(1e-3, 2, 512, falling),                                          # steady at check 4; the checks after it change nothing
            (1e-3, 1, 512, falling[:4]), (1e-3, 3, 64, falling),              # patience 1 and 3
            (1e-9, 2, 512, falling),                                          # never met
            (0.0, 2, 7, [(small(50, 1e-6), small(50, 1.0), 0), ([], small(50, 1.0), 0), ([], [], 0), ([], [], 0)]),   # tol = 0; 0 / 0
            (math.inf, 1, 1, [(small(9, 1.0), [], 0), ([], [], 0)]),         # tol = +inf meets r = +inf (x / 0)
            (1e300, 1, 3, [(small(9, 1.0), [], 0), (small(9, 1.0), small(9, 1.0), 0)]),   # ... a finite tol does not
            (1e-3, 2, 5, [falling[3], (falling[4][0], falling[4][1], 2), falling[5], falling[6]]),   # diverged at the check that would
            (1e30, 1, 1, [(small(20, 1.0), small(20, 1.0), 7), falling[0]]),  # have made it steady; diverged at once
            (0.5, 2, 1000, [(wide(400), wide(400), 0), (top, tiny, 0), (tiny, top, 0), (top[::-1], top, 0), (tiny, tiny[:5], 0)])]
    return runs


def verdict_text(tol, patience, E, checks):
    """the program's input for one run, the expected state after every check from math.fsum and the model"""
    lines = ["%x %d %d %d" % (dbits(tol), patience, E, len(checks))]
    rows, streak, stopped = [], 0, False
    for j, (dsq, usq, bad) in enumerate(checks, 1):
        sums = []
        for t in (dsq, usq):
            t = np.asarray(t, dtype=np.float32)
            lines.append(" ".join(["%d" % len(t)] + ["%x" % b for b in t.view(np.uint32).tolist()]))
            sums.append(math.fsum(float(v) for v in t))
        lines.append("%d %x" % (bad, (0x3f800000 << 32) | (0xffffffff - j)))
        rows.append(mrow(sums[0], sums[1], bad, E))
        want = rum.run_until(rows, j * E, E, tol, patience)                   # the model over the checks so far
        stop = 1 if want["steady"] else (2 if want["diverged"] else 0)
        code = 0 if stopped else stop
        if not stopped:
            streak = 0 if (bad > 0 or not rum.rel(rows[-1]) <= tol) else streak + 1
        stopped = stop != 0
        lines.append("%x %x %x %d %d %d %d %d" % (dbits(sums[0]), dbits(sums[1]), dbits(want["last_rel"]), code, streak, want["checks"], stop,
                                                   want["steady_step"]))
    return "\n".join(lines) + "\n"


def test_verdict_function_as_a_stand_alone_program(tmp_path):
    """lbm_residual_until.h under AddressSanitizer and UBSan, nothing preloaded (as residual_row_check is built): the
    device rounding against exact_sum_round and math.fsum, r_j and the state after every check against the model"""
    exe = str(tmp_path / "residual_until_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "residual_until_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    runs = verdict_runs()
    texts = [verdict_text(*r) for r in runs]
    last = lambda t: t.splitlines()[-1].split()[3:]                                              # noqa: E731
    assert last(texts[0]) == ["0", "2", "4", "1", "2048"]              # stopped at check 4, three more checks fed
    assert last(texts[1]) == ["0", "1", "3", "1", "1536"] and last(texts[2]) == ["0", "3", "5", "1", "320"]
    assert last(texts[3]) == ["0", "0", "7", "0", "-1"]
    assert last(texts[4]) == ["0", "2", "3", "1", "21"] and last(texts[5]) == ["0", "1", "1", "1", "1"]
    assert last(texts[6]) == ["1", "1", "2", "1", "6"]
    assert last(texts[7]) == ["0", "0", "2", "2", "-1"] and last(texts[8]) == ["0", "0", "1", "2", "-1"]
    run = subprocess.run([exe], input="".join(texts), capture_output=True, text=True)
    assert run.returncode == 0, f"residual_until_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert run.stdout == "%d runs, %d checks, 0 failed\n" % (len(runs), sum(len(r[3]) for r in runs))


# ---- the cases of the GPU tests, on the oracle alone ----------------------------------------------------------------
def margin(rels, tol):
    return sm.margin(rels, tol)


@pytest.mark.parametrize("shape", ["resident", "per_pass", rum.ODD])
def test_gpu_cases_stop_where_pinned(lbm, oracle, shape):
    p, ob = rum.case(lbm, shape)
    _, rows = rum.oracle_rows(oracle, p, ob, oracle.init_cells(p), 8, rum.STEADY["check_every"])
    r = rum.run_until(rows, **rum.STEADY)
    print(shape, r["rels"], [rum.rel(x) for x in rows])
    assert r["steady"] and r["steps_run"] == r["steady_step"] == rum.STEADY_STEPS and r["checks"] == 4 and not r["diverged"]
    assert margin(r["rels"], rum.STEADY["tol"]) >= rum.MARGIN, r["rels"]
    assert r["rels"][0] == 1.0                                            # from rest: the whole field is change
    floor = [rum.rel(x) for x in rows[2:]]
    assert all(5e-6 < v < 5e-5 for v in floor), floor                     # the fp32 floor the header states
    n = rum.run_until(rows, **rum.NOT_STEADY)
    assert not n["steady"] and not n["diverged"] and n["steps_run"] == 1300 and n["checks"] == 2
    assert not rum.run_until(rows, 4096, 512, 1e-9, 2)["steady"]


def test_gpu_batch_members_stop_where_pinned(lbm, oracle):
    member_rows = []
    for omega, accel in sm.BATCH:
        p, ob = rum.case(lbm, "resident", omega, accel)
        member_rows.append(rum.oracle_rows(oracle, p, ob, oracle.init_cells(p), 8, 512)[1])
    steps, members = rum.batch_run_until(member_rows, **rum.STEADY)
    print([m["steady_step"] for m in members], [m["rels"] for m in members])
    assert tuple(m["steady_step"] for m in members) == rum.BATCH_STEADY_STEPS and steps == 2560
    for m in members:
        assert m["steady"] and margin(m["rels"], rum.STEADY["tol"]) >= rum.BATCH_MARGIN, m["rels"]
    assert min(margin(m["rels"], rum.STEADY["tol"]) for m in members) == pytest.approx(2.466, abs=1e-3)
    steps, members = rum.batch_run_until(member_rows, 4096, 512, 1e-9, 2)
    assert steps == 4096 and not any(m["steady"] for m in members)


def test_divergence_case(lbm, oracle):
    from test_residual_abi import smallest
    p, ob, cells = smallest(lbm)
    _, rows = rum.oracle_rows(oracle, p, ob, residual_model.poisoned(cells), 3, 1)
    assert tuple(r["nonfinite"] for r in rows) == residual_model.POISON_COUNTS
    r = rum.run_until(rows, 3, 1, 1e-4, 2)
    assert r["diverged"] and not r["steady"] and r["steps_run"] == 1 and r["checks"] == 1 and r["last"]["nonfinite"] == residual_model.POISON_COUNTS[0]


def test_at_rest_is_steady_after_patience_checks(lbm, oracle):
    p = lbm.Params(16, 8, 400, 10, 0.1, 0.0, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[0, :3] = ob[3:5, 6:8] = 1
    _, rows = rum.oracle_rows(oracle, p, ob, oracle.init_cells(p), 4, 2)
    for patience in (1, 3):
        r = rum.run_until(rows, 8, 2, 0.0, patience)
        assert r["steady"] and r["steady_step"] == 2 * patience and r["last_rel"] == 0.0
