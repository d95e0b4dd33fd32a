"""CPU checks of the line profiles (lbm_set_profiles, lbm_read_profiles and their batch twins): exported and declared, the
line's layout, the argument checks that need no device, the text writer, the means, "words -> lines"
(csrc/lbm_profile_row.h, as a stand-alone program), and the numpy model the GPU tests compare against, checked on the
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

import profile_model
from conftest import ROOT

NAMES = ("lbm_set_profiles", "lbm_read_profiles", "lbm_batch_set_profiles", "lbm_batch_read_profiles")
FIELDS = ("sum_rho", "sum_jx", "sum_jy", "sum_ux", "sum_uy", "fluid", "nonfinite")


def test_profile_symbols_are_exported_declared_and_listed(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS and name not in lbm.ABI_SYMBOLS_NUMBERED
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert re.fullmatch(r"lbm_[a-z_]+", name)
    assert re.search(r"int lbm_set_profiles\(lbm_ctx\* ctx, int every, int capacity, int axes\);", header)
    assert re.search(r"int lbm_read_profiles\(lbm_ctx\* ctx, int max_records, lbm_profile_line\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_batch_set_profiles\(lbm_batch\* batch, int every, int capacity, int axes\);", header)
    assert re.search(r"int lbm_batch_read_profiles\(lbm_batch\* batch, int max_records, lbm_profile_line\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert re.search(r"#define LBM_PROFILE_ROWS\s+1\b", header) and re.search(r"#define LBM_PROFILE_COLUMNS\s+2\b", header)
    assert (lbm.PROFILE_ROWS, lbm.PROFILE_COLUMNS) == (1, 2)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout


def test_line_layout(lbm, tmp_path):
    """sizeof(lbm_profile_line) == 48 and its field offsets, by the C compiler, against PROFILE_DTYPE"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(lbm_profile_line), offsetof(lbm_profile_line, sum_rho),\n'
                   "         offsetof(lbm_profile_line, sum_jx), offsetof(lbm_profile_line, sum_jy), offsetof(lbm_profile_line, sum_ux),\n"
                   "         offsetof(lbm_profile_line, sum_uy), offsetof(lbm_profile_line, fluid), offsetof(lbm_profile_line, nonfinite));\n"
                   "  return 0;\n}\n" % os.path.join(ROOT, "include", "lbm_hip.h"))
    exe = str(tmp_path / "layout")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", str(src), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [48, 0, 8, 16, 24, 32, 40, 44]
    d = lbm.PROFILE_DTYPE
    assert d.itemsize == 48 and d.names == FIELDS
    assert [d.fields[k][1] for k in FIELDS] == got[1:]
    assert [d.fields[k][0] for k in FIELDS] == [np.dtype("<f8")] * 5 + [np.dtype("<i4")] * 2


def test_null_handles_are_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    assert lib.lbm_set_profiles(None, 10, 4, 3) != 0
    assert b"lbm_set_profiles" in lib.lbm_last_error()
    assert lib.lbm_read_profiles(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_profiles" in lib.lbm_last_error()
    assert lib.lbm_batch_set_profiles(None, 10, 4, 3) != 0
    assert b"lbm_batch_set_profiles" in lib.lbm_last_error()
    assert lib.lbm_batch_read_profiles(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_batch_read_profiles" in lib.lbm_last_error()


@pytest.mark.parametrize("every,capacity,axes,match", [
    (1.5, 4, 3, "every must be an integer"), (True, 4, 3, "every must be an integer"), ("1", 4, 3, "every must be an integer"),
    (None, 4, 3, "every must be an integer"), (10, 2.0, 3, "capacity must be an integer"), (10, None, 3, "capacity must be an integer"),
    (10, False, 3, "capacity must be an integer"),
    (-1, 4, 3, r"every must lie in \[0, 2\^31\)"), (2 ** 31, 4, 3, r"every must lie in \[0, 2\^31\)"),
    (10, -3, 3, r"capacity must lie in \[0, 2\^31\)"), (10, 2 ** 31, 3, r"capacity must lie in \[0, 2\^31\)"),
    (10, 0, 3, "at least one record"),
    (10, 4, 0, "select nothing"), (10, 4, 4, "select nothing"), (10, 4, -1, "select nothing"), (10, 4, (), "select nothing"),
    (10, 4, [], "select nothing"), (10, 4, ("rows", "diagonals"), "unknown axis 'diagonals'"), (10, 4, ("x",), "unknown axis 'x'"),
    (10, 4, (1,), "unknown axis 1"), (10, 4, True, "axes must be"), (10, 4, 1.0, "axes must be"), (10, 4, None, "axes must be"),
    (10, 4, "rows", "axes must be")])
def test_python_argument_checks_need_no_device(lbm, every, capacity, axes, match):
    with pytest.raises(lbm.LbmError, match="set_profiles: .*" + match):
        lbm._profile_args(every, capacity, axes)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._profile_args(0, 0, 3) == (0, 0, 3)
    assert lbm._profile_args(3, 2 ** 31 - 1, 1) == (3, 2 ** 31 - 1, 1)
    assert lbm._profile_args(3, 1, ("rows",)) == (3, 1, 1)
    assert lbm._profile_args(3, 1, ["columns"]) == (3, 1, 2)
    assert lbm._profile_args(3, 1, ("columns", "rows")) == (3, 1, 3)
    assert lbm._profile_args(3, 1, {"rows", "columns"}) == (3, 1, 3)
    every, capacity, axes = lbm._profile_args(np.int64(7), np.int32(2), np.int16(2))
    assert (every, capacity, axes) == (7, 2, 2) and type(every) is int and type(capacity) is int and type(axes) is int


def test_method_signatures(lbm):
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.set_profiles)
        assert list(sig.parameters) == ["self", "every", "capacity", "axes"]
        assert sig.parameters["capacity"].default == 16 and sig.parameters["axes"].default == ("rows", "columns")
        assert list(inspect.signature(cls.profiles).parameters) == ["self", "max_records"]
        assert inspect.signature(cls.profiles).parameters["max_records"].default is None
    assert lbm.BatchMember.set_profiles is lbm.Engine.set_profiles      # a member raises the engine's refusal
    assert list(inspect.signature(lbm.write_profile).parameters) == ["path", "lines"]
    assert list(inspect.signature(lbm.profile_means).parameters) == ["lines"]


def test_write_profile_format(lbm, tmp_path):
    path = str(tmp_path / "profile.dat")
    lines = np.zeros(2, dtype=lbm.PROFILE_DTYPE)
    lines[0] = (1638.25, 1.5, -2.0, 0.125, 0.5, 126, 2)
    lines[1] = (0.0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    lbm.write_profile(path, lines)
    assert open(path).read() == ("0\t1.638250000000E+03\t1.500000000000E+00\t-2.000000000000E+00\t1.250000000000E-01\t5.000000000000E-01\t126\t2\n"
                                 "1\t0.000000000000E+00\t0.000000000000E+00\t0.000000000000E+00\t0.000000000000E+00\t0.000000000000E+00\t0\t0\n")
    with pytest.raises(lbm.LbmError, match="lines must be"):
        lbm.write_profile(path, np.zeros((2, 2), dtype=lbm.PROFILE_DTYPE))
    with pytest.raises(lbm.LbmError, match="lines must be"):
        lbm.write_profile(path, np.zeros((2, 7)))


def test_profile_means(lbm):
    lines = np.zeros((2, 3), dtype=lbm.PROFILE_DTYPE)
    lines[0, 0] = (12.0, 3.0, -1.0, 0.75, -0.25, 4, 1)
    lines[1, 2] = (0.3, 0.03, 0.0, 0.1, 0.0, 3, 0)
    m = lbm.profile_means(lines)
    assert sorted(m) == ["j_x", "pressure", "rho", "u_x", "u_y"] and all(v.shape == (2, 3) and v.dtype == np.float64 for v in m.values())
    assert (m["rho"][0, 0], m["j_x"][0, 0], m["u_x"][0, 0], m["u_y"][0, 0]) == (3.0, 0.75, 0.1875, -0.0625)
    assert m["pressure"][0, 0] == 3.0 * (1.0 / 3.0) and m["u_x"][1, 2] == 0.1 / 3.0
    empty = np.ones((2, 3), dtype=bool)
    empty[0, 0] = empty[1, 2] = False
    for v in m.values():
        assert np.all(np.isnan(v[empty])) and not np.any(np.isnan(v[~empty]))


# ---- words -> lines -------------------------------------------------------------------------------------------------------
def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def line_cases():
    """[(nx, ny, axes, [(row_first, row_count)], {(slab, kind, index): ([5 term vectors], fluid, nonfinite)})]: random
    terms for every line of every slab's share; what a record must be follows from all terms"""
    rng = np.random.default_rng(8)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    pops = lambda n: f32(0.1 * (1 + 0.05 * rng.standard_normal(n)))
    wide = lambda n: f32(np.ldexp(rng.standard_normal(n), rng.integers(-140, 120, n)))
    carry = lambda n: f32(np.full(n, np.float32(4.0) - np.float32(2.0 ** -22)))   # 24 one-bits across the limbs 3 and 4: their sum carries
    empty = f32([])

    def line(n, kind):
        if kind == "zero":
            return [empty] * 5, 0, int(n)
        if kind == "carry":
            return [carry(300), -carry(300), carry(7), -carry(1), carry(2)], int(n), 0
        return [pops(n), f32(1e-3 * rng.standard_normal(n)), wide(n), -np.abs(wide(n)), f32(rng.standard_normal(n))], int(n), int(rng.integers(0, 3))

    cases = []
    for nx, ny, axes, ranges in ((5, 4, 3, [(0, 4)]), (3, 5, 3, [(0, 3), (3, 2)]), (4, 16, 3, [(0, 6), (6, 5), (11, 5)]),
                                 (6, 7, 1, [(0, 4), (4, 3)]), (6, 7, 2, [(0, 2), (2, 2), (4, 3)])):
        share = {}
        for s, (first, count) in enumerate(ranges):
            if axes & 1:
                for r in range(count):
                    kind = "zero" if first + r == 1 else "carry" if first + r == ny - 1 else "any"
                    share[(s, "rows", first + r)] = line(nx, kind)
            if axes & 2:
                for x in range(nx):
                    kind = "zero" if x == 1 else "carry" if x == 2 else "any"
                    share[(s, "columns", x)] = line(count, kind)
        cases.append((nx, ny, axes, ranges, share))
    return cases


def case_text(nx, ny, axes, ranges, share):
    out = ["%d %d %d %d" % (len(ranges), nx, ny, axes)]
    for s, (first, count) in enumerate(ranges):
        out.append("%d %d" % (first, count))
        keys = [(s, "rows", first + r) for r in range(count)] * (axes & 1) + [(s, "columns", x) for x in range(nx)] * ((axes >> 1) & 1)
        for key in keys:
            terms, fluid, bad = share[key]
            for t in terms:
                out.append(" ".join(["%d" % len(t)] + ["%x" % b for b in np.asarray(t, dtype=np.float32).view(np.uint32).tolist()]))
            out.append("%d %d" % (fluid, bad))
    return "\n".join(out) + "\n"


def case_expected(i, nx, ny, axes, ranges, share):
    out = ["case %d" % i]
    for kind, n in (("rows", ny if axes & 1 else 0), ("columns", nx if axes & 2 else 0)):
        for index in range(n):
            parts = [v for (s, k, j), v in sorted(share.items()) if k == kind and j == index]
            assert len(parts) == (1 if kind == "rows" else len(ranges))
            sums = [math.fsum(float(v) for p in parts for v in p[0][j]) for j in range(5)]
            out.append(" ".join("%016x" % dbits(v) for v in sums) + " %d %d" % (sum(p[1] for p in parts), sum(p[2] for p in parts)))
    return "\n".join(out) + "\n"


def test_words_to_lines(tmp_path):
    """lbm_profile_row.h, built as a stand-alone program under AddressSanitizer and UBSan (as stats_row_check is): 1, 2
    and 3 slabs with uneven row ranges, each axis alone and both, negative sums, a carry across limbs, an all-zero line"""
    exe = str(tmp_path / "profile_row_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "profile_row_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    cases = line_cases()
    text = "".join(case_text(*c) for c in cases)
    want = "".join(case_expected(i, *c) for i, c in enumerate(cases))
    zero = " ".join(["%016x" % 0] * 5)
    assert zero + " 0 5\n" in want and zero + " 0 16\n" in want                  # the all-zero lines: +0.0 five times
    assert any(line.split()[1][0] in "89abcdef" for line in want.splitlines() if " " in line)       # a negative sum
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, f"profile_row_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert run.stdout == want


# ---- the model, on the oracle alone ---------------------------------------------------------------------------------
def test_model_open_channel_columns_are_identical_and_counts_agree(lbm, oracle):
    """from the uniform equilibrium an open channel stays x-invariant: every column line has the same bits"""
    p = lbm.Params(64, 16, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((16, 64), dtype=np.int32)
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 12)
    rec = profile_model.record(cells, ob)
    assert len(rec["rows"]) == 16 and len(rec["columns"]) == 64
    first = rec["columns"][0]
    assert first["sum_jx"] > 0.0 and first["fluid"] == 16 and first["nonfinite"] == 0
    for col in rec["columns"]:
        assert not profile_model.same_bits([col], [first])
    assert rec["rows"][14]["sum_ux"] > rec["rows"][6]["sum_ux"]            # the driven row leads
    assert sum(r["fluid"] for r in rec["rows"]) == sum(c["fluid"] for c in rec["columns"]) == 16 * 64


def test_model_counts_blocked_and_nonfinite_cells(lbm, oracle):
    p = lbm.Params(16, 8, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[3:5, 6:8] = 1
    ob[6, :] = 1                                 # a fully blocked row
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 5)
    cells[0, 0, 1] = np.inf                      # fluid
    cells[3, 6, 4] = np.nan                      # blocked: counted nowhere
    cells[1, 1, :] = 0.0                         # rho = 0: u is 0 / 0
    rec = profile_model.record(cells, ob)
    fluid_cells = int((ob == 0).sum())
    assert sum(r["fluid"] + r["nonfinite"] for r in rec["rows"]) == sum(c["fluid"] + c["nonfinite"] for c in rec["columns"]) == fluid_cells
    assert [r["nonfinite"] for r in rec["rows"]] == [1, 1, 0, 0, 0, 0, 0, 0]
    assert [c["nonfinite"] for c in rec["columns"]] == [1, 1] + [0] * 14
    assert rec["rows"][6] == dict(sum_rho=0.0, sum_jx=0.0, sum_jy=0.0, sum_ux=0.0, sum_uy=0.0, fluid=0, nonfinite=0)
    assert rec["rows"][3]["fluid"] == 14 and rec["columns"][6]["fluid"] == 5
    for line in rec["rows"] + rec["columns"]:
        assert all(math.isfinite(line[k]) and not (line[k] == 0.0 and math.copysign(1.0, line[k]) < 0) for k in profile_model.SUMS)
