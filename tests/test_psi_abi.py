"""CPU checks of the stream function and its rows (lbm_read_psi, lbm_set_psi, lbm_read_psi_rows and the batch twins):
exported and declared, the row's layout, the argument checks that need no device, the two text writers, the Makefile's
dependency lines, "words -> row" and the device twin of the rounding (csrc/lbm_psi_row.h and csrc/lbm_exact_round.h, as a
stand-alone program), and the integer model the GPU tests compare against, checked on the oracle alone.  Host-only: passes
on a box without a GPU."""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import psi_model
from conftest import ROOT
import makefile_rules

NAMES = ("lbm_read_psi", "lbm_set_psi", "lbm_read_psi_rows", "lbm_batch_set_psi", "lbm_batch_read_psi_rows")
FIELDS = ("psi_min", "psi_max", "nonfinite", "min_x", "min_y", "max_x", "max_y", "fluid", "reserved")


def test_psi_symbols_are_exported_declared_and_listed(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS and name not in lbm.ABI_SYMBOLS_NUMBERED
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert re.fullmatch(r"lbm_[a-z_]+", name)
    assert re.search(r"int lbm_read_psi\(lbm_ctx\* ctx, double\* psi[^,)]*\);", header)
    assert re.search(r"int lbm_set_psi\(lbm_ctx\* ctx, int every, int capacity\);", header)
    assert re.search(r"int lbm_read_psi_rows\(lbm_ctx\* ctx, int max_rows, lbm_psi_row\* out, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_batch_set_psi\(lbm_batch\* batch, int every, int capacity\);", header)
    assert re.search(r"int lbm_batch_read_psi_rows\(lbm_batch\* batch, int max_rows, lbm_psi_row\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout
    for said in ("psi of u", "trapezoid weights", "the double engine", "rank contexts", "inside the resident or stream kernels", "d2q9-bgk"):
        assert said in header                                                                  # what is not offered is said


def test_row_layout(lbm, tmp_path):
    """sizeof(lbm_psi_row) == 48 and its field offsets, by the C compiler, against PSI_DTYPE"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu", sizeof(lbm_psi_row));\n' % os.path.join(ROOT, "include", "lbm_hip.h")
                   + "".join('  printf(" %%zu", offsetof(lbm_psi_row, %s));\n' % k for k in FIELDS) + '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", str(src), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [48, 0, 8, 16, 24, 28, 32, 36, 40, 44]
    d = lbm.PSI_DTYPE
    assert d.itemsize == 48 and d.names == FIELDS
    assert [d.fields[k][1] for k in FIELDS] == got[1:]
    assert [d.fields[k][0] for k in FIELDS] == [np.dtype("<f8")] * 2 + [np.dtype("<i8")] + [np.dtype("<i4")] * 6
    assert psi_model.FIELDS == FIELDS


def test_null_handles_are_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    psi = np.zeros(4, dtype=np.float64)
    assert lib.lbm_read_psi(None, psi.ctypes.data) != 0
    assert b"lbm_read_psi" in lib.lbm_last_error()
    assert lib.lbm_set_psi(None, 10, 4) != 0
    assert b"lbm_set_psi" in lib.lbm_last_error()
    assert lib.lbm_read_psi_rows(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_psi_rows" in lib.lbm_last_error()
    assert lib.lbm_batch_set_psi(None, 10, 4) != 0
    assert b"lbm_batch_set_psi" in lib.lbm_last_error()
    assert lib.lbm_batch_read_psi_rows(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_batch_read_psi_rows" in lib.lbm_last_error()


@pytest.mark.parametrize("every,capacity,match", [
    (1.5, 4, "every must be an integer"), (True, 4, "every must be an integer"), ("1", 4, "every must be an integer"),
    (None, 4, "every must be an integer"), (10, 2.0, "capacity must be an integer"), (10, None, "capacity must be an integer"),
    (-1, 4, r"every must lie in \[0, 2\^31\)"), (2 ** 31, 4, r"every must lie in \[0, 2\^31\)"),
    (10, -3, r"capacity must lie in \[0, 2\^31\)"), (10, 2 ** 31, r"capacity must lie in \[0, 2\^31\)"), (10, 0, "at least one row")])
def test_python_argument_checks_need_no_device(lbm, every, capacity, match):
    with pytest.raises(lbm.LbmError, match="set_psi: .*" + match):
        lbm._psi_args(every, capacity)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._psi_args(0, 0) == (0, 0)
    assert lbm._psi_args(3, 2 ** 31 - 1) == (3, 2 ** 31 - 1)
    every, capacity = lbm._psi_args(np.int64(7), np.int32(2))
    assert (every, capacity) == (7, 2) and type(every) is int and type(capacity) is int


def test_method_signatures(lbm):
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.set_psi)
        assert list(sig.parameters) == ["self", "every", "capacity"] and sig.parameters["capacity"].default == 4096
        assert list(inspect.signature(cls.psi_rows).parameters) == ["self", "max_rows"]
        assert inspect.signature(cls.psi_rows).parameters["max_rows"].default is None
    assert list(inspect.signature(lbm.Engine.psi).parameters) == ["self"]
    assert lbm.BatchMember.set_psi is lbm.Engine.set_psi      # a member raises the engine's refusal
    assert lbm.BatchMember.psi is lbm.Engine.psi              # ... and reads its own field
    assert list(inspect.signature(lbm.write_psi_rows).parameters) == ["path", "steps", "rows"]
    assert list(inspect.signature(lbm.write_psi).parameters) == ["path", "psi"]


def test_write_psi_rows_format(lbm, tmp_path):
    path = str(tmp_path / "psi_rows.dat")
    rows = np.zeros(2, dtype=lbm.PSI_DTYPE)
    rows[0] = (-9.25e-3, 1.5e-10, 0, 3, 7, 60, 2, 124, 0)
    rows[1] = (0.0, 0.0, 12, -1, -1, -1, -1, 0, 0)
    lbm.write_psi_rows(path, [0, 50], rows)
    assert open(path).read() == ("0:\t-9.250000000000E-03\t1.500000000000E-10\t3\t7\t60\t2\t124\t0\n"
                                 "50:\t0.000000000000E+00\t0.000000000000E+00\t-1\t-1\t-1\t-1\t0\t12\n")
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_psi_rows(path, [0], rows)
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_psi_rows(path, [0, 50], np.zeros((2, 9)))


def test_write_psi_format(lbm, tmp_path):
    path = str(tmp_path / "psi.dat")
    lbm.write_psi(path, np.array([[0.0, -1.5e-3, 2.0 ** -60], [1.0, 2.0 ** 60, -0.25]]))
    assert open(path).read() == ("0 0 0.000000000000E+00\n1 0 -1.500000000000E-03\n2 0 8.673617379884E-19\n"
                                 "0 1 1.000000000000E+00\n1 1 1.152921504607E+18\n2 1 -2.500000000000E-01\n")
    with pytest.raises(lbm.LbmError, match="psi must be"):
        lbm.write_psi(path, np.zeros(6))
    with pytest.raises(lbm.LbmError, match="psi must be"):
        lbm.write_psi(path, np.zeros((2, 3), dtype=np.float32))


def test_the_makefile_rebuilds_the_library_when_the_headers_change():
    csrc = os.path.join(ROOT, "lbm-asynchronous_amd", "csrc")
    kernels = open(os.path.join(csrc, "lbm_kernels.hip.h")).read()
    assert '#include "lbm_psi_row.h"' in kernels and '#include "lbm_exact_round.h"' in kernels
    text = open(os.path.join(csrc, "lbm_psi_row.h")).read()
    assert "hip_runtime" not in text and "8 words = 64 bytes" in text              # no HIP; the size is stated in the header's text
    until = open(os.path.join(csrc, "lbm_residual_until.h")).read()
    assert '#include "lbm_exact_round.h"' in until and "double exact_sum_round_hd(" not in until    # moved, not copied
    assert "double exact_sum_round_hd(" in open(os.path.join(csrc, "lbm_exact_round.h")).read()
    makefile = open(os.path.join(ROOT, "lbm-asynchronous_amd", "Makefile")).read()
    for target in ("liblbm_hip.so:", "asm:", "profile-lib:"):
        line = makefile_rules.rule_line(target)
        assert "csrc/lbm_psi_row.h" in line and "csrc/lbm_exact_round.h" in line, target
    line = next(l for l in makefile.splitlines() if l.startswith("psi-check:"))
    for dep in ("../tests/psi_row_check.cpp", "csrc/lbm_psi_row.h", "csrc/lbm_exact_round.h", "csrc/lbm_exact_sum.h"):
        assert dep in line


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_words_to_row_and_the_rounding_twin(tmp_path, sanitize):
    """tests/psi_row_check.cpp as a program of its own, once plain and once under AddressSanitizer and UBSan (as
    enstrophy_row_check is built; nothing is preloaded): lbm_psi_row.h on random and edge words, exact_sum_round_hd against
    exact_sum_round on running prefixes, carries, negative totals, ties to even and random limbs"""
    exe = str(tmp_path / "psi_row_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    cmd += [os.path.join(ROOT, "tests", "psi_row_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, f"psi_row_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert re.fullmatch(r"\d{5,} checks, 0 failed\n", run.stdout), run.stdout


# ---- the model, on the oracle alone ---------------------------------------------------------------------------------
def lattice(lbm, oracle, nx, ny, steps, seed, blocks=()):
    p = lbm.Params(nx, ny, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((ny, nx), dtype=np.int32)
    for y, x in blocks:
        ob[y, x] = 1
    rng = np.random.default_rng(seed)
    cells = (oracle.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    oracle.run(p, cells, ob, steps)
    return p, ob, cells


def test_model_every_prefix_is_fsum_of_its_terms(lbm, oracle):
    """16 x 12 with a block: each psi equals math.fsum of the terms below and at it; the last row is the column's total"""
    p, ob, cells = lattice(lbm, oracle, 16, 12, 4, 5, blocks=[(3, 4), (3, 5), (4, 4), (11, 0)])
    t, counted, bad = psi_model.terms(cells, ob)
    psi, _, _ = psi_model.field(cells, ob)
    assert not bad.any() and counted.sum() == 16 * 12 - 4 and np.any(t != 0)
    for x in range(16):
        for y in range(12):
            want = math.fsum(float(v) for v in t[:y + 1, x])
            assert np.float64(want).view(np.uint64) == psi[y, x].view(np.uint64), (x, y)
    assert all(psi[-1, x] == math.fsum(float(v) for v in t[:, x]) for x in range(16))


def test_model_jx_is_the_profiles_jx(lbm, oracle):
    """jx in the header's order, cell by cell, and psi[ny - 1] against the exact column sums of jx"""
    p, ob, cells = lattice(lbm, oracle, 7, 5, 3, 6, blocks=[(2, 3)])
    t, counted, _ = psi_model.terms(cells, ob)
    g = cells.reshape(5, 7, 9)
    for y in range(5):
        for x in range(7):
            jx = np.float32(np.float32(np.float32(g[y, x, 1] + g[y, x, 5]) + g[y, x, 8]) - np.float32(np.float32(g[y, x, 3] + g[y, x, 6]) + g[y, x, 7]))
            want = np.float32(0.0) if ob[y, x] else jx
            assert want.view(np.uint32) == t[y, x].view(np.uint32), (x, y)


def test_model_a_blocked_cell_with_populations_adds_nothing(lbm, oracle):
    p, ob, cells = lattice(lbm, oracle, 16, 12, 6, 7, blocks=[(5, 8)])
    g = cells.reshape(12, 16, 9)
    jx_blocked = float(g[5, 8, 1] + g[5, 8, 5] + g[5, 8, 8] - (g[5, 8, 3] + g[5, 8, 6] + g[5, 8, 7]))
    assert jx_blocked != 0.0                                      # rebounded populations: a non-zero jx inside the wall
    psi, counted, _ = psi_model.field(cells, ob)
    assert not counted[5, 8]
    assert psi[5, 8].view(np.uint64) == psi[4, 8].view(np.uint64)  # inside a wall psi is the wall's constant
    r = psi_model.row(cells, ob)
    assert r["fluid"] == 16 * 12 - 1 and (r["min_x"], r["min_y"]) != (8, 5) and (r["max_x"], r["max_y"]) != (8, 5)


def cancellation_lattice(nx, ny, x, rows):
    """cells_aos [ny, nx, 9] at rest (g0 = 1) but for column x, whose cells at the three `rows` carry jx = 2^60, 2^-60 and
    -2^60 exactly: only g1 or only g3 is non-zero there, so jx is that population and ux = +-1"""
    cells = np.zeros((ny, nx, 9), dtype=np.float32)
    cells[:, :, 0] = 1.0
    for y, (k, v) in zip(rows, ((1, 2.0 ** 60), (1, 2.0 ** -60), (3, 2.0 ** 60))):
        cells[y, x, :] = 0.0
        cells[y, x, k] = v
    return cells


def test_model_differs_from_a_float64_cumsum_on_the_cancellation_lattice():
    """2^60, 2^-60, -2^60 down one column: the exact prefix after the third term is 2^-60, a float64 running sum gives 0 --
    the GPU test can tell limbs from a double accumulator"""
    ob = np.zeros((12, 16), dtype=np.int32)
    cells = cancellation_lattice(16, 12, 5, (2, 6, 9))
    t, counted, bad = psi_model.terms(cells, ob)
    assert counted.all() and not bad.any()
    assert [float(t[y, 5]) for y in (2, 6, 9)] == [2.0 ** 60, 2.0 ** -60, -2.0 ** 60]
    psi, _, _ = psi_model.field(cells, ob)
    assert psi[9, 5] == 2.0 ** -60 and psi[11, 5] == 2.0 ** -60 and psi[6, 5] == 2.0 ** 60 and psi[1, 5] == 0.0
    naive = np.cumsum(t.astype(np.float64), axis=0)
    assert naive[9, 5] == 0.0 and not np.array_equal(naive.view(np.uint64), psi.view(np.uint64))
    r = psi_model.row(cells, ob)
    assert (r["psi_max"], r["max_x"], r["max_y"]) == (2.0 ** 60, 5, 2) and (r["psi_min"], r["min_x"], r["min_y"]) == (0.0, 0, 0)


def test_model_nonfinite_cells_add_nothing_and_ties_go_to_the_first_cell(lbm, oracle):
    p = lbm.Params(16, 8, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    cells = oracle.init_cells(p)
    assert psi_model.row(cells, ob) == dict(psi_min=0.0, psi_max=0.0, nonfinite=0, min_x=0, min_y=0, max_x=0, max_y=0, fluid=128, reserved=0)
    ob[0, :3] = 1
    first = psi_model.row(cells, ob)
    assert (first["min_x"], first["min_y"], first["max_x"], first["max_y"], first["fluid"]) == (3, 0, 3, 0, 125)   # the first FLUID cell
    assert psi_model.row(cells, np.ones((8, 16), dtype=np.int32)) == dict(psi_min=0.0, psi_max=0.0, nonfinite=0, min_x=-1, min_y=-1,
                                                                         max_x=-1, max_y=-1, fluid=0, reserved=0)
    p2, ob2, run = lattice(lbm, oracle, 16, 8, 5, 8)
    clean, _, _ = psi_model.field(run, ob2)
    bad_cells = run.copy().reshape(8, 16, 9)
    bad_cells[3, 7, 2] = np.inf
    psi, counted, bad = psi_model.field(bad_cells, ob2)
    assert bad.sum() == 1 and bad[3, 7] and not counted[3, 7] and np.isfinite(psi).all()
    t = psi_model.terms(run, ob2)[0]
    for y in range(3, 8):                                          # the cells above carry the prefix without it
        want = math.fsum(float(v) for yy, v in enumerate(t[:y + 1, 7]) if yy != 3)
        assert psi[y, 7] == want
    assert np.array_equal(np.delete(psi, 7, axis=1).view(np.uint64), np.delete(clean, 7, axis=1).view(np.uint64))


def test_model_band_rule():
    """the host's band rule as the GPU tests mirror it: at least 8 rows, about 1024 workgroups of 256 columns"""
    assert psi_model.band_rows(5, 16) == 8 and psi_model.band_rows(1024, 1024) == 8 and psi_model.band_rows(128, 128) == 8
    assert psi_model.band_rows(8192, 8192) == 256 and psi_model.band_rows(37, 262, override=8) == 8
    assert psi_model.band_rows(4096, 8192) == 128
