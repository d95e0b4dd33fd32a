"""CPU checks of the vorticity and the enstrophy rows (lbm_read_vorticity, lbm_set_enstrophy, lbm_read_enstrophy and the
batch twins): exported and declared, the row's layout, the argument checks that need no device, the text writer, the
Makefile's dependency lines, "words -> row" (csrc/lbm_enstrophy_row.h, as a stand-alone program), and the numpy model the
GPU tests compare against, checked on the oracle alone.  Host-only: passes on a box without a GPU."""
import ctypes
import inspect
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import vorticity_model
from conftest import ROOT
import makefile_rules

NAMES = ("lbm_read_vorticity", "lbm_set_enstrophy", "lbm_read_enstrophy", "lbm_batch_set_enstrophy", "lbm_batch_read_enstrophy")
FIELDS = ("enstrophy", "circulation", "nonfinite", "max_abs_w", "max_x", "max_y", "fluid")


def test_enstrophy_symbols_are_exported_declared_and_listed(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS and name not in lbm.ABI_SYMBOLS_NUMBERED
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert re.fullmatch(r"lbm_[a-z_]+", name)
    assert re.search(r"int lbm_read_vorticity\(lbm_ctx\* ctx, float\* w[^,)]*\);", header)
    assert re.search(r"int lbm_set_enstrophy\(lbm_ctx\* ctx, int every, int capacity\);", header)
    assert re.search(r"int lbm_read_enstrophy\(lbm_ctx\* ctx, int max_rows, lbm_enstrophy_row\* out, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_batch_set_enstrophy\(lbm_batch\* batch, int every, int capacity\);", header)
    assert re.search(r"int lbm_batch_read_enstrophy\(lbm_batch\* batch, int max_rows, lbm_enstrophy_row\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout


def test_row_layout(lbm, tmp_path):
    """sizeof(lbm_enstrophy_row) == 40 and its field offsets, by the C compiler, against ENSTROPHY_DTYPE"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(lbm_enstrophy_row), offsetof(lbm_enstrophy_row, enstrophy),\n'
                   "         offsetof(lbm_enstrophy_row, circulation), offsetof(lbm_enstrophy_row, nonfinite), offsetof(lbm_enstrophy_row, max_abs_w),\n"
                   "         offsetof(lbm_enstrophy_row, max_x), offsetof(lbm_enstrophy_row, max_y), offsetof(lbm_enstrophy_row, fluid));\n"
                   "  return 0;\n}\n" % os.path.join(ROOT, "include", "lbm_hip.h"))
    exe = str(tmp_path / "layout")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", str(src), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [40, 0, 8, 16, 24, 28, 32, 36]
    d = lbm.ENSTROPHY_DTYPE
    assert d.itemsize == 40 and d.names == FIELDS
    assert [d.fields[k][1] for k in FIELDS] == got[1:]
    assert [d.fields[k][0] for k in FIELDS] == [np.dtype("<f8")] * 2 + [np.dtype("<i8"), np.dtype("<f4")] + [np.dtype("<i4")] * 3
    assert vorticity_model.FIELDS == FIELDS


def test_null_handles_are_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    w = np.zeros(4, dtype=np.float32)
    assert lib.lbm_read_vorticity(None, w.ctypes.data) != 0
    assert b"lbm_read_vorticity" in lib.lbm_last_error()
    assert lib.lbm_set_enstrophy(None, 10, 4) != 0
    assert b"lbm_set_enstrophy" in lib.lbm_last_error()
    assert lib.lbm_read_enstrophy(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_enstrophy" in lib.lbm_last_error()
    assert lib.lbm_batch_set_enstrophy(None, 10, 4) != 0
    assert b"lbm_batch_set_enstrophy" in lib.lbm_last_error()
    assert lib.lbm_batch_read_enstrophy(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_batch_read_enstrophy" in lib.lbm_last_error()


@pytest.mark.parametrize("every,capacity,match", [
    (1.5, 4, "every must be an integer"), (True, 4, "every must be an integer"), ("1", 4, "every must be an integer"),
    (None, 4, "every must be an integer"), (10, 2.0, "capacity must be an integer"), (10, None, "capacity must be an integer"),
    (-1, 4, r"every must lie in \[0, 2\^31\)"), (2 ** 31, 4, r"every must lie in \[0, 2\^31\)"),
    (10, -3, r"capacity must lie in \[0, 2\^31\)"), (10, 2 ** 31, r"capacity must lie in \[0, 2\^31\)"), (10, 0, "at least one row")])
def test_python_argument_checks_need_no_device(lbm, every, capacity, match):
    with pytest.raises(lbm.LbmError, match="set_enstrophy: .*" + match):
        lbm._enstrophy_args(every, capacity)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._enstrophy_args(0, 0) == (0, 0)
    assert lbm._enstrophy_args(3, 2 ** 31 - 1) == (3, 2 ** 31 - 1)
    every, capacity = lbm._enstrophy_args(np.int64(7), np.int32(2))
    assert (every, capacity) == (7, 2) and type(every) is int and type(capacity) is int


def test_method_signatures(lbm):
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.set_enstrophy)
        assert list(sig.parameters) == ["self", "every", "capacity"] and sig.parameters["capacity"].default == 4096
        assert list(inspect.signature(cls.enstrophy).parameters) == ["self", "max_rows"]
        assert inspect.signature(cls.enstrophy).parameters["max_rows"].default is None
    assert list(inspect.signature(lbm.Engine.vorticity).parameters) == ["self"]
    assert lbm.BatchMember.set_enstrophy is lbm.Engine.set_enstrophy      # a member raises the engine's refusal
    assert lbm.BatchMember.vorticity is lbm.Engine.vorticity              # ... and reads its own field
    assert list(inspect.signature(lbm.write_enstrophy).parameters) == ["path", "steps", "rows"]


def test_write_enstrophy_format(lbm, tmp_path):
    path = str(tmp_path / "enstrophy.dat")
    rows = np.zeros(2, dtype=lbm.ENSTROPHY_DTYPE)
    rows[0] = (9.25e-3, -1.5e-10, 0, 0.5, 3, 7, 124)
    rows[1] = (0.0, 0.0, 12, 0.0, -1, -1, 0)
    lbm.write_enstrophy(path, [0, 50], rows)
    assert open(path).read() == ("0:\t9.250000000000E-03\t-1.500000000000E-10\t5.000000000000E-01\t3\t7\t124\t0\n"
                                 "50:\t0.000000000000E+00\t0.000000000000E+00\t0.000000000000E+00\t-1\t-1\t0\t12\n")
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_enstrophy(path, [0], rows)
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_enstrophy(path, [0, 50], np.zeros((2, 7)))


def test_the_makefile_rebuilds_the_library_when_the_header_changes():
    csrc = os.path.join(ROOT, "lbm-asynchronous_amd", "csrc")
    assert '#include "lbm_enstrophy_row.h"' in open(os.path.join(csrc, "lbm_kernels.hip.h")).read()
    text = open(os.path.join(csrc, "lbm_enstrophy_row.h")).read()
    assert "hip_runtime" not in text and "24 words = 192 bytes" in text          # no HIP; the size is stated in the header's text
    makefile = open(os.path.join(ROOT, "lbm-asynchronous_amd", "Makefile")).read()
    for target in ("liblbm_hip.so:", "asm:", "profile-lib:"):
        line = makefile_rules.rule_line(target)
        assert "csrc/lbm_enstrophy_row.h" in line, target


# ---- words -> row -------------------------------------------------------------------------------------------------------
def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def fbits(v):
    return int(np.float32(v).view(np.uint32))


def row_cases():
    """[(nx, [slab: ([wsq terms], [w terms], bad, fluid, [(|w|, cell)])])]; what the row must be follows from all terms"""
    rng = np.random.default_rng(12)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    small = lambda n: f32(1e-2 * rng.standard_normal(n))
    wide = lambda n: f32(np.ldexp(rng.standard_normal(n), rng.integers(-140, 100, n)))
    carry = lambda n: f32(np.full(n, np.float32(4.0) - np.float32(2.0 ** -22)))   # 24 one-bits across the limbs 3 and 4: their sum carries
    cases = []
    w = small(124)
    cases.append((16, [(w * w, w, 0, 124, [(np.float32(abs(v)), i) for i, v in enumerate(w)])]))                 # one slab
    cases.append((128, [(np.abs(wide(290)), -np.abs(wide(290)), s, 290,
                         [(np.float32(0.02 + 0.001 * ((i * 7 + s) % 11)), s * 300 + i) for i in range(290)]) for s in range(3)]))  # three; a negative circulation
    cases.append((20, [(carry(300), carry(300), 0, 300, [(np.float32(4.0), 7)]), (carry(7), -carry(301), 1, 7, [(np.float32(4.0), 47)])]))  # carries; the sum turns negative
    cancel = f32([0.1, 0.1, 0.2, 3e38, 1e-45])
    cases.append((8, [(cancel, cancel, 0, 5, [(np.float32(1.0), 5)]), (cancel[:2], -cancel, 0, 5, [(np.float32(0.5), 9)])]))  # total cancellation of w
    cases.append((64, [([], [], 0, 0, []), ([], [], 0, 0, [])]))                                                   # an all-zero row: the empty key, -1, -1
    cases.append((64, [([], [], 40, 0, []), ([], [], 24, 0, []), ([], [], 5, 0, [])]))                             # nothing finite
    tie = np.float32(0.0625)
    cases.append((64, [([], [], 0, 2, [(tie, 700), (np.float32(0.06), 3)]), ([], [], 0, 2, [(tie, 130), (tie, 131)]),
                       ([], [], 0, 1, [(tie, 4000)])]))                                                            # a tie between slabs: cell 130
    cases.append((64, [([], [], 0, 2, [(np.float32(0.0), 0), (np.float32(0.0), 1)]), ([], [], 0, 1, [(np.float32(0.0), 64)])]))  # cell index 0, |w| = +0
    cases.append((65536, [([], [], 0, 1, [(np.float32(3e38), 2 ** 31 - 2)]), ([], [], 0, 1, [(np.float32(1e-45), 2 ** 31 - 1)])]))
    return cases


def row_text(nx, slabs):
    lines = ["%d %d" % (len(slabs), nx)]
    total = [[], []]
    bad, fluid, best = 0, 0, None
    for wsq, w, n_bad, n_fluid, cells in slabs:
        for j, t in enumerate((wsq, w)):
            t = np.asarray(t, dtype=np.float32)
            lines.append(" ".join(["%d" % len(t)] + ["%x" % b for b in t.view(np.uint32).tolist()]))
            total[j] += [float(v) for v in t]
        lines.append("%d %d %d" % (n_bad, n_fluid, len(cells)) + "".join(" %x %d" % (fbits(u), c) for u, c in cells))
        bad += n_bad
        fluid += n_fluid
        for u, c in cells:
            if best is None or (float(u), -c) > (float(best[0]), -best[1]):
                best = (u, c)
    u, x, y = (np.float32(0.0), -1, -1) if best is None else (best[0], best[1] % nx, best[1] // nx)
    lines.append(" ".join("%x" % dbits(math.fsum(t)) for t in total) + " %d %x %d %d %d" % (bad, fbits(u), x, y, fluid))
    return "\n".join(lines) + "\n"


def test_words_to_row(tmp_path):
    """lbm_enstrophy_row.h, built as a stand-alone program under AddressSanitizer and UBSan (as ring_check is): 1, 2 and 3
    slabs, negative sums, carries across limbs, total cancellation, the empty key, ties between slabs, a large cell index"""
    exe = str(tmp_path / "enstrophy_row_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "enstrophy_row_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    cases = row_cases()
    text = "".join(row_text(nx, slabs) for nx, slabs in cases)
    assert "\n0 0 0 0 -1 -1 0\n" in text and " 0 %x 2 2 5\n" % fbits(0.0625) in text        # the all-zero row; the tie goes to cell 130
    wants = [t.splitlines()[-1].split() for t in (row_text(nx, slabs) for nx, slabs in cases)]
    assert sum(w[1][0] in "89abcdef" and len(w[1]) == 16 for w in wants) >= 2                  # negative circulations
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, f"enstrophy_row_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert run.stdout == "%d cases, 0 failed\n" % len(cases)


# ---- the model, on the oracle alone ---------------------------------------------------------------------------------
def test_model_on_the_uniform_equilibrium(lbm, oracle):
    """every w is +0 and the row is zeros with the first fluid cell as the maximum's"""
    p = lbm.Params(16, 8, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    cells = oracle.init_cells(p)
    w, counted, bad = vorticity_model.field(cells, ob)
    assert np.all(w.view(np.uint32) == 0) and counted.all() and not bad.any()
    assert vorticity_model.row(cells, ob) == dict(enstrophy=0.0, circulation=0.0, nonfinite=0, max_abs_w=0.0, max_x=0, max_y=0, fluid=128)
    ob[0, :3] = 1
    first = vorticity_model.row(cells, ob)
    assert (first["max_x"], first["max_y"], first["fluid"]) == (3, 0, 125)          # the first FLUID cell


def test_model_circulation_of_a_periodic_lattice_is_rounding_alone(lbm, oracle):
    """without obstacles the central differences telescope over both wraps: the circulation is what the roundings of the
    differences leave, tiny against sqrt(enstrophy)"""
    p = lbm.Params(20, 6, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((6, 20), dtype=np.int32)
    rng = np.random.default_rng(3)
    cells = (oracle.init_cells(p) * (1 + 0.05 * rng.standard_normal((6, 20, 9)))).astype(np.float32)
    oracle.run(p, cells, ob, 4)
    r = vorticity_model.row(cells, ob)
    fs = oracle.final_state(p, cells, ob)
    u_max = float(max(np.abs(fs["u_x"]).max(), np.abs(fs["u_y"]).max()))
    # per cell the three roundings (of dvdx and dudy, at most 2 u_max each, and of their difference, at most 4 u_max) leave at
    # most 0.5 * 2^-24 * (2 + 2 + 4) u_max; the exact differences sum to zero
    limit = 120 * 2.0 ** -22 * u_max
    print("circulation", r["circulation"], "limit", limit, "sqrt(enstrophy)", math.sqrt(r["enstrophy"]))
    assert r["fluid"] == 120 and r["nonfinite"] == 0 and r["max_abs_w"] > 0
    assert abs(r["circulation"]) <= limit < 1e-4 * math.sqrt(r["enstrophy"])


def test_model_matches_a_cell_by_cell_evaluation(lbm, oracle):
    """np.roll against the header's text, cell by cell with explicit wraps, on a lattice with a block at a corner"""
    p = lbm.Params(7, 5, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((5, 7), dtype=np.int32)
    ob[0, 0] = ob[4, 6] = ob[2, 3] = 1
    rng = np.random.default_rng(4)
    cells = (oracle.init_cells(p) * (1 + 0.05 * rng.standard_normal((5, 7, 9)))).astype(np.float32)
    oracle.run(p, cells, ob, 3)
    fs = oracle.final_state(p, cells, ob)
    ux, uy = fs["u_x"], fs["u_y"]                                 # blocked cells 0: the oracle's final state
    assert np.all(ux[ob != 0] == 0) and np.all(uy[ob != 0] == 0)
    w = vorticity_model.field(cells, ob)[0]
    for y in range(5):
        for x in range(7):
            dvdx = np.float32(uy[y, (x + 1) % 7] - uy[y, (x - 1) % 7])
            dudy = np.float32(ux[(y + 1) % 5, x] - ux[(y - 1) % 5, x])
            want = np.float32(0.0) if ob[y, x] else np.float32(0.5) * np.float32(dvdx - dudy)
            assert np.float32(want).view(np.uint32) == w[y, x].view(np.uint32), (x, y)


def test_model_counts_a_nan_and_its_fluid_neighbours(lbm, oracle):
    p = lbm.Params(16, 8, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[3:5, 6:8] = 1
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 5)
    clean = vorticity_model.row(cells, ob)
    assert clean["nonfinite"] == 0 and clean["fluid"] == 124 and clean["enstrophy"] > 0
    one = cells.copy()
    one[6, 12, 2] = np.nan                                        # far from the block: itself and four neighbours
    r = vorticity_model.row(one, ob)
    assert r["nonfinite"] == 5 and r["fluid"] == 119
    w = vorticity_model.field(one, ob)[0]
    assert sorted(zip(*np.nonzero(np.isnan(w)))) == [(5, 12), (6, 11), (6, 13), (7, 12)]       # its own w does not read its own velocity
    beside = cells.copy()
    beside[3, 5, 7] = np.inf                                      # west of the block: one neighbour is a wall
    assert vorticity_model.row(beside, ob)["nonfinite"] == 4
    two_wide = cells.copy()
    two_wide[0, 0, :] = np.nan                                    # the corner cell: its neighbours lie across both wraps
    w = vorticity_model.field(two_wide, ob)[0]
    assert sorted(zip(*np.nonzero(np.isnan(w)))) == [(0, 1), (0, 15), (1, 0), (7, 0)]


def test_model_band_rule():
    """the host's band rule as the GPU tests mirror it: at least 8 rows, about 4096 units"""
    assert vorticity_model.band_rows(5, 16) == 8 and vorticity_model.band_rows(1024, 1024) == 8
    assert vorticity_model.band_rows(8192, 8192) == 64 and vorticity_model.strips(8192) == 32
    assert (vorticity_model.strips(63), vorticity_model.strips(64), vorticity_model.strips(65), vorticity_model.strips(260)) == (1, 1, 2, 2)
    assert vorticity_model.groups(8192, 8192) == 512 and vorticity_model.groups(5, 16) == 1
