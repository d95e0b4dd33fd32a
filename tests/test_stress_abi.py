"""CPU checks of the stress fields and the stress rows (lbm_read_stress, lbm_set_stress, lbm_read_stress_rows and the
batch twins): exported and declared, the row's layout, the Python helpers and their refusal at omega == 1, the text
writer, the Makefile's dependency lines, "words -> row" (csrc/lbm_stress_row.h, as a stand-alone program, plain and
sanitized), and the numpy model the GPU tests compare against: on constructed lattices with a prescribed stress, its
float32 accuracy against the derived bounds, and its strain rate against central differences of the velocity, on the
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

import stress_model
from conftest import ROOT, dataset
import makefile_rules

NAMES = ("lbm_read_stress", "lbm_set_stress", "lbm_read_stress_rows", "lbm_batch_set_stress", "lbm_batch_read_stress_rows")
FIELDS = ("sum_q", "sum_txy", "nonfinite", "max_q", "max_x", "max_y", "fluid")


def test_stress_symbols_are_exported_declared_and_listed(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS and name not in lbm.ABI_SYMBOLS_NUMBERED
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert re.fullmatch(r"lbm_[a-z_]+", name)
    assert re.search(r"int lbm_read_stress\(lbm_ctx\* ctx, float\* txx[^,)]*, float\* txy[^,)]*, float\* tyy[^,)]*\);", header)
    assert re.search(r"int lbm_set_stress\(lbm_ctx\* ctx, int every, int capacity\);", header)
    assert re.search(r"int lbm_read_stress_rows\(lbm_ctx\* ctx, int max_rows, lbm_stress_row\* out, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_batch_set_stress\(lbm_batch\* batch, int every, int capacity\);", header)
    assert re.search(r"int lbm_batch_read_stress_rows\(lbm_batch\* batch, int max_rows, lbm_stress_row\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout


def test_the_header_states_the_definition_and_what_is_not_offered():
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    text = header[header.index("---- stress and dissipation"):header.index("} lbm_stress_row;")]
    flat = " ".join(text.replace("*", " ").split())
    for line in ("a56 = f5+f6 a78 = f7+f8", "mxx = ((f1+f3)+a56)+a78 myy = ((f2+f4)+a56)+a78 mxy = (f5+f7)-(f6+f8)", "third = rho / 3.0f",
                 "pxx = (mxx-third)-(jx ux) pyy = (myy-third)-(jy uy) pxy = mxy-(jx uy)", "txx = pxx/rho tyy = pyy/rho txy = pxy/rho",
                 "q = ((txx txx)+(tyy tyy)) + (2.0f (txy txy))"):
        assert line in flat, line
    assert "c = 3 omega / (2 (1 - omega))" in flat and "omega == 1" in flat
    for word in ("a d2q9-bgk mode", "the double engine", "rank contexts", "recording inside the resident or stream kernels",
                 "the pre-collision stress"):
        assert word in flat[flat.index("Not offered"):], word


def test_row_layout(lbm, tmp_path):
    """sizeof(lbm_stress_row) == 40 and its field offsets, by the C compiler, against STRESS_DTYPE"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(lbm_stress_row), offsetof(lbm_stress_row, sum_q),\n'
                   "         offsetof(lbm_stress_row, sum_txy), offsetof(lbm_stress_row, nonfinite), offsetof(lbm_stress_row, max_q),\n"
                   "         offsetof(lbm_stress_row, max_x), offsetof(lbm_stress_row, max_y), offsetof(lbm_stress_row, fluid));\n"
                   "  return 0;\n}\n" % os.path.join(ROOT, "include", "lbm_hip.h"))
    exe = str(tmp_path / "layout")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", str(src), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [40, 0, 8, 16, 24, 28, 32, 36]
    d = lbm.STRESS_DTYPE
    assert d.itemsize == 40 and d.names == FIELDS
    assert [d.fields[k][1] for k in FIELDS] == got[1:]
    assert [d.fields[k][0] for k in FIELDS] == [np.dtype("<f8")] * 2 + [np.dtype("<i8"), np.dtype("<f4")] + [np.dtype("<i4")] * 3
    assert [d.fields[k] for k in FIELDS] == [lbm.ENSTROPHY_DTYPE.fields[k] for k in lbm.ENSTROPHY_DTYPE.names]   # lbm_enstrophy_row's layout
    assert stress_model.FIELDS == FIELDS


def test_null_handles_are_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    t = np.zeros(4, dtype=np.float32)
    assert lib.lbm_read_stress(None, t.ctypes.data, None, None) != 0
    assert b"lbm_read_stress" in lib.lbm_last_error()
    assert lib.lbm_set_stress(None, 10, 4) != 0
    assert b"lbm_set_stress" in lib.lbm_last_error()
    assert lib.lbm_read_stress_rows(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_stress_rows" in lib.lbm_last_error()
    assert lib.lbm_batch_set_stress(None, 10, 4) != 0
    assert b"lbm_batch_set_stress" in lib.lbm_last_error()
    assert lib.lbm_batch_read_stress_rows(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_batch_read_stress_rows" in lib.lbm_last_error()


def test_method_signatures(lbm):
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.set_stress)
        assert list(sig.parameters) == ["self", "every", "capacity"] and sig.parameters["capacity"].default == 4096
        assert list(inspect.signature(cls.stress_rows).parameters) == ["self", "max_rows"]
        assert inspect.signature(cls.stress_rows).parameters["max_rows"].default is None
    assert list(inspect.signature(lbm.Engine.stress).parameters) == ["self"]
    assert lbm.BatchMember.set_stress is lbm.Engine.set_stress        # a member raises the engine's refusal
    assert lbm.BatchMember.stress is lbm.Engine.stress                # ... and reads its own fields
    assert list(inspect.signature(lbm.write_stress_rows).parameters) == ["path", "steps", "rows"]
    for fn, first in ((lbm.strain_rate, "stress"), (lbm.dissipation, "rows"), (lbm.shear_rate_max, "rows")):
        assert list(inspect.signature(fn).parameters) == [first, "omega"]


def test_write_stress_rows_format(lbm, tmp_path):
    path = str(tmp_path / "stress.dat")
    rows = np.zeros(2, dtype=lbm.STRESS_DTYPE)
    rows[0] = (9.25e-3, -1.5e-10, 0, 0.5, 3, 7, 124)
    rows[1] = (0.0, 0.0, 12, 0.0, -1, -1, 0)
    lbm.write_stress_rows(path, [0, 50], rows)
    assert open(path).read() == ("0:\t9.250000000000E-03\t-1.500000000000E-10\t5.000000000000E-01\t3\t7\t124\t0\n"
                                 "50:\t0.000000000000E+00\t0.000000000000E+00\t0.000000000000E+00\t-1\t-1\t0\t12\n")
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_stress_rows(path, [0], rows)
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_stress_rows(path, [0, 50], np.zeros((2, 7)))


def test_the_helpers_convert_with_the_post_collision_factor(lbm):
    omega = 1.85
    c = 3 * omega / (2 * (1 - omega))
    nu = (1 / omega - 0.5) / 3
    t = {"txx": np.float32([[1e-3, -2e-3]]), "txy": np.float32([[5e-4, 0.0]]), "tyy": np.float32([[-1e-3, 2e-3]])}
    s = lbm.strain_rate(t, omega)
    assert sorted(s) == ["S_xx", "S_xy", "S_yy"] and all(v.dtype == np.float64 and v.shape == (1, 2) for v in s.values())
    assert np.array_equal(s["S_xy"], -c * t["txy"].astype(np.float64)) and np.array_equal(s["S_xx"], -c * t["txx"].astype(np.float64))
    assert c < 0 and s["S_xy"][0, 0] > 0                    # above omega = 1 the stored stress has the strain rate's sign
    assert lbm.strain_rate(t, 0.5)["S_xy"][0, 0] == -1.5 * float(t["txy"][0, 0])
    rows = np.zeros(2, dtype=lbm.STRESS_DTYPE)
    rows["sum_q"] = (2.5e-3, 0.0)
    rows["max_q"] = (8e-6, 0.0)
    assert np.array_equal(lbm.dissipation(rows, omega), 2 * nu * c * c * rows["sum_q"])
    assert np.array_equal(lbm.shear_rate_max(rows, omega), abs(c) * np.sqrt(2 * rows["max_q"].astype(np.float64)))
    assert lbm.dissipation(rows, omega)[0] > 0 and lbm.dissipation(rows, omega).dtype == np.float64


@pytest.mark.parametrize("omega", [1.0, np.float32(1.0), 0.0, 2.0, -0.5, 2.5, float("nan")])
def test_the_helpers_refuse_omega_one_and_omega_outside_0_2(lbm, omega):
    t = {k: np.zeros((2, 2), dtype=np.float32) for k in ("txx", "txy", "tyy")}
    rows = np.zeros(1, dtype=lbm.STRESS_DTYPE)
    match = "pure equilibrium" if omega == 1.0 else r"outside \(0, 2\)"
    for fn, arg in ((lbm.strain_rate, t), (lbm.dissipation, rows), (lbm.shear_rate_max, rows)):
        with pytest.raises(ValueError, match=fn.__name__ + ": .*" + match):
            fn(arg, omega)


def test_the_makefile_rebuilds_the_library_when_the_header_changes():
    csrc = os.path.join(ROOT, "lbm-asynchronous_amd", "csrc")
    assert '#include "lbm_stress_row.h"' in open(os.path.join(csrc, "lbm_kernels.hip.h")).read()
    text = open(os.path.join(csrc, "lbm_stress_row.h")).read()
    assert "hip_runtime" not in text and "24 words = 192 bytes" in text          # no HIP; the size is stated in the header's text
    for target in ("liblbm_hip.so:", "asm:", "profile-lib:"):
        line = makefile_rules.rule_line(target)
        assert "csrc/lbm_stress_row.h" in line, target


# ---- words -> row -------------------------------------------------------------------------------------------------------
def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def fbits(v):
    return int(np.float32(v).view(np.uint32))


def row_cases():
    """[(nx, [slab: ([q terms], [txy terms], bad, fluid, [(q, cell)])])]; what the row must be follows from all terms"""
    rng = np.random.default_rng(21)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    small = lambda n: f32(1e-3 * rng.standard_normal(n))
    wide = lambda n: f32(np.ldexp(rng.standard_normal(n), rng.integers(-140, 100, n)))
    carry = lambda n: f32(np.full(n, np.float32(4.0) - np.float32(2.0 ** -22)))   # 24 one-bits across two limbs: their sum carries
    cases = []
    t = small(124)
    q = f32(2) * t * t
    cases.append((16, [(q, t, 0, 124, [(v, i) for i, v in enumerate(q)])]))                                       # one slab
    cases.append((32, [(np.abs(wide(90)), -np.abs(wide(90)), s, 90, [(np.float32(1e-6 * ((i * 5 + s) % 13)), s * 100 + i) for i in range(90)])
                       for s in range(2)]))                                                                       # two; a negative sum_txy
    cases.append((128, [(np.abs(wide(290)), -np.abs(wide(290)), s, 290,
                         [(np.float32(0.02 + 0.001 * ((i * 7 + s) % 11)), s * 300 + i) for i in range(290)]) for s in range(3)]))  # three; negative again
    cases.append((20, [(carry(300), carry(300), 0, 300, [(np.float32(4.0), 7)]), (carry(7), -carry(301), 1, 7, [(np.float32(4.0), 47)])]))  # carries; the sum turns negative
    cancel = f32([0.1, 0.1, 0.2, 3e38, 1e-45])
    cases.append((8, [(cancel, cancel, 0, 5, [(np.float32(1.0), 5)]), (cancel[:2], -cancel, 0, 5, [(np.float32(0.5), 9)])]))  # total cancellation of txy
    cases.append((64, [([], [], 0, 0, [])]))                                                                       # an empty lattice on one slab
    cases.append((64, [([], [], 0, 0, []), ([], [], 0, 0, []), ([], [], 0, 0, [])]))                               # ... and on three: the empty key, -1, -1
    cases.append((64, [([], [], 40, 0, []), ([], [], 24, 0, []), ([], [], 5, 0, [])]))                             # nothing finite
    tie = np.float32(0.0625)
    cases.append((64, [([], [], 0, 2, [(tie, 700), (np.float32(0.06), 3)]), ([], [], 0, 2, [(tie, 130), (tie, 131)]),
                       ([], [], 0, 1, [(tie, 4000)])]))                                                            # a tie across three slabs: cell 130
    cases.append((64, [([], [], 0, 1, [(tie, 900)]), ([], [], 0, 1, [(tie, 899)])]))                               # ... across two, the later slab's cell first
    cases.append((64, [([], [], 0, 2, [(np.float32(0.0), 0), (np.float32(0.0), 1)]), ([], [], 0, 1, [(np.float32(0.0), 64)])]))  # cell index 0, q = +0
    cases.append((65536, [([], [], 0, 1, [(np.float32(3e38), 2 ** 31 - 2)]), ([], [], 0, 1, [(np.float32(1e-45), 2 ** 31 - 1)])]))
    return cases


def row_text(nx, slabs):
    lines = ["%d %d" % (len(slabs), nx)]
    total = [[], []]
    bad, fluid, best = 0, 0, None
    for q, txy, n_bad, n_fluid, cells in slabs:
        for j, t in enumerate((q, txy)):
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


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                                             "-static-libubsan"]], ids=["plain", "sanitized"])
def test_words_to_row(tmp_path, flags):
    """lbm_stress_row.h, built as a stand-alone program, plain and under AddressSanitizer and UBSan (as stats_row_check is):
    1, 2 and 3 slabs, negative sum_txy, carries across limbs, total cancellation, an empty lattice, ties across slabs, a
    large cell index"""
    exe = str(tmp_path / "stress_row_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "stress_row_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    cases = row_cases()
    assert {len(slabs) for _, slabs in cases} == {1, 2, 3}
    texts = [row_text(nx, slabs) for nx, slabs in cases]
    text = "".join(texts)
    assert "\n0 0 0 0 -1 -1 0\n" in text and " 0 %x 2 2 5\n" % fbits(0.0625) in text        # the empty row; the tie goes to cell 130
    assert " 0 %x 3 14 2\n" % fbits(0.0625) in text                                          # ... and to cell 899 = 14 * 64 + 3
    wants = [t.splitlines()[-1].split() for t in texts]
    assert sum(w[1][0] in "89abcdef" and len(w[1]) == 16 for w in wants) >= 3                  # negative sum_txy
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, f"stress_row_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert run.stdout == "%d cases, 0 failed\n" % len(cases)


# ---- the model on constructed lattices ----------------------------------------------------------------------------------
STATES = [(1.0, 0.0, 0.0), (0.9, 0.08, -0.03), (0.1, -0.05, 0.05), (1.7, 0.2, 0.1), (0.5, 0.0, -0.15)]
TENSORS = [(0.0, 0.0, 0.0), (1e-3, 0.0, -1e-3), (0.0, 2e-3, 0.0), (-4e-3, 7e-4, 2.5e-3), (1e-2, -1e-2, 1e-2), (3e-7, -1e-7, 2e-7)]


def test_the_definition_returns_a_prescribed_stress_in_float64():
    """f = feq(rho, u) + (9/2) w_k (c_ka c_kb - delta_ab / 3) rho A_ab has t = A and the equilibrium's rho and j"""
    for rho, ux, uy in STATES:
        for axx, axy, ayy in TENSORS:
            v = stress_model.evaluate(stress_model.constructed(rho, ux, uy, axx, axy, ayy)[None, None, :], np.float64)
            got = [float(v[k][0, 0]) for k in ("rho", "ux", "uy", "txx", "txy", "tyy")]
            assert np.allclose(got, [rho, ux, uy, axx, axy, ayy], rtol=0, atol=1e-12), (rho, ux, uy, axx, axy, ayy, got)
            want_q = axx * axx + ayy * ayy + 2 * axy * axy
            assert abs(float(v["q"][0, 0]) - want_q) <= 1e-12


def test_a_pure_equilibrium_carries_no_stress(lbm, oracle):
    for rho, ux, uy in STATES:
        f = stress_model.constructed(rho, ux, uy, 0.0, 0.0, 0.0)[None, None, :]
        v = stress_model.evaluate(f, np.float64)
        assert max(abs(float(v[k][0, 0])) for k in ("txx", "txy", "tyy")) <= 1e-15          # to float64 rounding
        v32 = stress_model.evaluate(f.astype(np.float32))
        e = stress_model.t_bounds(stress_model.evaluate(f.astype(np.float32), np.float64))  # ... and to float32's, by the derived bounds
        for k, b in zip(("txx", "tyy", "txy"), e):
            assert abs(float(v32[k][0, 0])) <= float(b[0, 0]) + 1e-12 < 1e-6
    p = lbm.Params(16, 8, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    r = stress_model.row(oracle.init_cells(p), ob)                       # the oracle's initial lattice: equilibrium at rest
    assert r["fluid"] == 128 and r["nonfinite"] == 0 and r["sum_q"] < 128 * 3 * (5 * 2.0 ** -24) ** 2


def test_model_counts_non_finite_cells(lbm, oracle):
    p = lbm.Params(16, 8, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[3:5, 6:8] = 1
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 5)
    clean = stress_model.row(cells, ob)
    assert clean["nonfinite"] == 0 and clean["fluid"] == 124 and clean["sum_q"] > 0 and clean["max_q"] > 0
    one = cells.copy()
    one[6, 12, 2] = np.nan                                        # pointwise: the cell itself and no neighbour
    r = stress_model.row(one, ob)
    assert r["nonfinite"] == 1 and r["fluid"] == 123
    t = stress_model.field(one, ob)[0]
    assert all(sorted(zip(*np.nonzero(np.isnan(t[k])))) == [(6, 12)] for k in ("txx", "txy", "tyy"))   # stored as computed
    empty = cells.copy()
    empty[2, 3, :] = 0.0                                          # rho == 0: 0 / 0
    r = stress_model.row(empty, ob)
    assert r["nonfinite"] == 1 and r["fluid"] == 123 and np.isnan(stress_model.field(empty, ob)[0]["txy"][2, 3])
    wall = cells.copy()
    wall[3, 6, 4] = np.nan                                        # a blocked cell contributes to nothing and is not counted
    assert stress_model.same_bits(np.array([tuple(clean[k] for k in FIELDS)], dtype=lbm.STRESS_DTYPE)[0], stress_model.row(wall, ob)) == []
    assert all(np.all(stress_model.field(wall, ob)[0][k][ob != 0] == 0) for k in ("txx", "txy", "tyy"))
    blocked = np.ones((8, 16), dtype=np.int32)
    assert stress_model.row(cells, blocked) == dict(sum_q=0.0, sum_txy=0.0, nonfinite=0, fluid=0, max_q=0.0, max_x=-1, max_y=-1)


def test_model_takes_the_first_of_equal_maxima(lbm, oracle):
    """an x-invariant lattice: every cell of a row has the same q, the key is the row's first cell"""
    p = lbm.Params(12, 6, 100, 10, 0.1, 0.005, 1.85)
    f = np.stack([stress_model.constructed(1.0, 0.02 * y, 0.0, 0.0, 1e-3 * (1 + (y % 3)), 0.0) for y in range(6)])
    cells = np.repeat(f[:, None, :], 12, axis=1).astype(np.float32)
    r = stress_model.row(cells, np.zeros((6, 12), dtype=np.int32))
    assert (r["max_x"], r["max_y"]) == (0, 2) and r["fluid"] == 72


# ---- the model on the oracle's 128^2 lattice after 4000 steps -----------------------------------------------------------
@pytest.fixture(scope="module")
def cavity(oracle):
    """(Params, obstacles [ny, nx], the oracle's lattice after 4000 steps) of the reference's 128 x 128 data set"""
    p, ob = dataset("128x128")
    ob = np.asarray(ob).reshape(p.ny, p.nx)
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 4000)
    cells.setflags(write=False)
    return p, ob, cells


def test_float32_accuracy_holds_the_derived_bounds(cavity):
    """|t_ab(float32) - t_ab(float64)| against the bounds derived from the expression tree (stress_model.t_bounds; DESIGN.md,
    "Stress and dissipation"), cell by cell, with the derived counts and no fitted constant.  Measured on this lattice
    (rho about 0.1, |u| up to 0.053): the diagonal terms differ by at most 1.69 * 2^-24 where the bound is 4.8 * 2^-24
    (1.01e-8 in pxx and pyy), txy by at most 0.096 * 2^-24 where it is 0.22 * 2^-24 (5.4e-10 in pxy), and the float32 sum
    of q lies 3.1e-8 relative from the float64 one."""
    p, ob, cells = cavity
    fluid = ob == 0
    v32, v64 = stress_model.evaluate(cells), stress_model.evaluate(cells, np.float64)
    # what the derivation assumes: non-negative populations, and mxx - third exact by Sterbenz' lemma
    assert cells[fluid].min() >= 0
    for m in ("mxx", "myy"):
        assert np.all((v32[m][fluid] <= 2 * v32["third"][fluid]) & (v32["third"][fluid] <= 2 * v32[m][fluid]))
        assert np.array_equal((v32[m] - v32["third"]).astype(np.float64)[fluid], (v32[m].astype(np.float64) - v32["third"].astype(np.float64))[fluid])
    bounds = stress_model.t_bounds(v64)
    unit = stress_model.U
    worst = {}
    for name, b in zip(("txx", "tyy", "txy"), bounds):
        d = np.abs(v32[name].astype(np.float64) - v64[name])[fluid]
        worst[name] = (d.max() / unit, b[fluid].max() / unit, (d / b[fluid]).max())
        print(name, "largest difference %.3f, largest bound %.3f (units of 2^-24), largest difference / bound %.3f" % worst[name])
        assert np.all(d <= b[fluid]), name
    # the bounds say what the text says: a few units of 2^-24 on the diagonal -- the cancellation of mxx - rho/3 keeps the
    # roundings of rho/3 whatever txx is -- and a fraction of one for txy; and they are not vacuous
    assert 3 < worst["txx"][1] < 7 and 3 < worst["tyy"][1] < 7 and worst["txy"][1] < 0.5
    assert worst["txx"][0] > 1 and worst["txx"][0] > 10 * worst["txy"][0]
    assert min(w[2] for w in worst.values()) > 0.1
    dq = np.abs(v32["q"].astype(np.float64) - v64["q"])[fluid]
    qb = stress_model.q_bound(v64, *bounds)[fluid]
    assert np.all(dq <= qb)
    sum32, sum64 = math.fsum(float(v) for v in v32["q"][fluid]), math.fsum(v64["q"][fluid].tolist())
    print("sum_q: float32 terms %.12e, float64 terms %.12e, relative %.3e, bound %.3e" % (sum32, sum64, abs(sum32 - sum64) / sum64, qb.sum() / sum64))
    assert abs(sum32 - sum64) <= qb.sum() < 1e-3 * sum64


def interior(fluid):
    """the cells whose neighbours within two cells in x and y are all fluid, at least three rows from the top and the bottom"""
    ok = np.ones_like(fluid)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ok &= np.roll(np.roll(fluid, dy, axis=0), dx, axis=1)
    ok[:3] = False
    ok[-3:] = False
    return ok


def test_the_strain_rate_agrees_with_central_differences_of_the_velocity(lbm, oracle, cavity):
    """S_xy from the second moment against 0.25 * ((ux(y+1) - ux(y-1)) + (uy(x+1) - uy(x-1))): second-order agreement with
    the post-collision factor 1 / (1 - omega), none without it"""
    p, ob, cells = cavity
    t = stress_model.field(cells, ob)[0]
    s_xy = lbm.strain_rate(t, p.omega)["S_xy"]
    fs = oracle.final_state(p, np.array(cells), ob)
    ux, uy = fs["u_x"].astype(np.float64), fs["u_y"].astype(np.float64)
    fd = 0.25 * ((np.roll(ux, -1, axis=0) - np.roll(ux, 1, axis=0)) + (np.roll(uy, -1, axis=1) - np.roll(uy, 1, axis=1)))
    sel = interior(ob == 0)
    assert sel.sum() > 0.8 * ob.size
    rel = lambda a: math.sqrt(((a[sel] - fd[sel]) ** 2).sum() / (fd[sel] ** 2).sum())
    with_factor = rel(s_xy)
    forgotten = rel(-(3 * p.omega / 2) * t["txy"].astype(np.float64))          # c = 3 omega / 2
    print("relative rms difference: %.4f with 1 / (1 - omega), %.4f without" % (with_factor, forgotten))
    assert with_factor < 0.15
    assert not forgotten < 0.15
    # the dissipation of the row is that of the field
    r = stress_model.row(cells, ob)
    rows = np.array([tuple(r[k] for k in FIELDS)], dtype=lbm.STRESS_DTYPE)
    s = lbm.strain_rate(t, p.omega)
    nu = (1 / float(p.omega) - 0.5) / 3
    direct = 2 * nu * (s["S_xx"] ** 2 + s["S_yy"] ** 2 + 2 * s["S_xy"] ** 2)[ob == 0].sum()
    assert lbm.dissipation(rows, p.omega)[0] == pytest.approx(direct, rel=1e-6) and direct > 0
    peak = np.sqrt(2 * (s["S_xx"] ** 2 + s["S_yy"] ** 2 + 2 * s["S_xy"] ** 2))[r["max_y"], r["max_x"]]
    assert lbm.shear_rate_max(rows, p.omega)[0] == pytest.approx(peak, rel=1e-6)
