"""CPU checks of the lattice statistics (lbm_set_stats, lbm_read_stats and their batch twins): exported and declared, the
row's layout, the argument checks that need no device, the stats.dat writer, the command line's LBM_STATS parser and its
forbidden combinations, "words -> row" (csrc/lbm_stats_row.h, as a stand-alone program), and the numpy model the GPU
tests compare against, checked on the oracle alone.  Host-only: passes on a box without a GPU."""
import ctypes
import inspect
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import stats_model
from cli_case import run_cli
from conftest import ROOT

HOST = os.path.join(ROOT, "lbm-asynchronous_amd", "host")
NAMES = ("lbm_set_stats", "lbm_read_stats", "lbm_batch_set_stats", "lbm_batch_read_stats")


def test_stats_symbols_are_exported_declared_and_listed(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert re.fullmatch(r"lbm_[a-z_]+", name)
    assert re.search(r"int lbm_set_stats\(lbm_ctx\* ctx, int every, int capacity\);", header)
    assert re.search(r"int lbm_read_stats\(lbm_ctx\* ctx, int max_rows, lbm_stats_row\* out, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_batch_set_stats\(lbm_batch\* batch, int every, int capacity\);", header)
    assert re.search(r"int lbm_batch_read_stats\(lbm_batch\* batch, int max_rows, lbm_stats_row\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout


def test_row_layout(lbm, tmp_path):
    """sizeof(lbm_stats_row) == 56 and its field offsets, by the C compiler, against STATS_DTYPE"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(lbm_stats_row), offsetof(lbm_stats_row, mass),\n'
                   "         offsetof(lbm_stats_row, mom_x), offsetof(lbm_stats_row, mom_y), offsetof(lbm_stats_row, sum_u_sq),\n"
                   "         offsetof(lbm_stats_row, nonfinite), offsetof(lbm_stats_row, max_u), offsetof(lbm_stats_row, max_x),\n"
                   "         offsetof(lbm_stats_row, max_y), offsetof(lbm_stats_row, reserved));\n  return 0;\n}\n"
                   % os.path.join(ROOT, "include", "lbm_hip.h"))
    exe = str(tmp_path / "layout")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", str(src), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [56, 0, 8, 16, 24, 32, 40, 44, 48, 52]
    d = lbm.STATS_DTYPE
    assert d.itemsize == 56
    assert [d.fields[k][1] for k in ("mass", "mom_x", "mom_y", "sum_u_sq", "nonfinite", "max_u", "max_x", "max_y", "reserved")] == got[1:]
    assert [d.fields[k][0] for k in ("mass", "nonfinite", "max_u", "max_x")] == [np.dtype("<f8"), np.dtype("<i8"), np.dtype("<f4"), np.dtype("<i4")]


def test_null_handles_are_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    assert lib.lbm_set_stats(None, 10, 4) != 0
    assert b"lbm_set_stats" in lib.lbm_last_error()
    assert lib.lbm_read_stats(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_stats" in lib.lbm_last_error()
    assert lib.lbm_batch_set_stats(None, 10, 4) != 0
    assert b"lbm_batch_set_stats" in lib.lbm_last_error()
    assert lib.lbm_batch_read_stats(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_batch_read_stats" in lib.lbm_last_error()


@pytest.mark.parametrize("every,capacity,match", [
    (1.5, 4, "every must be an integer"), (True, 4, "every must be an integer"), ("1", 4, "every must be an integer"),
    (None, 4, "every must be an integer"), (10, 2.0, "capacity must be an integer"), (10, None, "capacity must be an integer"),
    (-1, 4, r"every must lie in \[0, 2\^31\)"), (2 ** 31, 4, r"every must lie in \[0, 2\^31\)"),
    (10, -3, r"capacity must lie in \[0, 2\^31\)"), (10, 2 ** 31, r"capacity must lie in \[0, 2\^31\)"), (10, 0, "at least one row")])
def test_python_argument_checks_need_no_device(lbm, every, capacity, match):
    with pytest.raises(lbm.LbmError, match="set_stats: .*" + match):
        lbm._stats_args(every, capacity)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._stats_args(0, 0) == (0, 0)
    assert lbm._stats_args(3, 2 ** 31 - 1) == (3, 2 ** 31 - 1)
    every, capacity = lbm._stats_args(np.int64(7), np.int32(2))
    assert (every, capacity) == (7, 2) and type(every) is int and type(capacity) is int


def test_method_signatures(lbm):
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.set_stats)
        assert list(sig.parameters) == ["self", "every", "capacity"] and sig.parameters["capacity"].default == 4096
        assert list(inspect.signature(cls.stats).parameters) == ["self", "max_rows"]
        assert inspect.signature(cls.stats).parameters["max_rows"].default is None
    assert lbm.BatchMember.set_stats is lbm.Engine.set_stats      # a member raises the engine's refusal
    assert list(inspect.signature(lbm.write_stats).parameters) == ["path", "steps", "rows"]


def test_write_stats_format(lbm, tmp_path):
    path = str(tmp_path / "stats.dat")
    rows = np.zeros(2, dtype=lbm.STATS_DTYPE)
    rows[0] = (1638.25, 1.5, -2.0, 0.125, 0, 0.5, 3, 7, 0)
    rows[1] = (-1e-3, 0.0, 3.0, 0.0, 12, 0.0, -1, -1, 0)
    lbm.write_stats(path, [0, 50], rows)
    assert open(path).read() == ("0:\t1.638250000000E+03\t1.500000000000E+00\t-2.000000000000E+00\t1.250000000000E-01\t5.000000000000E-01\t3\t7\t0\n"
                                 "50:\t-1.000000000000E-03\t0.000000000000E+00\t3.000000000000E+00\t0.000000000000E+00\t0.000000000000E+00\t-1\t-1\t12\n")
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_stats(path, [0], rows)
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_stats(path, [0, 50], np.zeros((2, 9)))


# ---- words -> row -------------------------------------------------------------------------------------------------------
def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def fbits(v):
    return int(np.float32(v).view(np.uint32))


def row_cases():
    """[(nx, [slab: ([rho terms], [jx], [jy], [usq], bad, [(umag, cell)])])]; what the row must be follows from all terms"""
    rng = np.random.default_rng(5)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    pops = lambda n: f32(0.1 * (1 + 0.05 * rng.standard_normal(n)))
    wide = lambda n: f32(np.ldexp(rng.standard_normal(n), rng.integers(-140, 120, n)))
    cases = []
    cases.append((16, [(pops(128), f32(1e-3 * rng.standard_normal(120)), wide(120), f32(rng.random(120) * 1e-4), 0,
                        [(np.float32(0.01 * (i % 7)), i) for i in range(120)])]))                      # one slab
    cases.append((128, [(pops(300), wide(290), -np.abs(wide(290)), f32(rng.random(290)), s,
                         [(np.float32(0.02 + 0.001 * ((i * 7 + s) % 11)), s * 300 + i) for i in range(290)]) for s in range(3)]))  # three; a negative momentum
    cancel = f32([0.1, 0.1, 0.2, 3e38, 1e-45])
    cases.append((8, [(cancel, cancel, cancel[:3], cancel[:2], 0, [(np.float32(1.0), 5)]),
                      (-cancel, -cancel, -cancel[:3], -cancel[:2], 0, [(np.float32(0.5), 9)])]))        # total cancellation
    cases.append((64, [([], [], [], [], 0, []), ([], [], [], [], 0, [])]))                                # an all-zero row: 0, -1, -1
    cases.append((64, [([], [], [], [], 40, []), ([], [], [], [], 24, [])]))                              # nothing finite
    tie = np.float32(0.0625)
    cases.append((64, [(pops(4), [], [], [], 0, [(tie, 700), (np.float32(0.06), 3)]), (pops(4), [], [], [], 0, [(tie, 130), (tie, 131)]),
                       (pops(4), [], [], [], 0, [(tie, 4000)])]))                                         # a tie between slabs: cell 130
    cases.append((64, [(pops(2), [], [], [], 0, [(np.float32(0.0), 0), (np.float32(0.0), 1)]), (pops(2), [], [], [], 0, [(np.float32(0.0), 64)])]))  # cell index 0, |u| = +0
    cases.append((65536, [(pops(2), [], [], [], 0, [(np.float32(3e38), 2 ** 31 - 2)]), (pops(2), [], [], [], 0, [(np.float32(1e-45), 2 ** 31 - 1)])]))
    cases.append((65535, [(pops(2), [], [], [], 0, [(np.float32(1e-45), 2 ** 31 - 2)])]))                # the smallest |u| above 0, a large cell
    return cases


def row_text(nx, slabs):
    lines = ["%d %d" % (len(slabs), nx)]
    total = [[], [], [], []]
    bad, best = 0, None
    for rho, jx, jy, usq, n_bad, cells in slabs:
        for j, t in enumerate((rho, jx, jy, usq)):
            t = np.asarray(t, dtype=np.float32)
            lines.append(" ".join(["%d" % len(t)] + ["%x" % b for b in t.view(np.uint32).tolist()]))
            total[j] += [float(v) for v in t]
        lines.append("%d %d" % (n_bad, len(cells)) + "".join(" %x %d" % (fbits(u), c) for u, c in cells))
        bad += n_bad
        for u, c in cells:
            if best is None or (float(u), -c) > (float(best[0]), -best[1]):
                best = (u, c)
    u, x, y = (np.float32(0.0), -1, -1) if best is None else (best[0], best[1] % nx, best[1] // nx)
    lines.append(" ".join("%x" % dbits(math.fsum(t)) for t in total) + " %d %x %d %d" % (bad, fbits(u), x, y))
    return "\n".join(lines) + "\n"


def test_words_to_row(tmp_path):
    """lbm_stats_row.h, built as a stand-alone program under AddressSanitizer and UBSan (as forces_sum_check is): one and
    three slabs, a negative momentum, total cancellation, an all-zero row, ties between slabs, cell indices 0 and 2^31 - 2"""
    exe = str(tmp_path / "stats_row_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "stats_row_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    cases = row_cases()
    text = "".join(row_text(nx, slabs) for nx, slabs in cases)
    assert "\n0 0 0 0 0 0 -1 -1\n" in text and " 0 %x 2 2\n" % fbits(0.0625) in text        # the all-zero row; the tie goes to cell 130
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, f"stats_row_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert run.stdout == "%d cases, 0 failed\n" % len(cases)


# ---- the model, on the oracle alone ---------------------------------------------------------------------------------
def small_case(lbm, nx=16, ny=8, accel=0.005):
    p = lbm.Params(nx, ny, 100, 10, 0.1, accel, 1.85)
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[3:5, 6:8] = 1
    return p, ob


def test_model_velocities_are_the_oracles_final_state(lbm, oracle):
    p, ob = small_case(lbm)
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 20)
    _, _, _, ux, uy, _, umag = stats_model.moments(cells)
    want = oracle.final_state(p, cells, ob)
    fluid = ob == 0
    for got, key in ((ux, "u_x"), (uy, "u_y"), (umag, "u")):
        assert np.array_equal(got[fluid].view(np.uint32), want[key][fluid].view(np.uint32)), key


def test_model_on_the_uniform_equilibrium_and_after_acceleration(lbm, oracle):
    p, ob = small_case(lbm)
    cells = oracle.init_cells(p)
    r = stats_model.row(cells, ob)
    assert r["mom_x"] == 0.0 and r["mom_y"] == 0.0 and r["max_u"] == 0.0 and (r["max_x"], r["max_y"]) == (0, 0)
    assert r["nonfinite"] == 0 and r["mass"] > 0.0
    ob2 = ob.copy()
    ob2[0, :3] = 1
    first = stats_model.row(cells, ob2)
    assert (first["max_x"], first["max_y"]) == (3, 0)                # the first FLUID cell
    oracle.run(p, cells, ob, 20)
    r = stats_model.row(cells, ob)
    assert r["mom_x"] > 0.0 and r["max_u"] > 0.0 and r["sum_u_sq"] > 0.0
    # the mass within the bound of a plain double sum of the same terms
    rho = stats_model.moments(cells)[0]
    plain = 0.0
    for v in rho.reshape(-1):
        plain += float(v)
    limit = stats_model.bound(cells, ob)["mass"]
    assert abs(r["mass"] - plain) <= limit and limit < 1e-12
    assert abs(r["mass"] - float(rho.astype(np.float64).sum())) <= limit


def test_model_leaves_nonfinite_cells_out(lbm):
    p, ob = small_case(lbm)
    cells = np.full((8, 16, 9), 0.01, dtype=np.float32)
    clean = stats_model.row(cells, ob)
    cells[0, 0, 1] = np.inf                      # fluid
    cells[3, 6, 4] = np.nan                      # blocked
    cells[1, 1, :] = 0.0                         # rho = 0: u is 0 / 0
    r = stats_model.row(cells, ob)
    assert r["nonfinite"] == 3 and abs(r["mass"] - (clean["mass"] - 3 * 0.09)) < 1e-6
    cells[:] = np.nan
    r = stats_model.row(cells, ob)
    assert r == dict(mass=0.0, mom_x=0.0, mom_y=0.0, sum_u_sq=0.0, nonfinite=128, max_u=0.0, max_x=-1, max_y=-1)


# ---- the command line ---------------------------------------------------------------------------------------------------
EARLIER = [("LBM_PRECISION=double", {"LBM_PRECISION": "double"}), ("LBM_STEADY", {"LBM_STEADY": "1e-6"}),
           ("LBM_PROBES", {"LBM_PROBES": "1,2"}), ("LBM_ANIMATION", {"LBM_ANIMATION": "100"}), ("LBM_MEAN", {"LBM_MEAN": "10:2"}),
           ("LBM_STATES", {"LBM_STATES": "10"}), ("LBM_FORCES", {"LBM_FORCES": "50"})]
OUTPUTS = ("av_vels.dat", "final_state.dat", "animation_data", "state_data", "probes.dat", "forces.dat", "stats.dat")


@pytest.mark.parametrize("earlier,env", EARLIER, ids=[name for name, _ in EARLIER])
def test_cli_refuses_each_pair_before_any_device_is_touched(lbm, tmp_path, earlier, env):
    out = run_cli(lbm, tmp_path, LBM_STATS="50", **env)
    message = ("LBM_STATS is not offered with LBM_PRECISION=double" if earlier == "LBM_PRECISION=double"
               else "%s and LBM_STATS cannot be combined" % earlier)
    assert out.returncode == 1
    assert re.fullmatch(r"Error at line \d+ of file .*:\n%s\n" % re.escape(message), out.stderr), out.stderr
    assert "no HIP device" not in out.stderr
    assert sorted(os.listdir(tmp_path)) == ["input.params", "obstacles.dat"]


@pytest.mark.parametrize("value", ["-5", "ten", "10x", "2147483648", "0", "10 ", "+10", "1e2", "10:2"])
def test_cli_refuses_malformed_values_before_any_device_is_touched(lbm, tmp_path, value):
    out = run_cli(lbm, tmp_path, LBM_STATS=value)
    assert out.returncode == 1
    assert re.fullmatch(r"Error at line \d+ of file .*lbm_options\.c:\ncould not read LBM_STATS: expected <every> with every >= 1\n", out.stderr), out.stderr
    assert sorted(os.listdir(tmp_path)) == ["input.params", "obstacles.dat"]
    for name in OUTPUTS:
        assert not (tmp_path / name).exists()


def test_valid_values_parse(tmp_path):
    """tests/stats_options_check.c over lbm_options.c and lbm_io.c alone, a stand-alone program under AddressSanitizer and UBSan"""
    exe = str(tmp_path / "stats_options_check")
    cmd = ["gcc", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "stats_options_check.c"), os.path.join(HOST, "lbm_options.c"), os.path.join(HOST, "lbm_io.c"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    for env, expect in (({"LBM_STATS": "1"}, "stats=1 mode=7 of 8 every=1 double=0"), ({"LBM_STATS": "2147483647"}, "stats=1 mode=7 of 8 every=2147483647 double=0"),
                        ({"LBM_STATS": "50", "LBM_GPUS": "2", "LBM_TILE": "32x16", "LBM_OUTPUT": "none"}, "stats=1 mode=7 of 8 every=50 double=0"),
                        ({"LBM_STATS": "", "LBM_FORCES": "5"}, "stats=0 mode=6 of 8 every=5 double=0"), ({}, "stats=0 mode=0 of 8 every=0 double=0"),
                        ({"LBM_STATS": "", "LBM_PRECISION": "double"}, "stats=0 mode=0 of 8 every=0 double=1")):
        run = subprocess.run([exe] + ["%s=%s" % kv for kv in env.items()], capture_output=True, text=True)
        assert (run.returncode, run.stderr, run.stdout) == (0, "", expect + "\n"), (env, run.stderr)
