"""CPU checks of the obstacle forces (lbm_set_forces, lbm_read_forces, lbm_forces_links): exported and declared, the
argument checks that need no device, the forces.dat writer, the command line's LBM_FORCES parser and its forbidden
combinations, the exact sum the engine takes (csrc/lbm_exact_sum.h, as a stand-alone program), and the numpy model the
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

import forces_model
from cli_case import run_cli
from conftest import ROOT


def test_forces_symbols_are_exported_and_declared(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in ("lbm_set_forces", "lbm_read_forces", "lbm_forces_links"):
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
    assert re.search(r"int lbm_set_forces\(lbm_ctx\* ctx, int n_bodies, const int\* body_of_cell[^,]*, int every, int capacity\);", header)
    assert re.search(r"int lbm_read_forces\(lbm_ctx\* ctx, int max_rows, double\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_forces_links\(lbm_ctx\* ctx, int\* links_per_body[^,)]*\);", header)
    assert re.search(r"#define LBM_MAX_BODIES\s+64\b", header) and lbm.LBM_MAX_BODIES == 64
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout


def test_null_context_is_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    assert lib.lbm_set_forces(None, 1, None, 10, 4) != 0
    assert b"lbm_set_forces" in lib.lbm_last_error()
    assert lib.lbm_read_forces(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_forces" in lib.lbm_last_error()
    assert lib.lbm_forces_links(None, None) != 0
    assert b"lbm_forces_links" in lib.lbm_last_error()


LABELS = np.zeros((8, 16), dtype=np.int32)


@pytest.mark.parametrize("every,capacity,bodies,n_bodies,match", [
    (1.5, 4, None, None, "every must be an integer"), (True, 4, None, None, "every must be an integer"),
    ("1", 4, None, None, "every must be an integer"), (None, 4, None, None, "every must be an integer"),
    (10, 2.0, None, None, "capacity must be an integer"), (10, None, None, None, "capacity must be an integer"),
    (-1, 4, None, None, r"every must lie in \[0, 2\^31\)"), (2 ** 31, 4, None, None, r"every must lie in \[0, 2\^31\)"),
    (10, -3, None, None, r"capacity must lie in \[0, 2\^31\)"), (10, 0, None, None, "at least one row"),
    (10, 4, np.zeros((8, 15), dtype=np.int32), None, "integer array of shape"), (10, 4, np.zeros((8, 16)), None, "integer array of shape"),
    (10, 4, "walls", None, "integer array of shape"), (10, 4, np.zeros(16, dtype=np.int32), None, "integer array of shape"),
    (10, 4, LABELS + 64, None, "65 bodies, between 1 and LBM_MAX_BODIES = 64"), (10, 4, LABELS, 0, "0 bodies, between 1 and"),
    (10, 4, None, 65, "65 bodies"), (10, 4, None, 2.0, "n_bodies must be an integer"), (10, 4, None, True, "n_bodies must be an integer")])
def test_python_argument_checks_need_no_device(lbm, every, capacity, bodies, n_bodies, match):
    with pytest.raises(lbm.LbmError, match=match):
        lbm._forces_args(every, capacity, bodies, n_bodies, 16, 8)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._forces_args(0, 0, None, None, 16, 8) == (0, 0, 1, None)
    assert lbm._forces_args(3, 2 ** 31 - 1, None, 64, 16, 8) == (3, 2 ** 31 - 1, 64, None)
    lab = LABELS.copy()
    lab[2, 3] = 5
    lab[0, 0] = -1              # a label outside the range: the engine refuses it if the cell is blocked
    every, capacity, n_bodies, flat = lbm._forces_args(np.int64(7), np.int32(2), lab.astype(np.int64), None, 16, 8)
    assert (every, capacity, n_bodies) == (7, 2, 6) and type(every) is int and type(n_bodies) is int
    assert flat.dtype == np.int32 and flat.flags.c_contiguous and flat.shape == (128,) and flat[2 * 16 + 3] == 5 and flat[0] == -1
    assert lbm._forces_args(7, 2, lab.reshape(-1), 9, 16, 8)[2] == 9


def test_engine_signatures(lbm):
    sig = inspect.signature(lbm.Engine.set_forces)
    assert list(sig.parameters)[:4] == ["self", "every", "capacity", "bodies"]
    assert sig.parameters["capacity"].default == 4096 and sig.parameters["bodies"].default is None
    assert sig.parameters["capacity"].default == inspect.signature(lbm.Engine.set_probes).parameters["capacity"].default
    assert list(inspect.signature(lbm.Engine.forces).parameters) == ["self", "max_rows"]
    assert list(inspect.signature(lbm.Engine.force_links).parameters) == ["self"]


def test_write_forces_format(lbm, tmp_path):
    path = str(tmp_path / "forces.dat")
    rows = np.array([[[1.5, -2.0], [0.25, 1.0]], [[-1e-3, 3.0], [0.0, 0.0]]])
    lbm.write_forces(path, [0, 50], rows)
    assert open(path).read() == "0:\t1.750000000000E+00\t-1.000000000000E+00\n50:\t-1.000000000000E-03\t3.000000000000E+00\n"
    with pytest.raises(lbm.LbmError, match="rows must be"):
        lbm.write_forces(path, [0], rows)


# ---- the exact sum ----------------------------------------------------------------------------------------------------
def sum_cases():
    rng = np.random.default_rng(11)
    cases = []

    def add(values, signs):
        values = np.asarray(values, dtype=np.float32)
        want = math.fsum(float(v) * int(s) for v, s in zip(values, signs))
        cases.append((values.view(np.uint32).tolist(), [int(s) for s in signs], struct.unpack("<Q", struct.pack("<d", want))[0]))
    add([], [])
    add([0.0, -0.0], [1, -1])
    add([1.0], [0])
    add([np.float32(1e-45)], [1])                          # the smallest denormal
    add([np.float32(1e-45)] * 3 + [np.float32(3.4e38)], [1, 1, -1, 1])
    add([np.float32(3.4028235e38)] * 64, [1] * 64)          # beyond FLT_MAX, far inside the doubles
    add([np.float32(3.4028235e38)] * 7, [-1] * 7)
    add([1.0, np.float32(2.0 ** -53)], [1, 1])              # a tie: to even (1.0)
    add([1.0, np.float32(2.0 ** -53), np.float32(1e-45)], [1, 1, 1])   # a tie broken by a sticky bit
    add([1.0, np.float32(2.0 ** -52), np.float32(2.0 ** -53)], [1, 1, 1])   # a tie: to even, upwards
    add([1.0, np.float32(2.0 ** -53)], [-1, -1])
    add([0.1, 0.1, 0.2], [1, 1, -1])                        # cancels to exactly 0
    for n in (2, 20, 257, 5000):
        w = np.float32(0.1) * np.array([1 / 9, 1 / 36], dtype=np.float32)[rng.integers(0, 2, n)]
        add(w * (1 + 0.05 * rng.standard_normal(n)).astype(np.float32), rng.integers(-1, 2, n))       # populations
        add(np.ldexp(rng.standard_normal(n), rng.integers(-140, 120, n)).astype(np.float32), rng.integers(-1, 2, n))  # every binade
    return cases


def test_exact_sum_equals_fsum(tmp_path):
    """lbm_exact_sum.h, built as a stand-alone program under AddressSanitizer and UBSan (as own_check is): terms dealt to
    four accumulators that are added afterwards give math.fsum's bits -- zeros, denormals, sums beyond FLT_MAX, ties with
    and without sticky bits, negative totals, total cancellation, populations, and floats of every binade."""
    exe = str(tmp_path / "forces_sum_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "forces_sum_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    text = "".join("%d\n%s%x\n" % (len(v), "".join("%x %d\n" % (b, s) for b, s in zip(v, sg)), want) for v, sg, want in sum_cases())
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, f"forces_sum_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"


# ---- the model, on the oracle alone -------------------------------------------------------------------------------
def small_case(lbm, nx=16, ny=8, accel=0.005):
    p = lbm.Params(nx, ny, 100, 10, 0.1, accel, 1.85)
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[3:5, 6:8] = 1
    return p, ob


def test_link_count_of_an_isolated_block(lbm):
    p, ob = small_case(lbm)
    ls = forces_model.links(ob)
    assert len(ls) == 20 and forces_model.link_counts(ob) == [20]      # 4 cells x (2 faces + 3 diagonals)
    assert ls == sorted(ls) and all(ob[y, x] for _, y, x, _ in ls)
    assert [(y, x, k) for _, y, x, k in ls[:5]] == [(3, 6, 3), (3, 6, 4), (3, 6, 6), (3, 6, 7), (3, 6, 8)]


def test_links_over_the_periodic_wraps(lbm):
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[0, 0] = 1
    ls = forces_model.links(ob)
    assert len(ls) == 8                                             # every neighbour is fluid, five of them over a wrap
    ob[0, 15] = 1                                                   # the west neighbour, over the x wrap
    ob[7, 0] = 1                                                    # the south neighbour, over the y wrap
    ks = {k for _, y, x, k in forces_model.links(ob) if (y, x) == (0, 0)}
    assert ks == {1, 2, 5, 6, 7, 8}
    ob[7, 15] = 1                                                   # the south-west neighbour, over both
    assert {k for _, y, x, k in forces_model.links(ob) if (y, x) == (0, 0)} == {1, 2, 5, 6, 8}


def test_uniform_equilibrium_gives_exactly_zero(lbm, oracle):
    p, ob = small_case(lbm)
    ob[0, 0] = ob[0, 15] = ob[7, 0] = ob[7, 15] = 1                  # a second symmetric block, over both wraps
    cells = oracle.init_cells(p)
    f = forces_model.force(cells, ob)
    assert f.shape == (1, 2) and f[0, 0] == 0.0 and f[0, 1] == 0.0


def test_accelerated_flow_pushes_the_block_downstream(lbm, oracle):
    p, ob = small_case(lbm)
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 20)
    f = forces_model.force(cells, ob)
    assert f[0, 0] > 0.0


def test_labelled_bodies_add_up_to_the_unlabelled_force(lbm, oracle):
    p, ob = small_case(lbm)
    ob[1, 12] = ob[6, 2:4] = 1
    bodies = np.zeros_like(ob)
    bodies[6, 2:4] = 1
    bodies[1, 12] = 1
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 20)
    whole, both = forces_model.force(cells, ob), forces_model.force(cells, ob, bodies, 2)
    limit = forces_model.bound(cells, ob)
    assert forces_model.link_counts(ob, bodies, 2) == [20, 8 + 14] and forces_model.link_counts(ob) == [42]
    for j in range(2):
        assert abs(both[0, j] + both[1, j] - whole[0, j]) <= limit[0, j]
        assert both[1, j] != 0.0


# ---- the command line ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,match", [
    ({"LBM_FORCES": "-5"}, "LBM_FORCES"), ({"LBM_FORCES": "ten"}, "LBM_FORCES"), ({"LBM_FORCES": "10x"}, "LBM_FORCES"),
    ({"LBM_FORCES": "50", "LBM_PRECISION": "double"}, "LBM_PRECISION=double"),
    ({"LBM_FORCES": "50", "LBM_ANIMATION": "100"}, "LBM_ANIMATION"), ({"LBM_FORCES": "50", "LBM_PROBES": "3,4"}, "LBM_PROBES"),
    ({"LBM_FORCES": "50", "LBM_MEAN": "10"}, "LBM_MEAN"), ({"LBM_FORCES": "50", "LBM_STATES": "100"}, "LBM_STATES"),
    ({"LBM_FORCES": "50", "LBM_STEADY": "1e-6"}, "LBM_STEADY")])
def test_command_line_refuses_bad_values_and_combinations(lbm, tmp_path, env, match):
    """Refused while the environment is read, before a device is looked for."""
    out = run_cli(lbm, tmp_path, **env)
    assert out.returncode != 0
    assert match in out.stderr and "LBM_FORCES" in out.stderr, out.stderr
    assert not os.path.exists(tmp_path / "forces.dat")
