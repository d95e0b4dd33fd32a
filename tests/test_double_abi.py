"""CPU checks of the double engine's boundary (lbm_double_* of include/lbm_hip.h): the symbols exist and are listed, the
create call fails loudly without a device and on bad parameters, and the host program's parser keeps the run constants as
doubles."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG_DIR, ROOT

DOUBLE_SYMBOLS = (
    "lbm_double_create", "lbm_double_destroy", "lbm_double_get_info", "lbm_double_run", "lbm_double_run_timed",
    "lbm_double_sync", "lbm_double_read_av_vels", "lbm_double_read_cells", "lbm_double_read_final_state",
    "lbm_double_av_velocity", "lbm_double_total_density", "lbm_double_calc_reynolds")


def test_double_symbols_are_declared_exported_and_listed(lbm):
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lbm_double_[a-z_]+)\s*\(", header))
    assert declared == set(DOUBLE_SYMBOLS)
    lib = ctypes.CDLL(lbm.LIB_PATH)
    for name in DOUBLE_SYMBOLS:
        assert hasattr(lib, name), f"liblbm_hip.so does not export {name}"
        assert name in lbm.ABI_SYMBOLS
    # a handle type of its own, and the struct the issue of precision turns on: three doubles
    assert "typedef struct lbm_double_ctx lbm_double_ctx;" in header
    assert ctypes.sizeof(lbm._CParamsDouble) == 4 * 4 + 3 * 8
    assert lbm._CParamsDouble.density.offset == 16


def test_double_create_fails_loudly_without_device_or_with_bad_args(lbm, datasets):
    """No CPU fallback in double either."""
    p32, ob = datasets("128x128")
    p = lbm.ParamsDouble(p32.nx, p32.ny, p32.max_iters, p32.reynolds_dim, 0.1, 0.005, 1.85)
    if lbm.device_count() == 0:
        with pytest.raises(lbm.LbmError, match="no HIP device"):
            lbm.DoubleEngine(p, ob)
    for bad in (lbm.ParamsDouble(0, 128, 10, 10, 0.1, 0.005, 1.85), lbm.ParamsDouble(128, 1, 10, 10, 0.1, 0.005, 1.85),
                lbm.ParamsDouble(128, 128, -1, 10, 0.1, 0.005, 1.85)):
        with pytest.raises(lbm.LbmError, match="invalid parameters"):
            lbm.DoubleEngine(bad, np.zeros((bad.ny, bad.nx), dtype=np.int32))
    with pytest.raises(lbm.LbmError, match="obstacles has"):
        lbm.DoubleEngine(p, ob[:-1])
    lib = lbm.load_library()
    huge = lbm.ParamsDouble(65536, 65536, 1, 10, 0.1, 0.005, 1.85)   # more cells than the reference's int counts
    dummy = np.zeros(4, dtype=np.int32)
    assert not lib.lbm_double_create(ctypes.byref(huge._c()), dummy.ctypes.data, None)
    assert b"invalid parameters" in lib.lbm_last_error()
    assert not lib.lbm_double_create(ctypes.byref(p._c()), None, None)
    assert b"obstacles is NULL" in lib.lbm_last_error()
    # NULL handles are refused, not dereferenced
    assert lib.lbm_double_run(None, 1) != 0 and b"null context" in lib.lbm_last_error()
    assert lib.lbm_double_sync(None) != 0
    out = ctypes.c_double()
    assert lib.lbm_double_av_velocity(None, ctypes.byref(out)) != 0
    lib.lbm_double_destroy(None)


def test_python_reader_keeps_doubles(lbm):
    p = lbm.read_params_double(os.path.join(GOLDEN, "inputs", "input_128x128.params"))
    p32 = lbm.read_params(os.path.join(GOLDEN, "inputs", "input_128x128.params"))
    assert (p.nx, p.ny, p.max_iters, p.reynolds_dim) == (p32.nx, p32.ny, p32.max_iters, p32.reynolds_dim)
    c = p._c()
    assert c.omega == p.omega and c.omega != float(np.float32(p.omega))
    assert p32._c().omega == float(np.float32(p.omega))


def test_c_parser_reads_doubles_and_writers_print_them(tmp_path):
    """host/lbm_io.c: 1.85 is parsed as the double 1.85, not as (double)1.85f; the double writers print %.12E of the
    doubles (a value rounded through float shows in the eighth digit)."""
    so = tmp_path / "liblbm_io_check.so"
    subprocess.run(["gcc", "-std=c99", "-O1", "-fopenmp", "-shared", "-fPIC", "-D_POSIX_C_SOURCE=200809L", "-D_DEFAULT_SOURCE",
                    os.path.join(PKG_DIR, "host", "lbm_io.c"), "-o", str(so)], check=True)
    io = ctypes.CDLL(str(so))

    class P(ctypes.Structure):
        _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("max_iters", ctypes.c_int), ("reynolds_dim", ctypes.c_int),
                    ("density", ctypes.c_double), ("accel", ctypes.c_double), ("omega", ctypes.c_double)]

    (tmp_path / "in.params").write_text("16\n8\n10\n7\n0.1\n0.005\n1.85\n")
    p = P()
    io.lbm_read_params_double(str(tmp_path / "in.params").encode(), ctypes.byref(p))
    assert (p.nx, p.ny, p.max_iters, p.reynolds_dim) == (16, 8, 10, 7)
    assert p.density == 0.1 and p.accel == 0.005 and p.omega == 1.85
    assert p.omega != float(np.float32(1.85))

    av = np.array([0.1, 1.85, 1.0 / 3.0], dtype=np.float64)
    io.lbm_write_av_vels_double(str(tmp_path / "av.dat").encode(), av.ctypes.data_as(ctypes.c_void_p), 3)
    assert (tmp_path / "av.dat").read_text() == "".join("%d:\t%.12E\n" % (i, v) for i, v in enumerate(av))
    assert "1.850000000000E+00" in (tmp_path / "av.dat").read_text()       # (double)1.85f prints 1.850000023842E+00

    p.nx, p.ny = 2, 2
    fields = [np.array([0.1, 0.2, 0.3, 1.0 / 3.0], dtype=np.float64) * (k + 1) for k in range(4)]
    ob = np.array([0, 1, 0, 0], dtype=np.int32)
    libc = ctypes.CDLL(None)
    libc.fopen.restype = ctypes.c_void_p
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [ctypes.c_void_p]
    fp = libc.fopen(str(tmp_path / "fs.dat").encode(), b"w")
    io.lbm_write_final_state_rows_double.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    io.lbm_write_final_state_rows_double(fp, ctypes.addressof(p), 0, 2, *(f.ctypes.data for f in fields), ob.ctypes.data)
    libc.fclose(fp)
    want = "".join("%d %d %.12E %.12E %.12E %.12E %d\n" % (i % 2, i // 2, fields[0][i], fields[1][i], fields[2][i], fields[3][i], ob[i])
                   for i in range(4))
    assert (tmp_path / "fs.dat").read_text() == want
