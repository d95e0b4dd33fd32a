"""CPU checks of the point-probe entry points (lbm_set_probes, lbm_read_probes): exported, declared, their structs laid
out as the header says, every argument check that needs no device made before any device call, the probes.dat writer
and the command line's LBM_PROBES parser.  Host-only: passes on a box without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from cli_case import MALFORMED, run_cli
from conftest import ROOT


def test_probe_symbols_are_exported_and_declared(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in ("lbm_set_probes", "lbm_read_probes"):
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)


def test_structs_match_the_header(lbm):
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    assert re.search(r"typedef struct \{ int x, y; \} lbm_probe;", header)
    assert re.search(r"typedef struct \{ float u_x, u_y, u_mag, pressure; \} lbm_probe_sample;", header)
    assert int(re.search(r"#define LBM_MAX_PROBES (\d+)", header).group(1)) == lbm.LBM_MAX_PROBES == 256
    assert [n for n, _ in lbm._CProbe._fields_] == ["x", "y"]
    assert [n for n, _ in lbm._CProbeSample._fields_] == ["u_x", "u_y", "u_mag", "pressure"]
    assert ctypes.sizeof(lbm._CProbe) == 8 and ctypes.sizeof(lbm._CProbeSample) == 16
    # the C side: the host program is built against the header; its struct sizes are the compiler's
    src = "#include <stdio.h>\n#include \"lbm_hip.h\"\nint main(void){printf(\"%zu %zu\\n\", sizeof(lbm_probe), sizeof(lbm_probe_sample));return 0;}\n"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "sizes.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "sizes")
        subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["8", "16"]
    # lbm_info / lbm_batch_info keep their layout: what a host needs it gets from lbm_read_probes(NULL, NULL)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4


def test_null_context_is_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int()
    cells = (lbm._CProbe * 1)()
    assert lib.lbm_set_probes(None, 1, cells, 1, 4) != 0
    assert b"lbm_set_probes" in lib.lbm_last_error()
    assert lib.lbm_read_probes(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_probes" in lib.lbm_last_error()


GOOD = [(1, 2), (3, 4)]


@pytest.mark.parametrize("cells,every,capacity,match", [
    (GOOD, 1.5, 4, "every must be an integer"), (GOOD, True, 4, "every must be an integer"),
    (GOOD, "1", 4, "every must be an integer"), (GOOD, -1, 4, r"every must lie in \[0, 2\^31\)"),
    (GOOD, 2 ** 31, 4, r"every must lie in \[0, 2\^31\)"),
    (GOOD, 1, 2.0, "capacity must be an integer"), (GOOD, 1, False, "capacity must be an integer"),
    (GOOD, 1, None, "capacity must be an integer"), (GOOD, 1, -3, r"capacity must lie in \[0, 2\^31\)"),
    (GOOD, 1, 2 ** 31, r"capacity must lie in \[0, 2\^31\)"),
    (GOOD, 1, 0, "capacity 0, at least one row of samples is needed"),
    ([(0, 0)] * 257, 1, 4, "257 probes, at most LBM_MAX_PROBES = 256"),
    ([(1, 2), 3], 1, 4, "cell 1 must be a pair of integers"), ([(1, 2, 3)], 1, 4, "cell 0 must be a pair of integers"),
    ([(1.0, 2)], 1, 4, "cell 0 must be a pair of integers"), ([(1, True)], 1, 4, "cell 0 must be a pair of integers"),
    ([(1, "2")], 1, 4, "cell 0 must be a pair of integers"), ([(1, 2 ** 31)], 1, 4, "cell 0 must be a pair of integers"),
    (5, 1, 4, "cells must be a sequence")])
def test_python_argument_checks_need_no_device(lbm, cells, every, capacity, match):
    with pytest.raises(lbm.LbmError, match=match):
        lbm._probe_args(cells, every, capacity)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._probe_args(GOOD, 1, 4) == ([(1, 2), (3, 4)], 1, 4)
    assert lbm._probe_args(np.array([[5, 6], [5, 6]]), np.int64(7), np.int32(9)) == ([(5, 6), (5, 6)], 7, 9)
    assert lbm._probe_args([(0, 0)] * 256, 2 ** 31 - 1, 1)[1:] == (2 ** 31 - 1, 1)
    assert lbm._probe_args([], 0, 0) == ([], 0, 0)            # disarming needs no capacity
    assert lbm._probe_args(GOOD, 0, 0) == (GOOD, 0, 0)
    out = lbm._probe_args(iter(GOOD), 1, 1)
    assert all(type(v) is int for cell in out[0] for v in cell) and type(out[1]) is int and type(out[2]) is int


def test_engine_signatures(lbm):
    sig = inspect.signature(lbm.Engine.set_probes)
    assert list(sig.parameters) == ["self", "cells", "every", "capacity"]
    assert sig.parameters["every"].default == 1
    assert isinstance(sig.parameters["capacity"].default, int) and sig.parameters["capacity"].default >= 1
    sig = inspect.signature(lbm.Engine.probes)
    assert list(sig.parameters) == ["self", "max_samples"] and sig.parameters["max_samples"].default is None
    assert lbm.BatchMember.set_probes is lbm.Engine.set_probes and lbm.BatchMember.probes is lbm.Engine.probes


def test_write_probes_matches_the_format(lbm, tmp_path):
    cells = [(64, 64), (10, 126)]
    samples = np.array([[[1.5e-3, -2.5e-4, np.float32(1e-40), 1.0 / 3.0], [0.0, -0.0, 0.0, 0.1 / 3.0]],
                        [[np.float32(3.4e38), 0.123456789, 1.0, 2.0], [1.0, 2.0, 3.0, 4.0]]], dtype=np.float32)
    path = tmp_path / "probes.dat"
    lbm.write_probes(str(path), cells, [0, 7], samples)
    want = ("0 64 64 1.500000013039E-03 -2.500000118744E-04 9.999946101115E-41 3.333333432674E-01\n"
            "0 10 126 0.000000000000E+00 -0.000000000000E+00 0.000000000000E+00 3.333333507180E-02\n"
            "7 64 64 3.399999952144E+38 1.234567910433E-01 1.000000000000E+00 2.000000000000E+00\n"
            "7 10 126 1.000000000000E+00 2.000000000000E+00 3.000000000000E+00 4.000000000000E+00\n")
    assert path.read_text() == want
    with pytest.raises(lbm.LbmError, match="write_probes"):
        lbm.write_probes(str(path), cells, [0], samples)


@pytest.mark.parametrize("value", [""] + MALFORMED["LBM_PROBES"])
def test_cli_dies_on_a_malformed_lbm_probes(lbm, tmp_path, value):
    """As for a malformed LBM_STEADY: a message and exit(EXIT_FAILURE), before any device is touched.  (An empty value
    counts as unset, so the run goes on to its usual end: on a box without a device that is lbm_create's error.)"""
    out = run_cli(lbm, tmp_path, LBM_PROBES=value)
    if value == "":
        assert "LBM_PROBES" not in out.stderr
        return
    assert out.returncode == 1
    assert "could not read LBM_PROBES" in out.stderr
    assert not (tmp_path / "av_vels.dat").exists()
    assert not (tmp_path / "probes.dat").exists()
