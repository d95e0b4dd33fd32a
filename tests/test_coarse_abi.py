"""CPU checks of the coarse frames (lbm_read_coarse, lbm_set_coarse_frames, lbm_read_coarse_frames and the batch twins):
exported and declared, the argument checks that need no device, the text writer, the geometry and "words -> frame"
(csrc/lbm_coarse_row.h, as a stand-alone program), and the numpy model the GPU tests compare against, checked on the
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

import coarse_model
import profile_model
from conftest import ROOT

NAMES = ("lbm_read_coarse", "lbm_set_coarse_frames", "lbm_read_coarse_frames", "lbm_batch_set_coarse_frames", "lbm_batch_read_coarse_frames")


def test_coarse_symbols_are_exported_declared_and_listed(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS and name not in lbm.ABI_SYMBOLS_NUMBERED
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert re.fullmatch(r"lbm_[a-z_]+", name)
    assert re.search(r"int lbm_read_coarse\(lbm_ctx\* ctx, int bx, int by, lbm_profile_line\* out[^,]*\);", header)
    assert re.search(r"int lbm_set_coarse_frames\(lbm_ctx\* ctx, int every, int capacity, int bx, int by\);", header)
    assert re.search(r"int lbm_read_coarse_frames\(lbm_ctx\* ctx, int max_frames, lbm_profile_line\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_batch_set_coarse_frames\(lbm_batch\* batch, int every, int capacity, int bx, int by\);", header)
    assert re.search(r"int lbm_batch_read_coarse_frames\(lbm_batch\* batch, int max_frames, lbm_profile_line\* out[^,]*, int\* steps, int\* n_read\);",
                     header)
    assert re.search(r"#define LBM_COARSE_MAX_BOX\s+256\b", header) and lbm.COARSE_MAX_BOX == 256
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout


def test_null_handles_are_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    line = np.zeros(1, dtype=lbm.PROFILE_DTYPE)
    assert lib.lbm_read_coarse(None, 1, 1, line.ctypes.data) != 0
    assert b"lbm_read_coarse" in lib.lbm_last_error()
    assert lib.lbm_set_coarse_frames(None, 10, 4, 16, 16) != 0
    assert b"lbm_set_coarse_frames" in lib.lbm_last_error()
    assert lib.lbm_read_coarse_frames(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_coarse_frames" in lib.lbm_last_error()
    assert lib.lbm_batch_set_coarse_frames(None, 10, 4, 16, 16) != 0
    assert b"lbm_batch_set_coarse_frames" in lib.lbm_last_error()
    assert lib.lbm_batch_read_coarse_frames(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_batch_read_coarse_frames" in lib.lbm_last_error()


@pytest.mark.parametrize("every,capacity,box,match", [
    (1.5, 4, 16, "every must be an integer"), (True, 4, 16, "every must be an integer"), (None, 4, 16, "every must be an integer"),
    (10, 2.0, 16, "capacity must be an integer"), (10, None, 16, "capacity must be an integer"), (10, False, 16, "capacity must be an integer"),
    (-1, 4, 16, r"every must lie in \[0, 2\^31\)"), (2 ** 31, 4, 16, r"every must lie in \[0, 2\^31\)"),
    (10, -3, 16, r"capacity must lie in \[0, 2\^31\)"), (10, 2 ** 31, 16, r"capacity must lie in \[0, 2\^31\)"),
    (10, 0, 16, "at least one frame"),
    (10, 4, True, "box must be a pair"), (10, 4, 16.0, "box must be a pair"), (10, 4, None, "box must be a pair"), (10, 4, "16", "box must be a pair"),
    (10, 4, (16,), "box must be a pair.*1 values"), (10, 4, (16, 16, 16), "box must be a pair.*3 values"), (10, 4, (), "box must be a pair"),
    (10, 4, (16, 2.0), "box must be a pair"), (10, 4, (True, 16), "box must be a pair"), (10, 4, (None, 16), "box must be a pair"),
    (10, 4, 0, r"box side bx must lie in \[1, 256\] \(got 0\)"), (10, 4, (16, 0), r"box side by must lie in \[1, 256\] \(got 0\)"),
    (10, 4, (-4, 16), r"box side bx must lie in \[1, 256\] \(got -4\)"), (10, 4, (16, 257), r"box side by must lie in \[1, 256\] \(got 257\)"),
    (10, 4, 2 ** 31, r"box side bx must lie in \[1, 256\]")])
def test_python_argument_checks_need_no_device(lbm, every, capacity, box, match):
    with pytest.raises(lbm.LbmError, match="set_coarse_frames: .*" + match):
        lbm._coarse_args(every, capacity, box)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._coarse_args(0, 0, 16) == (0, 0, 16, 16)
    assert lbm._coarse_args(3, 2 ** 31 - 1, (1, 256)) == (3, 2 ** 31 - 1, 1, 256)
    assert lbm._coarse_args(3, 1, [33, 5]) == (3, 1, 33, 5)
    assert lbm._coarse_args(3, 1, np.array([4, 2])) == (3, 1, 4, 2)
    got = lbm._coarse_args(np.int64(7), np.int32(2), (np.int16(2), np.int64(3)))
    assert got == (7, 2, 2, 3) and all(type(v) is int for v in got)
    assert lbm._coarse_shape(130, 7, 33, 3) == (3, 4) and lbm._coarse_shape(128, 128, 16, 16) == (8, 8)


def test_method_signatures(lbm):
    for cls in (lbm.Engine, lbm.Batch):
        sig = inspect.signature(cls.set_coarse_frames)
        assert list(sig.parameters) == ["self", "every", "capacity", "box"]
        assert sig.parameters["capacity"].default == 16 and sig.parameters["box"].default == (16, 16)
        assert list(inspect.signature(cls.coarse_frames).parameters) == ["self", "max_frames"]
        assert inspect.signature(cls.coarse_frames).parameters["max_frames"].default is None
    assert list(inspect.signature(lbm.Engine.coarse).parameters) == ["self", "box"]
    assert lbm.BatchMember.set_coarse_frames is lbm.Engine.set_coarse_frames      # a member raises the engine's refusal
    assert lbm.BatchMember.coarse is lbm.Engine.coarse
    assert list(inspect.signature(lbm.write_coarse_state).parameters) == ["path", "frame"]
    assert "coarse frame" in lbm.profile_means.__doc__


def test_write_coarse_state_format(lbm, tmp_path):
    path = str(tmp_path / "coarse.dat")
    frame = np.zeros((2, 2), dtype=lbm.PROFILE_DTYPE)
    frame[0, 0] = (12.0, 3.0, -1.0, 0.75, -1.0, 4, 1)
    frame[0, 1] = (0.0, 0.0, 0.0, 0.0, 0.0, 0, 3)          # no finite fluid cell: an obstacle in the picture
    frame[1, 0] = (3.0, 0.0, 0.0, 0.0, 0.0, 2, 0)
    frame[1, 1] = (1.5, 0.0, 0.0, 0.375, 0.5, 1, 0)
    lbm.write_coarse_state(path, frame)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    want = [(0, 0, 0.1875, -0.25, f32(math.sqrt(0.1875 ** 2 + 0.25 ** 2)), f32(3.0 * (1.0 / 3.0)), 0), (1, 0, 0.0, 0.0, 0.0, 0.0, 1),
            (0, 1, 0.0, 0.0, 0.0, f32(1.5 * (1.0 / 3.0)), 0), (1, 1, 0.375, 0.5, 0.625, f32(1.5 * (1.0 / 3.0)), 0)]
    assert open(path).read() == "".join("%d %d %.12E %.12E %.12E %.12E %d\n" % w for w in want)
    for bad in (np.zeros(4, dtype=lbm.PROFILE_DTYPE), np.zeros((2, 2))):
        with pytest.raises(lbm.LbmError, match="frame must be one frame"):
            lbm.write_coarse_state(path, bad)


# ---- geometry and words -> frame ------------------------------------------------------------------------------------------
def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def slab_geometry(ny, by, first, count):
    """(box rows that touch the slab's rows [first, first + count), the whole ones, the partial ones), by the definition"""
    touch = [Y for Y in range(-(-ny // by)) if Y * by < first + count and min(ny, (Y + 1) * by) > first]
    whole = [Y for Y in touch if Y * by >= first and min(ny, (Y + 1) * by) <= first + count]
    return touch, whole, [Y for Y in touch if Y not in whole]


# (nx, ny, bx, by, [(row_first, row_count)]): 1, 2, 3 and 8 slabs with uneven row ranges; by of 1, a divisor of a slab's
# rows, straddling two slabs, taller than a slab (a middle slab's only box row is both its first and its last), the
# whole grid; a ragged last box in x and in y
GEOMETRIES = [(5, 4, 2, 1, [(0, 4)]), (7, 9, 3, 4, [(0, 9)]), (6, 10, 6, 5, [(0, 5), (5, 5)]), (6, 10, 4, 4, [(0, 5), (5, 5)]),
              (5, 16, 2, 1, [(0, 6), (6, 5), (11, 5)]), (5, 16, 5, 4, [(0, 6), (6, 5), (11, 5)]), (5, 16, 2, 5, [(0, 6), (6, 5), (11, 5)]),
              (5, 16, 1, 16, [(0, 6), (6, 5), (11, 5)]), (4, 16, 3, 12, [(0, 6), (6, 5), (11, 5)]), (4, 17, 2, 7, [(0, 3), (3, 2), (5, 12)]),
              (3, 16, 2, 3, [(2 * s, 2) for s in range(8)]), (3, 16, 3, 2, [(2 * s, 2) for s in range(8)]),
              (3, 19, 1, 8, [(0, 3), (3, 2), (5, 2), (7, 3), (10, 2), (12, 2), (14, 3), (17, 2)])]


def coarse_cases():
    """[(nx, ny, bx, by, ranges, {(slab, X, Y): ([5 term vectors], fluid, nonfinite)})]: random terms for every box of every
    slab's share; what a frame must be follows from all terms"""
    rng = np.random.default_rng(12)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    pops = lambda n: f32(0.1 * (1 + 0.05 * rng.standard_normal(n)))  # noqa: E731
    wide = lambda n: f32(np.ldexp(rng.standard_normal(n), rng.integers(-140, 120, n)))  # noqa: E731
    carry = lambda n: f32(np.full(n, np.float32(4.0) - np.float32(2.0 ** -22)))   # noqa: E731  24 one-bits across two limbs: their sum carries
    empty = f32([])

    def box(n, kind):
        if kind == "zero":
            return [empty] * 5, 0, int(n)
        if kind == "carry":
            return [carry(300), -carry(300), carry(7), -carry(1), carry(2)], int(n), 0
        return [pops(n), f32(1e-3 * rng.standard_normal(n)), wide(n), -np.abs(wide(n)), f32(rng.standard_normal(n))], int(n), int(rng.integers(0, 3))

    cases = []
    for nx, ny, bx, by, ranges in GEOMETRIES:
        cx = -(-nx // bx)
        share = {}
        for s, (first, count) in enumerate(ranges):
            for Y in slab_geometry(ny, by, first, count)[0]:
                rows = min(ny, (Y + 1) * by, first + count) - max(Y * by, first)
                for X in range(cx):
                    kind = "zero" if (X, Y) == (1, 0) else "carry" if (X, Y) == (0, 1) else "any"
                    share[(s, X, Y)] = box(rows * (min(nx, (X + 1) * bx) - X * bx), kind)
        cases.append((nx, ny, bx, by, ranges, share))
    return cases


def case_text(nx, ny, bx, by, ranges, share):
    out = ["%d %d %d %d %d" % (len(ranges), nx, ny, bx, by)]
    cx = -(-nx // bx)
    for s, (first, count) in enumerate(ranges):
        out.append("%d %d" % (first, count))
        _, whole, partial = slab_geometry(ny, by, first, count)
        for Y in whole + partial:
            for X in range(cx):
                terms, fluid, bad = share[(s, X, Y)]
                for t in terms:
                    out.append(" ".join(["%d" % len(t)] + ["%x" % b for b in np.asarray(t, dtype=np.float32).view(np.uint32).tolist()]))
                out.append("%d %d" % (fluid, bad))
    return "\n".join(out) + "\n"


def case_expected(i, nx, ny, bx, by, ranges, share):
    out = ["case %d" % i]
    cx, cy = -(-nx // bx), -(-ny // by)
    for s, (first, count) in enumerate(ranges):
        touch, whole, partial = slab_geometry(ny, by, first, count)
        assert len(partial) <= 2 and all(Y in (touch[0], touch[-1]) for Y in partial)
        whole_first = touch[0] + (1 if touch[0] in partial else 0)      # where the whole box rows would start, also when there is none
        assert not whole or whole == list(range(whole_first, whole_first + len(whole)))
        out.append("slab %d %d %d %d %d %d %d %d" % (s, touch[0], len(touch), whole_first, len(whole), partial[0] if partial else -1,
                                                     partial[1] if len(partial) > 1 else -1, cx * (6 * len(whole) + 48 * len(partial))))
    for Y in range(cy):
        for X in range(cx):
            parts = [v for (s, x, y), v in sorted(share.items()) if (x, y) == (X, Y)]
            assert parts
            sums = [math.fsum(float(v) for p in parts for v in p[0][j]) for j in range(5)]
            out.append(" ".join("%016x" % dbits(v) for v in sums) + " %d %d" % (sum(p[1] for p in parts), sum(p[2] for p in parts)))
    return "\n".join(out) + "\n"


def test_geometry_and_words_to_frame(tmp_path):
    """lbm_coarse_row.h, built as a stand-alone program under AddressSanitizer and UBSan (as profile_row_check is): the
    slabs' whole and partial box rows, the slot's words and offsets (every box inside the slot, no word shared, none left
    over), and the frame against math.fsum over all terms: negative sums, a carry across limbs, an all-zero box"""
    exe = str(tmp_path / "coarse_row_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "coarse_row_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    cases = coarse_cases()
    # what the cases cover: by taller than a slab (a slab whose one box row is partial), a box row over three slabs, 8 slabs
    assert any(len(r) == 8 for _, _, _, _, r in GEOMETRIES)
    assert any(slab_geometry(ny, by, f, c)[1:] == ([], [f // by]) for _, ny, _, by, r in GEOMETRIES for f, c in r[1:-1])
    assert any(len(slab_geometry(ny, by, f, c)[2]) == 2 for _, ny, _, by, r in GEOMETRIES for f, c in r)
    assert any(nx % bx for nx, _, bx, _, _ in GEOMETRIES) and any(ny % by for _, ny, _, by, _ in GEOMETRIES)
    text = "".join(case_text(*c) for c in cases)
    want = "".join(case_expected(i, *c) for i, c in enumerate(cases))
    zero = " ".join(["%016x" % 0] * 5)
    assert any(line.startswith(zero + " 0 ") for line in want.splitlines())                         # the all-zero box: +0.0 five times
    assert any(line.split()[1][0] in "89abcdef" for line in want.splitlines() if len(line) > 80)    # a negative sum
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, f"coarse_row_check: exit status {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert run.stdout == want


# ---- the model, on the oracle alone ---------------------------------------------------------------------------------------
def flat(frame):
    return [b for row in frame for b in row]


def test_model_ties_to_the_line_profiles_and_counts(lbm, oracle):
    p = lbm.Params(16, 8, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((8, 16), dtype=np.int32)
    ob[3:5, 6:8] = 1
    ob[6:8, 8:12] = 1                            # the box (2, 3) of 4 x 2 boxes, fully blocked
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 5)
    cells[0, 0, 1] = np.inf                      # fluid
    cells[3, 6, 4] = np.nan                      # blocked: counted nowhere
    rec = profile_model.record(cells, ob)
    rows = coarse_model.frame(cells, ob, (16, 1))
    assert [len(r) for r in rows] == [1] * 8 and flat(rows) == rec["rows"]             # (nx, 1): the row lines
    columns = coarse_model.frame(cells, ob, (1, 8))
    assert len(columns) == 1 and columns[0] == rec["columns"]                          # (1, ny): the column lines
    fluid_cells = int((ob == 0).sum())
    for box in ((4, 2), (5, 3), (1, 1), (16, 8), (3, 8)):
        frame = coarse_model.frame(cells, ob, box)
        assert (len(frame), len(frame[0])) == coarse_model.shape(16, 8, box)
        assert sum(b["fluid"] + b["nonfinite"] for b in flat(frame)) == fluid_cells
        assert sum(b["nonfinite"] for b in flat(frame)) == 1 and frame[0][0]["nonfinite"] == 1
        for b in flat(frame):
            assert all(math.isfinite(b[k]) and not (b[k] == 0.0 and math.copysign(1.0, b[k]) < 0) for k in coarse_model.SUMS)
    frame = coarse_model.frame(cells, ob, (4, 2))
    assert frame[3][2] == dict(sum_rho=0.0, sum_jx=0.0, sum_jy=0.0, sum_ux=0.0, sum_uy=0.0, fluid=0, nonfinite=0)
    assert frame[1][1]["fluid"] == 6 and frame[2][1]["fluid"] == 6 and frame[1][0]["fluid"] == 8
    ragged = coarse_model.frame(cells, ob, (5, 3))
    assert ragged[2][3]["fluid"] == 1 * 2 and ragged[0][3]["fluid"] == 1 * 3           # the last boxes: 1 cell wide, 2 rows tall


def test_model_same_bits_reports_shape_and_value(lbm, oracle):
    p = lbm.Params(8, 4, 100, 10, 0.1, 0.005, 1.85)
    ob = np.zeros((4, 8), dtype=np.int32)
    cells = oracle.init_cells(p)
    oracle.run(p, cells, ob, 2)
    frame = coarse_model.frame(cells, ob, (4, 2))
    got = np.zeros((2, 2), dtype=lbm.PROFILE_DTYPE)
    for Y in range(2):
        for X in range(2):
            got[Y, X] = tuple(frame[Y][X][k] for k in coarse_model.FIELDS)
    assert not coarse_model.same_bits(got, frame)
    got[1, 0]["sum_jx"] = np.nextafter(got[1, 0]["sum_jx"], 1.0)
    assert [d[:3] for d in coarse_model.same_bits(got, frame)] == [(1, 0, "sum_jx")]
    assert coarse_model.same_bits(got[:1], frame)[0][0] == "shape"
