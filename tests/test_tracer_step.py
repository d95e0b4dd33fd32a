"""CPU check of the tracer step (csrc/lbm_tracer_step.h, the functions tracer_advance runs on the device) as a stand-alone
program under AddressSanitizer and UBSan, built with -ffp-contract=off like the library: nothing is loaded into Python.
The program checks tracer_wrap and tracer_cell over adversarial doubles itself (tests/tracer_step_check.cpp says how) and
advances the tracers of the cases on its standard input; those are compared here, bit for bit, with the numpy model
(tests/tracer_model.py), which is written from the definition in include/lbm_hip.h.  Host-only."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import makefile_rules
import tracer_model as tm

CSRC = os.path.join(ROOT, "lbm-asynchronous_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tracer_step") / "tracer_step_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "tracer_step_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, f"{' '.join(cmd)}\n{out.stdout}\n{out.stderr}"
    return exe


def run(program, text=""):
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, f"tracer_step_check: exit status {out.returncode}\n{out.stdout[-4000:]}\n{out.stderr[-4000:]}"
    return out.stdout.splitlines()


def test_wrap_and_cell_over_adversarial_doubles(program):
    lines = run(program)
    assert len(lines) == 1 and lines[0].endswith(" cases, 0 failed")
    assert int(lines[0].split()[0]) > 5 * 40000                        # five grid sizes, 20 000 random pairs each and the lists


def case_text(ux, uy, xy, h):
    ny, nx = ux.shape
    lines = ["%d %d %d %d" % (nx, ny, h, len(xy))]
    lines += ["%08x %08x" % (a, b) for a, b in zip(ux.view(np.uint32).ravel().tolist(), uy.view(np.uint32).ravel().tolist())]
    lines += ["%016x %016x" % (a, b) for a, b in np.ascontiguousarray(xy).view(np.uint64).tolist()]
    return "\n".join(lines) + "\n"


def positions(rng, nx, ny, n):
    """random positions, every cell centre (fx == 0 == fy), the last doubles below the far edges, the corner"""
    xy = rng.random((n, 2)) * (nx, ny)
    centres = np.stack(np.meshgrid(np.arange(nx), np.arange(ny)), axis=-1).reshape(-1, 2).astype(np.float64)
    edge = np.array([[np.nextafter(nx, 0), np.nextafter(ny, 0)], [0.0, 0.0], [nx - 2.0 ** -40, ny - 2.0 ** -40], [nx - 1.0, 0.5], [0.5, ny - 1.0]])
    return np.concatenate([xy, centres, edge])


@pytest.mark.parametrize("nx,ny", [(5, 3), (13, 5)])
def test_advance_on_random_fields_against_the_model(program, nx, ny):
    """random float fields with speeds up to 0.3 and spans up to 16: displacements of several cells, larger than the 5 x 3
    grid, so both wraps happen in both directions (asserted on the model); some cells are 0, 0 as blocked cells are"""
    rng = np.random.default_rng(nx * 100 + ny)
    text, want = "", []
    for h in (1, 3, 4, 16):
        ux = (0.3 * rng.standard_normal((ny, nx))).astype(np.float32)
        uy = (0.3 * rng.standard_normal((ny, nx))).astype(np.float32)
        ux[1, 2] = uy[1, 2] = ux[ny - 1, nx - 1] = uy[ny - 1, nx - 1] = 0.0
        xy = positions(rng, nx, ny, 200)
        text += case_text(ux, uy, xy, h)
        model, ends = tm.advance(ux, uy, xy, h, unwrapped=True)
        assert np.all(np.isfinite(model)) and np.all(model >= 0) and np.all(model[:, 0] < nx) and np.all(model[:, 1] < ny)
        if h >= 4:                                                    # wraps in both directions along both axes
            assert tm.crossed(ends, nx, ny) == (True, True, True, True)
        want.append(model)
    want = np.concatenate(want)
    lines = run(program, text)[1:]
    got = np.array([[int(w, 16) for w in line.split()] for line in lines], dtype=np.uint64).view(np.float64)
    assert got.shape == want.shape
    differ = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert differ.size == 0, (differ[:5], got[differ[:5]], want[differ[:5]])


def test_lost_tracers(program):
    """a NaN and an infinite velocity in a field: the tracers whose cells of either stage touch them are lost, (NaN, NaN);
    a lost tracer stays lost, no index is formed from it (the program runs under ASan and aborts on an index outside)"""
    rng = np.random.default_rng(7)
    nx, ny = 13, 5
    ux = (0.1 * rng.standard_normal((ny, nx))).astype(np.float32)
    uy = (0.1 * rng.standard_normal((ny, nx))).astype(np.float32)
    ux[2, 6] = np.nan
    uy[4, 0] = np.inf
    xy = np.concatenate([positions(rng, nx, ny, 100), [[np.nan, np.nan], [np.nan, 1.0], [2.0, np.inf], [-np.inf, np.nan]]])
    model = tm.advance(ux, uy, xy, 4)
    lost = np.isnan(model[:, 0])
    assert np.array_equal(lost, np.isnan(model[:, 1])) and 10 < lost.sum() < len(xy) - 10
    assert lost[-4:].all() and np.all(np.isfinite(model[~lost]))
    lines = run(program, case_text(ux, uy, xy, 4))[1:]
    got = np.array([[int(w, 16) for w in line.split()] for line in lines], dtype=np.uint64).view(np.float64)
    assert tm.same_bits(got, model)
    again = run(program, case_text(ux, uy, got, 4))[1:]
    got2 = np.array([[int(w, 16) for w in line.split()] for line in again], dtype=np.uint64).view(np.float64)
    assert np.all(np.isnan(got2[lost])) and tm.same_bits(got2, tm.advance(ux, uy, model, 4))


def test_model_wrap():
    """the model's own W by hand: identity inside, -ulp -> 0.0 (the rounding case the definition names), n -> 0"""
    z = np.array([0.0, 2.5, -0.25, 3.0, 7.25, -1e-300, np.inf, np.nan, -6.5])
    w = tm.wrap(z, 3)
    assert w[:6].tolist() == [0.0, 2.5, 2.75, 0.0, 1.25, 0.0] and np.isnan(w[6]) and np.isnan(w[7]) and w[8] == 2.5


def test_the_engine_has_the_step_nowhere_else():
    """the kernels call the header's tracer_advance; the Makefile rebuilds the library when the header changes"""
    src = open(os.path.join(CSRC, "lbm_kernels.hip.h")).read()
    assert '#include "lbm_tracer_step.h"' in src and "lbm_tracers::tracer_advance(" in src
    for target in ("liblbm_hip.so:", "asm:", "profile-lib:"):
        assert "csrc/lbm_tracer_step.h" in makefile_rules.rule_line(target), target
