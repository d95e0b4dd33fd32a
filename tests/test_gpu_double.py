"""The double-precision engine (lbm_double_*, DoubleEngine) on the GPU.

1. bit for bit against tests/double_model.py (the float64 reading of the reference's timestep) at the smallest shapes
   at which the kernels can go wrong;
2. a run issued in pieces equals the run issued at once;
3. the reference's own pin: full runs against the double-precision goldens of check/ (tests/golden/check_goldens.npz),
   to the digits they are printed with;
4. the command line, LBM_PRECISION=double;
5. an fp32 Engine and a DoubleEngine side by side;
6. in tests/test_gpu_double_edges.py, on the inputs of tests/double_edge_lattice.py: the refused lid acceleration in
   every kernel that accelerates, cells far from equilibrium (denormals, 2^1000, negative and zero density, Inf, NaN, a
   cell of -0.0), more than 256 workgroups and 65 536 cells, the ring of partials across calls, lattices staged in chunks.

Bounds.  Lattice, u_x, u_y, pressure and u (IEEE sqrt) are compared as bit patterns.  av_vels[t] is a sum of n = fluid
cells non-negative terms that the kernels add in another order than the model (or the reference): two orders of such a
sum differ by at most 2 (n - 1) 2^-53 relative.  The goldens are printed with %.12E, so a printed value is within
5e-13 relative of the value computed: av_vels must meet 5e-13 + 2 (n - 1) 2^-53, the pressure field (no sum) 1e-12."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import double_model
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DENSITY, ACCEL, OMEGA = 0.1, 0.005, 1.85
STEPS = 40


def sum_order_bound(n_fluid):
    return 2.0 * (n_fluid - 1) * 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_cases = {}


def case(nx, ny):
    """A random positive lattice, random obstacles with blocked cells on the lid row, and the model's results after
    STEPS timesteps; computed once per shape and never changed."""
    if (nx, ny) not in _cases:
        rng = np.random.default_rng(1000 * nx + ny)
        ob = (rng.random((ny, nx)) < 0.15).astype(np.int32)
        lid = ny - 2
        ob[lid, :] = 0
        ob[lid, rng.choice(nx, size=max(1, nx // 8), replace=False)] = 1   # blocked cells on the lid row ...
        ob[lid, 0] = 0                                                      # ... and fluid ones, the row ends among them
        ob[lid, nx - 1] = 1
        start = double_model.init_cells(nx, ny, DENSITY) * (0.5 + rng.random((ny, nx, 9)))
        cells = start.copy()
        av = double_model.run(cells, ob, DENSITY, ACCEL, OMEGA, STEPS)
        assert np.isfinite(cells).all() and (av > 0).all()
        want = {"start": start, "ob": ob, "cells": cells, "av": av, "final": double_model.final_state(cells, ob, DENSITY)}
        for v in (start, ob, cells, av, *want["final"].values()):
            v.setflags(write=False)
        _cases[(nx, ny)] = want
    return _cases[(nx, ny)]


# 130x6: the wave edge at cell 128 and a ragged last wave; 516x5, 512x4: the workgroup edge at cell 512 and a row count
# that does not fill a workgroup; 8x3: the smallest grid, lid row 1, both wraps; 7x5, 129x4: odd nx, the one-cell kernel
@pytest.mark.parametrize("nts", [0, 1])
@pytest.mark.parametrize("nx,ny", [(130, 6), (516, 5), (512, 4), (8, 3), (7, 5), (129, 4)])
def test_bit_identical_to_the_model(lbm, monkeypatch, nx, ny, nts):
    want = case(nx, ny)
    monkeypatch.setenv("LBM_DOUBLE_NTS", str(nts))
    p = lbm.ParamsDouble(nx, ny, STEPS, 10, DENSITY, ACCEL, OMEGA)
    with lbm.DoubleEngine(p, want["ob"], want["start"]) as eng:
        info = eng.info()
        assert info["lane_cells"] == (2 if nx % 2 == 0 else 1)
        assert info["nontemporal"] == (nts if nx % 2 == 0 else 0)
        assert info["fluid_cells"] == int((want["ob"] == 0).sum())
        assert np.array_equal(bits(eng.cells()), bits(want["start"]))        # aos_to_soa / soa_to_aos round trip
        eng.run(STEPS)
        assert eng.info()["steps_done"] == STEPS
        got, av, final = eng.cells(), eng.av_vels(), eng.final_state()
        av_now, mass, reynolds = eng.av_velocity(), eng.total_density(), eng.reynolds()
    assert np.array_equal(bits(got), bits(want["cells"])), "lattice differs from the float64 model"
    for name in ("u_x", "u_y", "pressure", "u"):
        assert np.array_equal(bits(final[name]), bits(want["final"][name])), name
    n = info["fluid_cells"]
    rel = np.abs(av - want["av"]) / want["av"]
    print(f"{nx}x{ny} nts={nts}: av_vels max relative difference {rel.max():.3e} (bound {sum_order_bound(n):.3e})")
    assert rel.max() <= sum_order_bound(n)
    assert abs(av_now - want["av"][-1]) / want["av"][-1] <= sum_order_bound(n)
    total = float(want["cells"].sum())
    assert abs(mass - total) / total <= sum_order_bound(9 * nx * ny)
    viscosity = 1.0 / 6.0 * (2.0 / OMEGA - 1.0)
    assert reynolds == av_now * 10 / viscosity


def test_run_in_pieces_equals_one_run(lbm):
    """run(3); run(4) against run(7): the first step's accelerate_row pass, the lid row left unaccelerated by a call's
    last step, and the parity of the two lattices."""
    want = case(130, 6)
    p = lbm.ParamsDouble(130, 6, 7, 10, DENSITY, ACCEL, OMEGA)
    with lbm.DoubleEngine(p, want["ob"], want["start"]) as a, lbm.DoubleEngine(p, want["ob"], want["start"]) as b:
        a.run(3)
        a.run(4)
        b.run(7)
        whole = b.cells()
        assert np.array_equal(bits(a.cells()), bits(whole))
        assert np.array_equal(bits(a.av_vels()), bits(b.av_vels()))
        with pytest.raises(lbm.LbmError, match="av_vels record holds 7"):
            a.run(1)
    cells = want["start"].copy()
    double_model.run(cells, want["ob"], DENSITY, ACCEL, OMEGA, 7)
    assert np.array_equal(bits(whole), bits(cells))


def test_equilibrium_start_equals_the_model(lbm):
    want = case(130, 6)
    p = lbm.ParamsDouble(130, 6, 1, 10, DENSITY, ACCEL, OMEGA)
    with lbm.DoubleEngine(p, want["ob"]) as eng:
        assert np.array_equal(bits(eng.cells()), bits(double_model.init_cells(130, 6, DENSITY)))


def golden_run(lbm, name, steps):
    p = lbm.read_params_double(os.path.join(GOLDEN, "inputs", f"input_{name}.params"))
    ob = lbm.read_obstacles(os.path.join(GOLDEN, "inputs", f"obstacles_{name}.dat"), p.nx, p.ny)
    gold = np.load(os.path.join(GOLDEN, "check_goldens.npz"))
    with lbm.DoubleEngine(p, ob) as eng:
        eng.run(steps)
        av, final, n = eng.av_vels(), eng.final_state(), eng.info()["fluid_cells"]
    want = gold[f"av_vels_{name}"][:steps]
    rel = float(np.max(np.abs(av - want) / np.abs(want)))
    bound = 5e-13 + sum_order_bound(n)
    print(f"{name}, {steps} steps: av_vels max relative difference to the goldens {rel:.3e} (bound {bound:.3e})")
    return rel, bound, final, gold, p


@pytest.mark.parametrize("name", ["128x128", "128x256"])
def test_full_runs_meet_the_goldens_to_their_printed_digits(lbm, name):
    rel, bound, final, gold, p = golden_run(lbm, name, 40000)
    assert p.max_iters == 40000
    assert rel <= bound
    want = gold[f"pressure_{name}"]
    prel = float(np.max(np.abs(final["pressure"].ravel() - want) / np.abs(want)))
    print(f"{name}: pressure max relative difference to the goldens {prel:.3e} (bound 1e-12)")
    assert prel <= 1e-12


def test_first_2000_steps_of_256x256_meet_the_goldens(lbm):
    rel, bound, _, _, _ = golden_run(lbm, "256x256", 2000)
    assert rel <= bound


def test_command_line_in_double_and_unchanged_without(lbm, tmp_path):
    pf = os.path.join(GOLDEN, "inputs", "input_128x128.params")
    of = os.path.join(GOLDEN, "inputs", "obstacles_128x128.dat")
    env = {k: v for k, v in os.environ.items() if k != "LBM_PRECISION"}
    dirs = {}
    for label, extra in (("double", {"LBM_PRECISION": "double"}), ("single", {})):
        d = tmp_path / label
        d.mkdir()
        out = subprocess.run([lbm.CLI_PATH, pf, of], cwd=d, capture_output=True, text=True, env=dict(env, **extra), timeout=120)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[0] == "==done==" and lines[1].startswith("Reynolds number:\t\t")
        dirs[label] = d
    gold = np.load(os.path.join(GOLDEN, "check_goldens.npz"))
    ob = lbm.read_obstacles(of, 128, 128)
    n = int((ob == 0).sum())
    # the files hold printed values, as the goldens do: the same bounds (a last printed digit that falls the other way
    # is 1e-13 .. 1e-12 relative, 3e-13 at the pressure's 3.3E-02)
    av = np.loadtxt(dirs["double"] / "av_vels.dat", usecols=[1])
    want = gold["av_vels_128x128"]
    assert av.size == want.size
    rel = float(np.max(np.abs(av - want) / np.abs(want)))
    print(f"LBM_PRECISION=double: av_vels.dat max relative difference to the goldens {rel:.3e}")
    assert rel <= 5e-13 + sum_order_bound(n)
    fs = np.loadtxt(dirs["double"] / "final_state.dat")
    assert fs.shape == (128 * 128, 7) and np.array_equal(fs[:, 6].astype(np.int32), ob.ravel())
    prel = float(np.max(np.abs(fs[:, 5] - gold["pressure_128x128"]) / gold["pressure_128x128"]))
    print(f"LBM_PRECISION=double: final_state.dat pressure max relative difference {prel:.3e}")
    assert prel <= 1e-12
    # without the variable: the very bytes SerialCode writes
    known = str(np.load(os.path.join(GOLDEN, "serialcode_128x128.npz"))["md5_final_state"])
    assert known.startswith("b72c5803")
    assert hashlib.md5((dirs["single"] / "final_state.dat").read_bytes()).hexdigest() == known
    bad = subprocess.run([lbm.CLI_PATH, pf, of], cwd=tmp_path, capture_output=True, text=True,
                         env=dict(env, LBM_PRECISION="double", LBM_GPUS="2"), timeout=120)
    assert bad.returncode == 1 and "not offered with LBM_PRECISION=double" in bad.stderr


def test_fp32_and_double_engines_side_by_side(lbm, oracle, datasets):
    p32, ob = datasets("128x128")
    p64 = lbm.read_params_double(os.path.join(GOLDEN, "inputs", "input_128x128.params"))
    ref = oracle.init_cells(p32)
    oracle.run(p32, ref, ob, 20)
    cells64 = double_model.init_cells(p64.nx, p64.ny, p64.density)
    double_model.run(cells64, ob, p64.density, p64.accel, p64.omega, 20)
    with lbm.Engine(p32, ob, oracle.init_cells(p32), n_gpus=1, math="exact") as e32, lbm.DoubleEngine(p64, ob) as e64:
        for _ in range(4):     # interleaved calls
            e32.run(5)
            e64.run(5)
        got32, got64 = e32.cells(), e64.cells()
    assert np.array_equal(ref.view(np.uint32), got32.view(np.uint32)), "the fp32 lattice differs from the oracle's"
    assert np.array_equal(bits(got64), bits(cells64)), "the double lattice differs from the model's"
