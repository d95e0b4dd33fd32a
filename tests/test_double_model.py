"""Pins tests/double_model.py -- the float64 reading of the reference's timestep that the double engine is compared with
bit for bit -- to the reference's own golden results (check/*.dat, kept as tests/golden/check_goldens.npz): they are the
reference algorithm evaluated in IEEE double with the run constants parsed as doubles.

The bound: the goldens are printed with %.12E, 13 significant digits, so a printed value is within 5e-13 relative (the
half-ulp of the print) of the value computed.  1e-12 is twice that; the pairwise instead of sequential sum of
av_velocity contributes about 1e-15.  The same run with the three constants first rounded to float, as the fp32
engine's interface carries them, sits near 6e-8 over these 500 steps (1.7e-7 over the full run) and must miss the bound: the test can tell the two apart."""
import os

import numpy as np
import pytest

import double_model
from conftest import GOLDEN

STEPS = 500
BOUND = 1e-12


def _run(lbm, round_to_float):
    p = lbm.read_params_double(os.path.join(GOLDEN, "inputs", "input_128x128.params"))
    ob = lbm.read_obstacles(os.path.join(GOLDEN, "inputs", "obstacles_128x128.dat"), p.nx, p.ny)
    density, accel, omega = p.density, p.accel, p.omega
    if round_to_float:
        density, accel, omega = (float(np.float32(v)) for v in (density, accel, omega))
    cells = double_model.init_cells(p.nx, p.ny, density)
    av = double_model.run(cells, ob, density, accel, omega, STEPS)
    gold = np.load(os.path.join(GOLDEN, "check_goldens.npz"))["av_vels_128x128"][:STEPS]
    return float(np.max(np.abs(av - gold) / np.abs(gold)))


def test_model_reproduces_the_goldens_to_their_printed_digits(lbm):
    worst = _run(lbm, round_to_float=False)
    print(f"128x128, first {STEPS} av_vels against the goldens: max relative difference {worst:.3e}")
    assert worst <= BOUND


def test_float_rounded_constants_miss_the_bound(lbm):
    worst = _run(lbm, round_to_float=True)
    print(f"the same with density, accel, omega rounded to float: {worst:.3e}")
    assert worst > BOUND
    assert worst < 1e-5   # ... and they are the same flow: a float's rounding of the constants, not another run
