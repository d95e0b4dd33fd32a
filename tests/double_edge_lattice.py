"""Inputs that take the double engine (lbm_double_*) where its own test lattices never go, and the float64 model's account
of them.  Inputs only, no GPU: tests/test_double_edge_lattice.py shows by the model alone that they reach what they aim
at, tests/test_gpu_double_edges.py compares the kernels with the model on them.

Refusal lattice.  The ramp of tests/edge_lattice.py read in float64: rows ny-4 .. ny-1 and row 0 of a random positive
lattice (weights x (1 +- 5 %)) are scaled per column, so that along the lid row ny-2 the ratios f3/a1, f6/a2, f7/a2 run
from well above 1 through 1 to well below and back; the noise makes the three sub-conditions of accelerate_flow
(SerialCode/d2q9-bgk.c:229-232) disagree near the crossings.  LID_SPECIALS are written onto the lid row before step 0.

Extreme lattice.  Each kind of EXTREME_KINDS is a 9-vector T that is to be the PRE-COLLISION cell of step 0: scattered
against the stream directions into the 3 x 3 neighbourhood (edge_lattice._scatter), in rows whose feeders are not on the
lid row, so step 0's acceleration leaves T alone.
"""
import numpy as np

import double_model
import edge_lattice as el

DENSITY, ACCEL, OMEGA = 0.1, 0.005, 1.85      # as tests/test_gpu_double.py
STEPS = 13
A1, A2 = el.accel_terms(DENSITY, ACCEL, np.float64)
A1, A2 = float(A1), float(A2)

# ---- refusal --------------------------------------------------------------------------------------------------------
# The ramp: s(x) = RAMP_LO * RAMP_SPAN^(|x mod 128 - 64| / 64), the threshold s = accel = 0.005 crossed twice per period.
# Span and seed are chosen so that the model's run meets the conditions of test_double_edge_lattice.py; they are inputs,
# nothing measured on a kernel enters them.
RAMP_LO, RAMP_SPAN = 0.00125, 16.0
REFUSAL_SEED = 3
REFUSAL_SHAPES = [(130, 12), (131, 12)]
SPECIALS_X0 = 68                              # sixteen columns from here, in the ramp's refusing stretch

_OK1, _OK2 = 4.0 * A1, 4.0 * A2               # comfortably positive after the subtraction
_UP = float(np.nextafter(A1, np.inf))
# name -> (populations 3, 6, 7, accepts, the one sub-condition that fails or None)
LID_SPECIALS = {
    "f3==a1": ((A1, _OK2, _OK2), False, 3),
    "f6==a2": ((_OK1, A2, _OK2), False, 6),
    "f7==a2": ((_OK1, _OK2, A2), False, 7),
    "f3==next(a1)": ((_UP, _OK2, _OK2), True, None),
    "f3 alone fails": ((0.5 * A1, _OK2, _OK2), False, 3),
    "f6 alone fails": ((_OK1, 0.5 * A2, _OK2), False, 6),
    "f7 alone fails": ((_OK1, _OK2, 0.5 * A2), False, 7),
    "f3<0": ((-_OK1, _OK2, _OK2), False, 3),
}


def place_lid_specials(cells, ob):
    """Every special at an even and at an odd column (the second eight are the first eight with neighbours swapped), the
    exact zero at x = 0 and its accepting neighbour at x = nx-1.  Returns [(x, name)]."""
    ny, nx = ob.shape
    lid = ny - 2
    names = list(LID_SPECIALS)
    swapped = [names[i ^ 1] for i in range(len(names))]
    where = [(SPECIALS_X0 + i, name) for i, name in enumerate(names + swapped)]
    where += [(0, "f3==a1"), (nx - 1, "f3==next(a1)")]
    for x, name in where:
        f3, f6, f7 = LID_SPECIALS[name][0]
        ob[lid, x] = 0
        cells[lid, x, 3], cells[lid, x, 6], cells[lid, x, 7] = f3, f6, f7
    return where


def build_refusal(nx, ny, seed=REFUSAL_SEED):
    """(ob, cells, specials)."""
    rng = np.random.default_rng(seed)
    ob = (rng.random((ny, nx)) < 0.05).astype(np.int32)
    lid = ny - 2
    ob[lid, :] = 0
    ob[lid, rng.choice(nx, size=nx // 16, replace=False)] = 1          # blocked cells on the lid row too
    cells = DENSITY * el.WEIGHTS * (0.95 + 0.1 * rng.random((ny, nx, 9)))
    el.apply_ramp(cells, RAMP_LO, RAMP_SPAN)
    specials = place_lid_specials(cells, ob)
    return ob, cells, specials


def lid_decisions(lid_cells, lid_ob):
    """What accelerate_flow decides on a lid row, in float64 as the model decides it: boolean rows `fluid`, `accept`, and
    `only` = {3, 6, 7} -> exactly that sub-condition fails."""
    c3, c6, c7 = el.verdicts(lid_cells, A1, A2)
    fluid = np.asarray(lid_ob) == 0
    return {"fluid": fluid, "accept": fluid & c3 & c6 & c7,
            "only": {3: fluid & ~c3 & c6 & c7, 6: fluid & c3 & ~c6 & c7, 7: fluid & c3 & c6 & ~c7}}


def decision_counts(d):
    return {"accept": int(d["accept"].sum()), "refuse": int((d["fluid"] & ~d["accept"]).sum()),
            **{f"only f{k}": int(v.sum()) for k, v in d["only"].items()}}


_runs = {}


def refusal_run(nx, ny):
    """The model's run of the refusal lattice, computed once per shape and never changed: start, ob, specials, the lid row
    before each step (`lids`), the lattice after each (`states`), av_vels and the per-step decision counts."""
    if ("refusal", nx, ny) not in _runs:
        ob, start, specials = build_refusal(nx, ny)
        cells, lids, states, av, counts = start.copy(), [], [], [], []
        for _ in range(STEPS):
            lids.append(cells[ny - 2].copy())
            counts.append(decision_counts(lid_decisions(cells[ny - 2], ob[ny - 2])))
            double_model.timestep(cells, ob, DENSITY, ACCEL, OMEGA)
            states.append(cells.copy())
            av.append(double_model.av_velocity(cells, ob))
        av = np.array(av)
        for a in (ob, start, av, *lids, *states):
            a.setflags(write=False)
        _runs[("refusal", nx, ny)] = dict(ob=ob, start=start, specials=specials, lids=lids, states=states, av=av, counts=counts)
    return _runs[("refusal", nx, ny)]


# ---- extreme cells --------------------------------------------------------------------------------------------------
def _tilted(scale):
    t = el.WEIGHTS * scale
    t[1] *= 1.5
    t[3] *= 0.5
    return t


EXTREME_KINDS = {
    "all denormal": _tilted(2.0 ** -1040),
    "numerators denormal": el._cell(f0=0.04, f1=1e-310, f5=3e-311),
    "huge": _tilted(2.0 ** 1000),
    "rho<0": -DENSITY * _tilted(1.0),
    "|u|>1": el._cell(f1=1.0, f2=0.5, f3=-0.75, f4=-0.375),      # finite and far from equilibrium: u = (14/3, 7/3)
    "sum 0, infinite u": el._cell(f1=1.0, f2=0.5, f3=-1.0, f4=-0.5),
    "all zero": np.zeros(9),
}
EXTREME_SEED = 11
EXTREME_SHAPES = [(130, 6), (7, 5)]


def extreme_places(nx, ny):
    """[(kind, x, y)]: rows 0 .. ny-4 only (their feeders are rows ny-1 .. ny-3: none is the lid row ny-2).  Even nx: row 0
    holds every kind at both cells of one lane pair at once, row 1 at the even cell of a pair, row 2 at the odd cell --
    and the last kind closes the row, x = nx-2 and nx-1.  Odd nx (one cell per lane, no pairs): row 0 from x = 0, row 1
    one column on, wrapping."""
    kinds = list(EXTREME_KINDS)
    out = []
    if nx % 2 == 0:
        assert ny >= 6 and nx >= 18 * len(kinds)
        for i, kind in enumerate(kinds):
            x = 18 * i + 6 if i + 1 < len(kinds) else nx - 2
            out += [(kind, x, 0), (kind, x + 1, 0), (kind, 18 * i + 2, 1), (kind, 18 * i + 13, 2)]
    else:
        assert ny >= 5 and nx >= len(kinds)
        for i, kind in enumerate(kinds):
            out += [(kind, i, 0), (kind, (i + 1) % nx, 1)]
    return out


def build_extreme(nx, ny, seed=EXTREME_SEED):
    """(ob, cells, places) on the double engine's own test lattice, 0.5 .. 1.5 x equilibrium with 15 % obstacles."""
    rng = np.random.default_rng(seed)
    ob = (rng.random((ny, nx)) < 0.15).astype(np.int32)
    cells = double_model.init_cells(nx, ny, DENSITY) * (0.5 + rng.random((ny, nx, 9)))
    places = extreme_places(nx, ny)
    for kind, x, y in places:
        el._scatter(cells, ob, x, y, EXTREME_KINDS[kind])
    return ob, cells, places


def build_signed_zeros(nx, ny):
    """(ob, cells): a stored fluid cell of nine -0.0 at x = 2 and 3 of row 0 (both cells of a pair where nx is even), one of
    nine +0.0 at x = 4 and 5, on a random positive lattice.  For a lattice that is read without a step."""
    rng = np.random.default_rng(17)
    ob = (rng.random((ny, nx)) < 0.15).astype(np.int32)
    cells = double_model.init_cells(nx, ny, DENSITY) * (0.5 + rng.random((ny, nx, 9)))
    ob[0, 2:6] = 0
    cells[0, 2:4] = -0.0
    cells[0, 4:6] = 0.0
    return ob, cells


def extreme_run(nx, ny, steps=(1, 2, 4)):
    """The model's lattice, final_state and av_vels after 1, 2 and 4 steps; once per shape.  (Non-finite values travel one
    cell per step: after 4 steps the 7 x 5 lattice holds nothing else, after 2 it still holds numbers.)"""
    if ("extreme", nx, ny) not in _runs:
        ob, start, places = build_extreme(nx, ny)
        cells, after, av = start.copy(), {}, []
        with np.errstate(all="ignore"):
            for t in range(1, max(steps) + 1):
                double_model.timestep(cells, ob, DENSITY, ACCEL, OMEGA)
                av.append(double_model.av_velocity(cells, ob))
                if t in steps:
                    after[t] = {"cells": cells.copy(), "final": double_model.final_state(cells, ob, DENSITY)}
        av = np.array(av)
        for a in (ob, start, av, *(s["cells"] for s in after.values()), *(f for s in after.values() for f in s["final"].values())):
            a.setflags(write=False)
        _runs[("extreme", nx, ny)] = dict(ob=ob, start=start, places=places, after=after, av=av)
    return _runs[("extreme", nx, ny)]
