"""The inputs of tests/double_edge_lattice.py do what they claim, and tests/double_model.py decides and computes on them
what the reference does -- by the CPU alone.  Conditions on the inputs, not measurements of any kernel: the GPU
comparison (tests/test_gpu_double_edges.py) means nothing without them.

1. tests/double_cell_reference.py, a per-cell reading of the reference in plain Python floats, agrees with double_model
   bit for bit (NaN matches NaN) on every special and extreme cell and on a whole small lattice;
2. the model's lid-row decision equals the exact rational comparison, on every fluid lid cell of every step;
3. the refusal lattice offers accepting, refusing and singly-failing cells, its specials decide as listed, it stays finite;
4. the extreme cells arrive at step 0's collision as placed and show their property;
5. the density of a cell of nine -0.0 is +0.0, as the reference's sum from 0.f makes it."""
from fractions import Fraction

import numpy as np
import pytest

import double_cell_reference as cell_ref
import double_edge_lattice as dl
import double_model

TINY = np.finfo(np.float64).tiny


def same(a, b):
    """Bit for bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ---- 1. the per-cell reference -----------------------------------------------------------------------------------
def model_collision(t):
    """double_model's collision of one pre-collision cell: cell (1, 1) of a 3 x 5 lattice pulls T from rows 0 .. 2, none
    of them the lid row 3."""
    cells = np.ones((5, 3, 9)) * 0.01
    ob = np.zeros((5, 3), dtype=np.int32)
    dl.el._scatter(cells, ob, 1, 1, t)
    with np.errstate(all="ignore"):
        double_model.timestep(cells, ob, dl.DENSITY, dl.ACCEL, dl.OMEGA)
    return np.array(t, dtype=np.float64), cells[1, 1]


@pytest.mark.parametrize("kind", list(dl.EXTREME_KINDS))
def test_cell_reference_agrees_on_every_extreme_kind(kind):
    t, want = model_collision(dl.EXTREME_KINDS[kind])
    assert same(cell_ref.collide_cell([float(v) for v in t], dl.OMEGA), want), kind


@pytest.mark.parametrize("name", list(dl.LID_SPECIALS))
def test_cell_reference_agrees_on_every_lid_special(name):
    """accelerate_flow of the special, then its collision as a pre-collision cell."""
    (f3, f6, f7), accepts, _ = dl.LID_SPECIALS[name]
    rng = np.random.default_rng(7)
    cell = dl.DENSITY * dl.el.WEIGHTS * (0.95 + 0.1 * rng.random(9))
    cell[3], cell[6], cell[7] = f3, f6, f7
    row = np.tile(cell, (4, 2, 1))            # ny = 4: the lid row is row 2
    double_model.accelerate_flow(row, np.zeros((4, 2), dtype=bool), dl.DENSITY, dl.ACCEL)
    got = cell_ref.accelerate_cell([float(v) for v in cell], dl.DENSITY, dl.ACCEL)
    assert same(got, row[2, 0]) and same(row[1, 0], cell)
    assert (got != [float(v) for v in cell]) == accepts, name
    if name == "f3==next(a1)":
        assert 0.0 < got[3] <= np.spacing(dl.A1)
    t, want = model_collision(got)
    assert same(cell_ref.collide_cell([float(v) for v in t], dl.OMEGA), want), name


def test_cell_reference_agrees_on_a_whole_lattice():
    """8 x 3 (the smallest grid: lid row 1, both wraps), blocked cells on and off the lid row, five steps."""
    rng = np.random.default_rng(83)
    ob = (rng.random((3, 8)) < 0.2).astype(np.int32)
    ob[1, 0], ob[1, 5] = 0, 1
    cells = double_model.init_cells(8, 3, dl.DENSITY) * (0.5 + rng.random((3, 8, 9)))
    nested = cells.tolist()
    for t in range(5):
        double_model.timestep(cells, ob, dl.DENSITY, dl.ACCEL, dl.OMEGA)
        nested = cell_ref.timestep(nested, ob.tolist(), dl.DENSITY, dl.ACCEL, dl.OMEGA)
        assert same(np.array(nested), cells), t


# ---- 2., 3. the refusal lattice ----------------------------------------------------------------------------------
def covered(c):
    return (c["accept"] >= 8 and c["refuse"] >= 8 and c["only f3"] + c["only f6"] + c["only f7"] >= 4
            and min(c["only f3"], c["only f6"], c["only f7"]) >= 1)


@pytest.mark.parametrize("nx,ny", dl.REFUSAL_SHAPES)
def test_model_decides_by_the_exact_comparison(nx, ny):
    """(f - a) > 0.0 in float64 is f > a over the rationals (a difference of doubles rounds to zero only if it is zero):
    the model's own accelerate_flow, judged by whether it changed the cell, against Fraction on every fluid lid cell."""
    run = dl.refusal_run(nx, ny)
    a1, a2 = Fraction(dl.A1), Fraction(dl.A2)
    blocked = run["ob"] != 0
    assert dl.A1 == dl.DENSITY * dl.ACCEL / 9.0 and dl.A2 == dl.DENSITY * dl.ACCEL / 36.0     # as the host forms them
    for t, lid in enumerate(run["lids"]):
        after = np.zeros((ny, nx, 9))
        after[ny - 2] = lid
        double_model.accelerate_flow(after, blocked, dl.DENSITY, dl.ACCEL)
        changed = (after[ny - 2] != lid).any(axis=1)
        d = dl.lid_decisions(lid, run["ob"][ny - 2])
        for x in range(nx):
            exact = (not blocked[ny - 2, x] and Fraction(float(lid[x, 3])) > a1 and Fraction(float(lid[x, 6])) > a2
                     and Fraction(float(lid[x, 7])) > a2)
            assert bool(changed[x]) == exact == bool(d["accept"][x]), (t, x)


@pytest.mark.parametrize("nx,ny", dl.REFUSAL_SHAPES)
def test_refusal_lattice_meets_its_conditions(nx, ny):
    run = dl.refusal_run(nx, ny)
    for t, c in enumerate(run["counts"]):
        print(f"{nx}x{ny} before step {t}: {c}")
    # step 0 (the accelerate_row pass of a single call) and every step from 7 on (the step kernel's epilogue)
    for t in (0, *range(7, dl.STEPS)):
        assert covered(run["counts"][t]), (t, run["counts"][t])
    # every special decides as listed, at an even and at an odd column, the row ends among them
    d = dl.lid_decisions(run["lids"][0], run["ob"][ny - 2])
    seen = {}
    for x, name in run["specials"]:
        _, accepts, fails = dl.LID_SPECIALS[name]
        assert run["ob"][ny - 2, x] == 0 and bool(d["accept"][x]) == accepts, (name, x)
        if fails is not None:
            assert d["only"][fails][x], (name, x)
        seen.setdefault(name, set()).add(x % 2)
    assert all(v == {0, 1} for v in seen.values()) and set(seen) == set(dl.LID_SPECIALS)
    xs = dict(run["specials"])
    assert 0 in xs and nx - 1 in xs
    lid0 = run["lids"][0]
    x = next(x for x, name in run["specials"] if name == "f3==a1")
    assert lid0[x, 3] - dl.A1 == 0.0 and lid0[x, 6] > 2 * dl.A2 and lid0[x, 7] > 2 * dl.A2
    x = next(x for x, name in run["specials"] if name == "f3<0")
    assert lid0[x, 3] < 0.0
    # finite throughout, a flow that counts
    assert all(np.isfinite(s).all() for s in run["states"])
    assert np.isfinite(run["av"]).all() and (run["av"] > 0).all()


# ---- 4. the extreme lattice --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", dl.EXTREME_SHAPES)
def test_extreme_cells_arrive_and_show_their_property(nx, ny):
    ob, cells, places = dl.build_extreme(nx, ny)
    blocked = ob != 0
    pre = cells.copy()
    double_model.accelerate_flow(pre, blocked, dl.DENSITY, dl.ACCEL)
    tmp = double_model.propagate(pre)
    with np.errstate(all="ignore"):
        rho, u_x, u_y = double_model._moments(tmp)
    denormal = lambda v: bool(np.all((np.abs(v) > 0) & (np.abs(v) < TINY)))
    for kind, x, y in places:
        t = dl.EXTREME_KINDS[kind]
        assert same(tmp[y, x], t) and ob[y, x] == 0, (kind, x, y)
        num_x = t[1] + t[5] + t[8] - (t[3] + t[6] + t[7])
        num_y = t[2] + t[5] + t[6] - (t[4] + t[7] + t[8])
        if kind == "all denormal":
            assert denormal(t) and denormal(rho[y, x]) and 0.01 < abs(u_x[y, x]) < 1
        elif kind == "numerators denormal":
            assert denormal(num_x) and denormal(num_y) and rho[y, x] >= 0.04 and denormal(u_x[y, x]) and denormal(u_y[y, x])
        elif kind == "huge":
            assert rho[y, x] > 2.0 ** 999 and 0.01 < abs(u_x[y, x]) < 1
        elif kind == "rho<0":
            assert rho[y, x] < 0 and np.isfinite(u_x[y, x]) and u_x[y, x] != 0
        elif kind == "|u|>1":
            assert rho[y, x] == 0.375 and u_x[y, x] == 1.75 / 0.375 and u_y[y, x] == 0.875 / 0.375
        elif kind == "sum 0, infinite u":
            assert rho[y, x] == 0 and num_x != 0 and num_y != 0 and np.isinf(u_x[y, x]) and np.isinf(u_y[y, x])
        else:
            assert not t.any() and np.isnan(u_x[y, x]) and np.isnan(u_y[y, x])
    if nx % 2 == 0:                           # both cells of a lane pair, together and one at a time; the row end
        for kind in dl.EXTREME_KINDS:
            mine = [(x, y) for k, x, y in places if k == kind]
            assert any((x ^ 1, y) in mine for x, y in mine)
            assert {x % 2 for x, y in mine if (x ^ 1, y) not in mine} == {0, 1}, kind
        assert any(x == nx - 1 for _, x, _ in places)
    else:                                     # one cell per lane: two columns, two rows
        assert all(len({x for k, x, _ in places if k == kind}) == 2 for kind in dl.EXTREME_KINDS)


@pytest.mark.parametrize("nx,ny", [(8, 3), (7, 5)])
def test_density_of_negative_zeros_is_positive_zero(nx, ny):
    """`local_density = 0.f; local_density += speeds[kk]` (:325-330, :692): 0.0 + -0.0 is +0.0, so nine -0.0 sum to +0.0,
    not to the -0.0 that adding them to one another gives.  The model's pressure of such a cell is +0.0, its u NaN."""
    ob, cells = dl.build_signed_zeros(nx, ny)
    with np.errstate(all="ignore"):
        final = double_model.final_state(cells, ob, dl.DENSITY)
    assert np.signbit(cells[0, 2:4]).all() and not np.signbit(cells[0, 4:6]).any() and not cells[0, 2:6].any()
    assert not ob[0, 2:6].any()
    assert (final["pressure"][0, 2:6] == 0).all() and not np.signbit(final["pressure"][0, 2:6]).any()
    assert np.isnan(final["u"][0, 2:6]).all()
    local_density = 0.0
    for v in cells[0, 2].tolist():
        local_density += v
    assert str(local_density) == "0.0" and str(sum(cells[0, 2].tolist()[1:], cells[0, 2, 0].item())) == "-0.0"


@pytest.mark.parametrize("nx,ny", dl.EXTREME_SHAPES)
def test_extreme_run_is_what_the_gpu_tests_take_it_for(nx, ny):
    """After step 0 the finite kinds are finite and the two degenerate ones NaN, at every placement; the NaNs then
    spread as the model says (nothing here requires them to stay contained), and finite cells remain to be compared."""
    run = dl.extreme_run(nx, ny)
    one, four = run["after"][1]["cells"], run["after"][4]["cells"]
    for kind, x, y in run["places"]:
        if kind in ("sum 0, infinite u", "all zero"):
            assert np.isnan(one[y, x]).all(), (kind, x, y)
        else:
            assert np.isfinite(one[y, x]).all(), (kind, x, y)
            if kind == "all denormal":
                assert (np.abs(one[y, x]) < TINY).all() and one[y, x].any()
    n1, n4 = int(np.isnan(one).any(axis=2).sum()), int(np.isnan(four).any(axis=2).sum())
    print(f"{nx}x{ny}: cells with a NaN after 1 step {n1}, after 4 steps {n4} of {nx * ny}; av_vels {run['av']}")
    assert n4 > n1 >= sum(k in ("sum 0, infinite u", "all zero") for k, _, _ in run["places"])
    two = run["after"][2]["cells"]
    assert np.isfinite(one).all(axis=2).sum() > np.isfinite(two).all(axis=2).sum() >= 6
    assert nx % 2 or np.isfinite(four).all(axis=2).sum() > nx * ny // 2
    assert np.isnan(run["after"][1]["final"]["u"]).any() and np.isnan(run["av"]).all()
