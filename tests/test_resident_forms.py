"""Every one of the resident kernel's 50 forms has a GPU case that launches it -- shown without a GPU.

tests/resident_forms.py holds the forms (FORMS) and the cases of tests/test_gpu_resident_forms.py.  Here each case is
planned by tests/plan_dump.cpp (lbm_plan.h, 256 CUs): the plan must run the resident kernel with the rows, grouping and
placement the case expects, and "resident_form" (lbm_plan::resident_form, the index resident_kernel() in lbm_hip.hip
uses) must be the shape the case claims -- so a planner change that moves a case onto another form fails here instead of
leaving a form unlaunched on the GPU.  The (nx, ny, env) lists of the recorder tests that existed before are pinned to
the forms they really launch in the same way.
"""
import collections
import importlib

import numpy as np
import pytest

import plan_tool
import resident_forms
from resident_forms import CASES, CUS, EXISTING, EXISTING_USERS, FORMS, GEOMETRY, REC, SHAPES


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return plan_tool.build(tmp_path_factory.mktemp("plan_dump_forms"))


@pytest.fixture(scope="module")
def planned(plan_dump):
    """geometry name -> plan_dump's answer, one planner run per geometry."""
    return {name: plan_tool.run(plan_dump, nx=g[0], ny=g[1], cus=CUS, env=dict(g[2], LBM_RESIDENT_MIN_STEPS="1"))
            for name, g in GEOMETRY.items()}


def test_there_are_50_forms():
    assert len(FORMS) == 50 == len(set(FORMS))
    assert set(FORMS) == {(b, r, s) for b in (0, 1) for r in REC for s in range(5)}
    assert REC == ("none", "frames", "probes", "mean", "fields")
    # resident_form<BATCH, REC>'s switch: two 1024-thread shapes, one JOINT shape, and that one has four-row bands
    assert sorted(SHAPES) == [0, 1, 2, 3, 4]
    assert [s for s, (maxt, _, _) in SHAPES.items() if maxt == 1024] == [0, 2]
    assert [s for s, (_, joint, rows) in SHAPES.items() if joint] == [3] and SHAPES[3][2] == 4
    assert [rows for _, _, rows in SHAPES.values()] == [2, 2, 4, 4, 4]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_the_case_launches_the_form_it_claims(planned, case):
    got = planned[case.geometry]
    plan = got["plan"]
    assert plan["resident"] == 1 and plan["resident_min_steps"] == 1
    assert got["resident_form"] == case.shape == case.form[2], (got["resident_form"], plan)
    maxt, joint, rows = SHAPES[case.shape]
    assert plan["resident_rows"] == rows == case.rows and plan["resident_joint"] == int(joint)
    assert case.nx <= maxt and (maxt == 1024) == (case.nx > 512)
    assert plan["resident_bands"] == case.bands == case.ny // rows
    # what Engine.info() will report (lbm_get_info)
    assert case.expect == {"resident_rows": plan["resident_rows"], "resident_group": plan["resident_group"],
                           "resident_one_xcd": plan["resident_one_xcd"]}
    assert case.env == dict(GEOMETRY[case.geometry][2], LBM_RESIDENT_MIN_STEPS="1")
    if rows == 4:
        assert (case.ny - 2) % 4 == 2, "the lid row is not an interior row of a four-row band"
    assert case.ny % 4 == 0 and case.ny // 4 >= 3, "a four-row band's south and north neighbours would be one band"
    assert (case.batch == 1) == (case.members > 1)


def test_every_form_is_claimed_exactly_once():
    """The ledger, form -> cases: one "form" case each; the placement and two-launch extras claim forms a second time."""
    ledger = collections.OrderedDict((form, []) for form in FORMS)
    extras = collections.OrderedDict((form, []) for form in FORMS)
    for case in CASES:
        (ledger if case.kind == "form" else extras)[case.form].append(case.id)
    for form, ids in ledger.items():
        print(f"ledger {'batch ' if form[0] else 'single'} {form[1]:7s} shape {form[2]}  {' '.join(ids + extras[form])}")
    assert all(len(ids) == 1 for ids in ledger.values()), {f: ids for f, ids in ledger.items() if len(ids) != 1}
    assert sorted(c.kind for c in CASES if c.kind != "form") == ["placement"] * 5 + ["two-launch"] * 4
    # the other member placement, blockIdx.x / round_up(member_wgs, 8), on every recorder at a member_wgs that is no
    # multiple of 8 (the stride is rounded up); one-XCD placement on shape 1's own cases
    placement = [c for c in CASES if c.kind == "placement"]
    assert [c.rec for c in placement] == list(REC) and all(c.shape == 1 and not c.one_xcd and c.bands % 8 != 0 for c in placement)
    assert all(c.one_xcd == (c.shape == 1) for c in CASES if c.kind == "form")
    # three members everywhere else: two armed ones around an unarmed one, all in one launch
    assert all(c.members == 3 and c.launches == 1 and c.armed == (0, 2) and c.unarmed == [1]
               for c in CASES if c.batch and c.kind != "two-launch")
    assert all(c.members == 1 and c.armed == (0,) for c in CASES if not c.batch)


def test_two_launch_cases_arm_a_member_of_the_second_launch():
    two = [c for c in CASES if c.kind == "two-launch"]
    assert [(c.rec, c.geometry, c.shape, c.bands, c.per_launch, c.members) for c in two] == [
        ("frames", "576x256", 0, 128, 2, 3), ("probes", "576x256", 0, 128, 2, 3),
        ("mean", "320x256-rows4", 4, 64, 4, 5), ("fields", "320x256-rows4", 4, 64, 4, 5)]
    for c in two:
        assert c.launches == 2 and c.armed[0] < c.per_launch <= c.armed[1] == c.members - 1
        assert c.bands % 8 == 0, "the XCD-affinity band permutation does not run inside a member"
        assert c.bands * c.per_launch <= CUS and -(-c.bands // 8) * c.per_launch <= CUS // 8


@pytest.mark.parametrize("nx,ny,env,form", EXISTING,
                         ids=[f"{nx}x{ny}" + "".join(f"-{k[13:]}{v}" for k, v in env.items()) for nx, ny, env, _ in EXISTING])
def test_what_the_older_recorder_tests_launch(plan_dump, nx, ny, env, form):
    """resident_forms' table of the forms the older parameter lists run: LBM_RESIDENT_JOINT has no say under two-row bands,
    which the planner prefers wherever ny / 2 <= CUs."""
    got = plan_tool.run(plan_dump, nx=nx, ny=ny, cus=CUS, env=dict(env, LBM_RESIDENT_MIN_STEPS="1"))
    plan = got["plan"]
    assert plan["resident"] == 1
    assert got["resident_form"] == form, (nx, ny, env, got["resident_form"])
    assert SHAPES[form][1:] == (bool(plan["resident_joint"]), plan["resident_rows"])
    if "LBM_RESIDENT_ROWS" not in env:
        assert plan["resident_rows"] == (2 if ny // 2 <= CUS else 4) and plan["resident_joint"] == 0


def test_the_older_parameter_lists_are_the_table():
    """The lists are read from the modules' own parametrize marks, so an added shape has to be added to EXISTING."""
    listed = [(nx, ny, env) for nx, ny, env, _ in EXISTING[:9]]
    for module, (name, count) in EXISTING_USERS.items():
        mod = importlib.import_module(module)
        if module == "test_gpu_fields":                      # parametrised by the names of its RESIDENT_SHAPES
            params = [tuple(v) for v in mod.RESIDENT_SHAPES.values()]
            assert params == [listed[i] for i in (0, 1, 3, 5, 7)]
        else:
            mark = next(m for m in getattr(mod, name).pytestmark if m.name == "parametrize" and "nx" in m.args[0])
            params = [tuple(v) for v in mark.args[1]]
        assert len(params) == count and all(p in listed for p in params), (module, params)
    # the reference data sets of test_resident_reference_datasets (frames, probes, mean): the last four of EXISTING
    import conftest
    for module in ("test_gpu_frames", "test_gpu_probes", "test_gpu_mean"):
        marks = importlib.import_module(module).test_resident_reference_datasets.pytestmark
        names = {v if isinstance(v, str) else v[0] for m in marks if m.name == "parametrize" and "name" in m.args[0] for v in m.args[1]}
        shapes = {(p.nx, p.ny) for p in (conftest.dataset(name)[0] for name in names)}
        assert shapes <= {e[:2] for e in EXISTING[9:] if not e[2]} and (1024, 1024) in shapes, (module, names)
    # shape 4 had no case at all; shape 2 a single engine's only, through the 1024 x 1024 data set
    assert {form for _, _, _, form in EXISTING} == {0, 1, 2, 3}
    assert [e[:2] for e in EXISTING if e[3] == 2] == [(1024, 1024)] and [e[:2] for e in EXISTING if e[3] == 3] == [(128, 64)]


def test_the_lattices_mark_the_seams():
    for name, (nx, ny, _, shape, rows, _) in GEOMETRY.items():
        p, ob, cells = resident_forms.lattice(nx, ny)
        assert (p.nx, p.ny) == (nx, ny) == ob.shape[::-1] and cells.shape == (ny, nx, 9)
        cols = resident_forms.wave_edge_columns(nx)
        assert {0, 63, 64, nx - 1} <= set(cols) and ((nx == 576) == (512 in cols))
        lid = ny - 2
        assert ob[lid, ::5].all() and (ob[lid] == 0).sum() > nx // 2
        assert all(ob[lid, x] == 0 for x in (63, 64, 1))                     # fluid lid cells at the first wave seam
        for band in range(ny // 4):                                          # both seam rows of every four-row band
            assert ob[4 * band].any() and ob[4 * band + 3].any()
        assert all(ob[y].any() for y in range(ny))                           # ... and of every two-row band
        for y in resident_forms.mark_rows(ny):
            assert ob[y, cols].all()
        assert (ob == 0).sum() > 0.8 * nx * ny
        assert (ob[:, 0] == 0).any() and (ob[:, -1] == 0).any() and (ob[0] == 0).any() and (ob[-1] == 0).any()
        assert np.isfinite(cells).all() and (cells > 0).all()


def test_members_differ_and_member_0_is_the_lattice():
    params, obstacles, cells = resident_forms.member_inputs(128, 12, 3)
    p0, ob0, c0 = resident_forms.lattice(128, 12)
    assert np.array_equal(obstacles[0], ob0) and np.array_equal(cells[0], c0)
    assert (params[0].omega, params[0].accel) == (p0.omega, p0.accel)
    assert len({p.omega for p in params}) == 3 == len({p.accel for p in params})
    for i in (1, 2):
        assert not np.array_equal(obstacles[i], ob0) and not np.array_equal(cells[i], c0)
        assert obstacles[i][10, ::5].sum() < 26                              # the rolled maps keep fluid lid cells elsewhere


def test_probes_and_windows_reach_what_the_forms_differ_in():
    for nx, ny in {(g[0], g[1]) for g in GEOMETRY.values()}:
        lid, off = resident_forms.probe_sets(nx, ny)
        assert len(lid) <= 256 and all(0 <= x < nx and 0 <= y < ny for x, y in lid)
        assert not any(y == ny - 2 for _, y in off) and sum(y == ny - 2 for _, y in lid) >= 6
        for y in (ny - 2, 4, 7, 5, 6):                                       # lid, a band's seam rows, its interior rows
            xs = {x for x, yy in lid if yy == y}
            assert {0, 63, 64, nx - 1} <= xs and ((nx > 512) == any(x >= 512 for x in xs))
        assert len(set(off)) == len(off) - 1                                 # one duplicate
        windows = resident_forms.field_windows(nx, ny)
        assert windows["whole"] is None
        x0, y0, wnx, wny = windows["lid-seam"]
        assert y0 <= ny - 2 < y0 + wny and x0 <= 63 and x0 + wnx > 64 and x0 + wnx <= nx
        assert (nx > 512) == (x0 + wnx > 512)
        assert windows["rows-1-2"][1] == 1 and windows["rows-1-2"][3] == 2
        for x0, y0, wnx, wny in (w for w in windows.values() if w):
            assert 0 <= x0 and x0 + wnx <= nx and 0 <= y0 and y0 + wny <= ny
    # a sample on step 0 (the last step of the first call), on the first and the last step of a launch, and inside one
    firsts = np.cumsum((0,) + resident_forms.CALLS[:-1]).tolist()
    lasts = (np.cumsum(resident_forms.CALLS) - 1).tolist()
    for every in resident_forms.EVERY:
        steps = set(range(0, resident_forms.STEPS, every))
        assert 0 in steps and 0 in lasts and steps - set(firsts) - set(lasts)
    first_every = set(range(0, 27, resident_forms.EVERY[0]))
    assert first_every & set(firsts[1:]) and first_every & set(lasts[1:])
    # rings smaller than the run's records but not than one call's
    for every, cap, pcap in zip(resident_forms.EVERY, resident_forms.CAPACITY, resident_forms.PROBE_CAPACITY):
        per_call = max(len([t for t in range(f, l + 1) if t % every == 0]) for f, l in zip(firsts, lasts))
        assert per_call <= cap < len(range(0, 27, every)) and per_call <= pcap


def test_the_model_is_the_oracles_run(oracle):
    case = next(c for c in CASES if c.geometry == "128x12-rows4" and c.batch)
    ref, moment = resident_forms.model(case, 2)
    p, ob, cells = resident_forms.inputs(case, 2)
    again = cells.copy()
    for n in resident_forms.CALLS:
        oracle.run(p, again, ob, n)
    assert np.array_equal(ref.view(np.uint32), again.view(np.uint32))
    assert len(moment) == 27 and all(m.shape == ob.shape and (m[ob != 0] == 0).all() for m in moment)
    assert not np.array_equal(ref.view(np.uint32), cells.view(np.uint32))
