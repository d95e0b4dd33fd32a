"""The kernel plan, pinned without a GPU.

tests/golden/kernel_plans.json holds what the engine chose before the planner existed -- every selection and geometry
field of lbm_plan::KernelPlan and every slab's rows, lid-row images and one-step launch sizes -- for grids,
decompositions and LBM_* knobs that between them take every branch of the selection.  plan_kernels / slab_rows
(lbm-asynchronous_amd/csrc/lbm_plan.h) are pure host arithmetic: tests/plan_dump.cpp, built as a stand-alone program
under AddressSanitizer and UBSan, must reproduce every field of every case exactly.  A change of a default, a threshold
or a cost model shows up here as a diff of the table.

PROVENANCE OF THE TABLE -- NOT YET WHAT WAS ASKED FOR.  The table was to be recorded on an MI355X from an instrumented
build of the commit before the planner.  No device could be had when this was written, so the table was produced on
the host instead: that commit's own selection code (plan_stream and the body of create_common, verbatim), compiled
with the device queries answered by the MI355X's public numbers (256 CUs, one device) and the occupancy query taken to
admit every shape the arithmetic admits.  It therefore pins the planner to the previous code, not to a device record;
the resident fields in particular are the candidate, not an answer confirmed by a device.  Re-record on the device
and replace the table (same format) when one is available.
"""
import json
import os

import pytest

import plan_tool

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_plans.json")

with open(TABLE) as f:
    CASES = json.load(f)


def case_id(case):
    env = ",".join(f"{k[4:]}={v}" for k, v in sorted(case["env"].items()))
    return f"{case['nx']}x{case['ny']}/{case['n_slabs']}/{case['kind']}" + (f"[{env}]" if env else "")


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return plan_tool.build(tmp_path_factory.mktemp("plan_dump"))


def test_table_covers_the_selection():
    """The cases the plan is pinned on: no duplicates, and each kernel family, band model and placement occurs."""
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    assert 100 <= len(CASES) < 300
    plans = [c["plan"] for c in CASES]
    assert {p["resident_group"] for p in plans if p["resident_one_xcd"]} == {1, 2, 4}
    assert {p["tile_shape"] for p in plans if p["tile_steps"]} >= {0, 1, 3}
    assert {(p["lane_cells"], p["pass_steps"]) for p in plans if p["fuse2"]} >= {(2, 2), (2, 3), (4, 2), (4, 3), (4, 4)}
    assert {p["band_groups"] for p in plans} == {1, 2, 3}
    assert any(p["xcd_chunk"] for p in plans) and any(p["want_team"] for p in plans)
    assert any(p["use_graph"] and c["halo"] for c, p in zip(CASES, plans))
    assert {c["halo"] for c in CASES} == {0, 1, 2, 3}
    assert any(s["accel_row2"] > -1000000 for c in CASES for s in c["slabs"])
    assert any(s["accel_row"] < 0 for c in CASES for s in c["slabs"] if s["accel_row"] > -1000000)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_planner_reproduces_the_recorded_plan(plan_dump, case):
    got = plan_tool.run(plan_dump, nx=case["nx"], ny=case["ny"], world=case["world"], rank=case["rank"],
                        n_slabs=case["n_slabs"], halo=case["halo"], cus=case["cus"], n_devices=case["n_devices"],
                        distinct_devices=case["distinct_devices"], env=case["env"])
    assert got["plan"] == case["plan"]
    assert got["slabs"] == case["slabs"]
