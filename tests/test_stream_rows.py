"""Every exact row of the stream kernels' dispatch tables has a GPU case that launches it -- shown without a GPU.

tests/stream_rows.py holds the 64 rows (EXACT_DISPATCH) and the cases of tests/test_gpu_stream_rows.py.  Here each case is
planned by tests/plan_dump.cpp (lbm_plan.h, 256 CUs): the plan must be the case's request field for field, the first of
the planner's "stream_rows" must be the case's row, and the row must be the table entry the request names literally --
so a request that the planner drops, thins or folds onto another kernel (an INERT request) fails here instead of passing
on the GPU as if it had been tested.
"""
import collections

import numpy as np
import pytest

import plan_tool
import stream_rows
from stream_rows import ALL_ROWS, CASES, EXACT_DISPATCH, PLAN_FIELDS

HALO_OF_OWNER = {"periodic": "none", "slabs": "memcpy", "rank": "rccl"}


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return plan_tool.build(tmp_path_factory.mktemp("plan_dump_rows"))


@pytest.fixture(scope="module")
def planned(plan_dump):
    """case id -> plan_dump's answer, one planner run per case."""
    out = {}
    for case in CASES:
        env = {k: v for k, v in case.env.items() if k not in ("LBM_HALO", "LBM_FORCE_HALO", "LBM_GRAPH_PASSES")}
        out[case.id] = plan_tool.run(plan_dump, nx=case.nx, ny=case.ny, n_slabs=case.slabs,
                                     halo=plan_tool.HALO[HALO_OF_OWNER[case.owner]], cus=256, env=env)
    return out


def test_the_tables_have_64_distinct_rows():
    sizes = {family: len(rows) for family, (rows, _) in EXACT_DISPATCH.items()}
    assert sizes == {"step2_stream": 4, "stepk_stream": 10, "stepk_pk": 28, "stepk_pk1": 22}
    # the tables' entries before the folding: [2][2], [2][3][2], [2][3][2][3], [2][3][2][2]
    assert stream_rows.TABLE_ENTRIES == {"step2_stream": 4, "stepk_stream": 12, "stepk_pk": 36, "stepk_pk1": 24}
    assert len(ALL_ROWS) == 64 == len(set(ALL_ROWS))
    assert all("lbm_hip.hip" in where for _, where in EXACT_DISPATCH.values())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_the_plan_is_the_request_and_the_row_is_launched(planned, case):
    got = planned[case.id]
    plan = got["plan"]
    assert {f: plan[f] for f in PLAN_FIELDS} == case.request
    assert plan["fuse2"] == 1 and plan["vec4"] == 1 and plan["tile_steps"] == 0 and plan["resident"] == 0
    rows = got["stream_rows"]
    assert len(rows) == 3
    full, tail = stream_rows.row_of_json(rows[0]), stream_rows.row_of_json(rows[1])
    assert full == case.row, (full, plan)
    assert case.row == stream_rows.literal_row(case.request), "the request is folded onto another row: it is inert"
    assert case.row in ALL_ROWS and tail in ALL_ROWS and stream_rows.row_k(tail) == 2
    assert (tail == full) == (case.k == 2)
    # the two-step tail keeps the family and takes min(lds_windows, 1) windows
    if case.k > 2 and case.row[0] != "stepk_stream":
        assert tail[0] == case.row[0] and tail[4] == min(case.request["lds_windows"], 1)
    assert rows[2] == {"family": "step_vec4", "math": 0, "nts": case.request["nts"], "neigh": 0}
    # what Engine.info() will report (lbm_get_info)
    assert case.expect == {"steps_per_launch": plan["pass_steps"], "lane_cells": plan["lane_cells"], "band_rows": plan["band_rows"],
                           "band_groups": plan["band_groups"], "nontemporal": plan["nts"], "n_slabs": len(got["slabs"]),
                           "graph": bool(plan["use_graph"])}
    assert [s["rows"] for s in got["slabs"]] == case.slab_rows()
    assert case.steps == 2 * case.k + 3 and case.calls == ((case.steps,), (case.k + 1, case.k + 2))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_seams_are_present_and_chunks_are_ragged(planned, case):
    plan = planned[case.id]["plan"]
    assert plan["n_strips"] == case.n_strips >= 3 and plan["halo_lanes"] == case.halo_lanes
    assert case.lanes % case.strip_lanes != 0, "the last strip is not ragged"
    assert case.nx % 64 != 0                                # the row pitch is not nx
    assert all(rows >= 2 * case.k for rows in case.slab_rows())
    chunk = case.request["xcd_chunk"]
    if chunk:
        assert case.n_strips % chunk != 0
        counts = case.chunk_counts()
        assert counts and all(n % 8 != 0 for n in counts), counts      # trailing workgroups return early in every launch
    if case.request["band_groups"] > 1:
        assert min(case.band_counts()) >= 1                 # every group keeps an interior


def test_group_interiors_go_down_to_one_row():
    thinnest = min(case.ny // case.request["band_groups"] - 2 * case.k for case in CASES if case.request["band_groups"] > 1)
    assert thinnest == 1


def ledger(owner):
    rows = collections.OrderedDict((row, []) for row in ALL_ROWS)
    for case in CASES:
        if case.owner == owner:
            rows[case.row].append(case.id)
    return rows


def test_coverage_is_complete_per_owner(planned):
    """The ledger, row -> cases, per owner; every row has a case on one periodic slab and one on three slabs."""
    for owner in ("periodic", "slabs"):
        table = ledger(owner)
        for row, ids in table.items():
            assert all(stream_rows.row_of_json(planned[i]["stream_rows"][0]) == row for i in ids)
            print(f"ledger {owner:8s} {'-'.join(str(x) for x in row):24s} {len(ids)}  {' '.join(ids)}")
        covered = [row for row, ids in table.items() if ids]
        print(f"ledger {owner}: {len(covered)} / {len(ALL_ROWS)} rows")
        assert len(covered) == 64
    extras = [c for c in CASES if c.owner == "rank"]
    assert {c.row[0] for c in extras} == set(EXACT_DISPATCH)
    for name, pick in (("chunk", lambda c: c.request["xcd_chunk"]), ("graph", lambda c: c.request["use_graph"])):
        for owner in (("periodic", "slabs") if name == "chunk" else ("periodic",)):
            seen = {(c.row[0], c.k) for c in CASES if pick(c) and c.owner == owner}
            if name == "chunk":
                assert seen == {(f, k) for f in ("stepk_stream", "stepk_pk", "stepk_pk1") for k in (2, 3, 4)}, (name, owner)
            else:
                assert {f for f, _ in seen} == set(EXACT_DISPATCH)
    grouped = {(c.row[0], c.k, c.row[4] if len(c.row) > 4 else None, c.request["band_groups"]) for c in CASES
               if c.request["band_groups"] > 1}
    assert grouped == {("stepk_pk", k, lds, g) for k in (3, 4) for lds in (0, 2) for g in (2, 3)} | \
        {("stepk_stream", 4, None, g) for g in (2, 3)}


def test_no_request_reaches_a_row_outside_the_tables(plan_dump):
    """Every request at this shape -- the folded and thinned ones the cases leave out too -- launches rows of the 64, and
    between them the requests reach all 64 and nothing else: the tables hold no instantiation the cases could have missed."""
    reached = set()
    for packed, lane_cells, stepk in ((1, 4, 0), (1, 2, 0), (0, 4, 0), (0, 4, 1), (0, 2, 0)):
        for k in (2, 3, 4):
            for pf in (0, 1):
                for lds in ((0, 1, 2) if packed else (0,)):
                    for nts in (0, 1):
                        env = {"LBM_FUSE2": "1", "LBM_LANE_CELLS": str(lane_cells), "LBM_PACKED": str(packed),
                               "LBM_LDS_WINDOWS": str(lds), "LBM_PASS_STEPS": str(k), "LBM_PREFETCH": str(pf), "LBM_STEPK": str(stepk),
                               "LBM_NTS": str(nts), "LBM_BAND_ROWS": str(stream_rows.BAND), "LBM_GRAPH": "0"}
                        got = plan_tool.run(plan_dump, nx=stream_rows.NX, ny=stream_rows.NY, cus=256, env=env)
                        rows = [stream_rows.row_of_json(r) for r in got["stream_rows"][:2]]
                        assert all(r in ALL_ROWS for r in rows), (env, rows)
                        assert stream_rows.row_k(rows[0]) == got["plan"]["pass_steps"] and stream_rows.row_k(rows[1]) == 2
                        reached.update(rows)
    assert reached == set(ALL_ROWS)


def test_the_lattice_marks_every_seam():
    p, ob, cells = stream_rows.lattice()
    assert (p.nx, p.ny) == (stream_rows.NX, stream_rows.NY) == ob.shape[::-1] and cells.shape == (p.ny, p.nx, 9)
    assert stream_rows.seam_columns() == [120, 124, 240, 248, 360, 372, 480, 496]
    for x in (247, 248, 495, 496, 123, 124, 371, 372, 119, 120, 239, 240, 359, 360, 479, 480, 0, p.nx - 1):
        assert x in stream_rows.MARK_COLUMNS
        for y in stream_rows.MARK_ROWS:
            assert ob[y, x] != 0
    # the marked rows: the lid row, a band's first and last row, every slab's boundary rows
    assert stream_rows.LID_ROW == p.ny - 2 == 27 and stream_rows.LID_ROW in stream_rows.MARK_ROWS
    assert {0, 4, 5, 9} <= set(stream_rows.MARK_ROWS)
    first = 0
    for rows in next(c for c in CASES if c.owner == "slabs").slab_rows():
        assert first in stream_rows.MARK_ROWS and first + rows - 1 in stream_rows.MARK_ROWS
        first += rows
    assert first == p.ny
    # fluid remains: on the lid row, next to the seams on the other rows, and both wraps are open
    assert (ob[stream_rows.LID_ROW] == 0).sum() > p.nx // 2
    assert (ob == 0).sum() > 0.9 * p.nx * p.ny
    assert (ob[:, 0] == 0).any() and (ob[:, -1] == 0).any() and (ob[0] == 0).any() and (ob[-1] == 0).any()
    for s in stream_rows.seam_columns():
        assert (ob[:, s - 1] == 0).sum() >= 10 and (ob[:, s] == 0).sum() >= 10
    assert np.isfinite(cells).all() and (cells > 0).all()


def test_the_model_is_the_oracles_run(oracle):
    """model(steps) is oracle.run on a copy; run in pieces it ends in the same lattice."""
    p, ob, cells = stream_rows.lattice()
    want, av, fields = stream_rows.model(7)
    again = cells.copy()
    for n in (3, 4):
        oracle.run(p, again, ob, n)
    assert np.array_equal(want.view(np.uint32), again.view(np.uint32))
    assert len(av) >= 7 and np.isfinite(np.asarray(av)[:7]).all() and (np.asarray(av)[:7] > 0).all()
    assert set(fields) >= {"u_x", "u_y", "u", "pressure"}
    assert not np.array_equal(want.view(np.uint32), cells.view(np.uint32))
