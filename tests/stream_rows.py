"""The exact rows of the stream kernels' dispatch tables, and the GPU cases that launch every one of them.

TEST INFRASTRUCTURE: numpy and the oracle binding only, no GPU.  tests/test_stream_rows.py checks all of this on the CPU
against the planner (tests/plan_dump.cpp: "plan" and "stream_rows"); tests/test_gpu_stream_rows.py runs every case
against the oracle bit for bit.

Exact arithmetic can launch 64 instantiations of the multi-step stream kernels (lbm-asynchronous_amd/csrc/lbm_hip.hip,
launch_step2 and launch_stepk; which one runs is lbm_plan::stream_row, lbm_plan.h).  EXACT_DISPATCH restates the tables
from their macros, entry by entry, and keeps the distinct instantiations.  CASES names each of them twice -- on one
periodic slab and on three slabs with device-copy halos -- at a shape where every row has strip seams:

516 x 29, band height 5
    four cells per lane: 129 lanes, three strips of 62 + 62 + 5 own lanes (one halo lane per side);
    two cells per lane: 258 lanes, five strips: 4 x 62 + 10 at K = 2 (one halo lane), 4 x 60 + 18 at K >= 3 (two);
    516 is no multiple of 64, so the row pitch is not nx;
    29 rows are bands of 5, 5, 5, 5, 5 and 4; the lid row 27 lies inside the warm-up of the band at row 0 through the wrap;
    three slabs of 10, 10 and 9 rows, each at least 2K = 8 rows, which a K = 4 pass across slabs needs.

A case runs 2K + 3 steps: full passes, a two-step pass and a one-step launch, in one call and split as (K + 1, K + 2).
"""
import functools

import numpy as np

NX, NY, BAND = 516, 29, 5
SLABS = 3                       # the cut owner: rows 10 + 10 + 9
SEED = 51629

# ---------------------------------------------------------------------------------------------------------------------
# the exact dispatch tables, as data
# ---------------------------------------------------------------------------------------------------------------------
# A row is the tuple of template arguments that differ between the instantiations of its family:
#   ("step2_stream", nts, lane_cells)         ("stepk_stream", nts, k, prefetch)
#   ("stepk_pk", nts, k, prefetch, lds)       ("stepk_pk1", nts, k, prefetch, lds)


def _table_step2():
    # launch_step2, table[0][nts][lane_cells == 2]
    return [("step2_stream", nts, lc) for nts in (0, 1) for lc in (4, 2)]


def _table_stepk():
    # launch_stepk, LBM_K_ROW: table[0][nts][k - 2][prefetch]; the K = 4 entry with prefetch is the kernel without it
    return [("stepk_stream", nts, k, pf if k < 4 else 0) for nts in (0, 1) for k in (2, 3, 4) for pf in (0, 1)]


def _table_pk():
    # LBM_PK(N, KK, PF) = {<N, KK, PF && KK < 4, 0>, <N, KK, PF && KK < 4, 1>, <N, KK, PF, KK > 2 ? 2 : 1>}
    out = []
    for nts in (0, 1):
        for k in (2, 3, 4):
            for pf in (0, 1):
                out += [("stepk_pk", nts, k, pf if k < 4 else 0, 0), ("stepk_pk", nts, k, pf if k < 4 else 0, 1),
                        ("stepk_pk", nts, k, pf, 2 if k > 2 else 1)]
    return out


def _table_pk1():
    # LBM_PK1(N, KK, PF) = {<N, KK, PF && KK < 4, 0, false, 1>, <N, KK, PF, 1, false, 1>}
    out = []
    for nts in (0, 1):
        for k in (2, 3, 4):
            for pf in (0, 1):
                out += [("stepk_pk1", nts, k, pf if k < 4 else 0, 0), ("stepk_pk1", nts, k, pf, 1)]
    return out


def _distinct(entries):
    return sorted(set(entries))


EXACT_DISPATCH = {
    "step2_stream": (_distinct(_table_step2()), "lbm_hip.hip launch_step2: table[0][nts][lane_cells == 2]"),
    "stepk_stream": (_distinct(_table_stepk()), "lbm_hip.hip launch_stepk: table[0][nts][k - 2][prefetch] (LBM_K_ROW)"),
    "stepk_pk": (_distinct(_table_pk()), "lbm_hip.hip launch_stepk: table_pk[nts][k - 2][prefetch][lds] (LBM_PK)"),
    "stepk_pk1": (_distinct(_table_pk1()), "lbm_hip.hip launch_stepk: table_pk1[nts][k - 2][prefetch][lds != 0] (LBM_PK1)"),
}
ALL_ROWS = [row for rows, _ in EXACT_DISPATCH.values() for row in rows]
TABLE_ENTRIES = {"step2_stream": len(_table_step2()), "stepk_stream": len(_table_stepk()), "stepk_pk": len(_table_pk()),
                 "stepk_pk1": len(_table_pk1())}


def row_of_json(r):
    """A row of plan_dump's "stream_rows" as the tuple used here."""
    assert r["math"] == 0
    if r["family"] == "step2_stream":
        return ("step2_stream", r["nts"], r["lane_cells"])
    if r["family"] == "stepk_stream":
        return ("stepk_stream", r["nts"], r["k"], r["prefetch"])
    assert r["family"] in ("stepk_pk", "stepk_pk1") and r["lane_cells"] == (4 if r["family"] == "stepk_pk" else 2)
    return (r["family"], r["nts"], r["k"], r["prefetch"], r["lds"])


def row_k(row):
    return 2 if row[0] == "step2_stream" else row[2]


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
PLAN_FIELDS = ("pass_steps", "lane_cells", "packed", "lds_windows", "prefetch", "xcd_chunk", "nts", "band_rows", "band_groups",
               "use_graph", "use_stepk")
INFO_FIELDS = ("steps_per_launch", "lane_cells", "band_rows", "band_groups", "nontemporal", "n_slabs")


def request_of_row(row, chunk=0, groups=1, graph=0):
    """The plan that asks for `row` and nothing else: every field of PLAN_FIELDS."""
    fam, nts = row[0], row[1]
    if fam == "step2_stream":
        k, lane_cells, packed, pf, lds, stepk = 2, row[2], 0, 0, 0, 0
    elif fam == "stepk_stream":
        k, pf = row[2], row[3]
        # two steps without prefetch or chunks run through stepk_stream only where LBM_STEPK asks for it
        lane_cells, packed, lds, stepk = 4, 0, 0, 1 if (k == 2 and not pf and not chunk) else 0
    else:
        k, pf, lds = row[2], row[3], row[4]
        lane_cells, packed, stepk = (4 if fam == "stepk_pk" else 2), 1, 0
    return {"pass_steps": k, "lane_cells": lane_cells, "packed": packed, "lds_windows": lds, "prefetch": pf, "xcd_chunk": chunk,
            "nts": nts, "band_rows": BAND, "band_groups": groups, "use_graph": graph, "use_stepk": stepk}


def literal_row(request):
    """The table entry a request names when nothing of it is dropped or folded: what the case must launch."""
    r = request
    if r["packed"]:
        return ("stepk_pk" if r["lane_cells"] == 4 else "stepk_pk1", r["nts"], r["pass_steps"], r["prefetch"], r["lds_windows"])
    if r["lane_cells"] == 4 and (r["pass_steps"] > 2 or r["prefetch"] or r["xcd_chunk"] or r["use_stepk"]):
        return ("stepk_stream", r["nts"], r["pass_steps"], r["prefetch"])
    return ("step2_stream", r["nts"], r["lane_cells"])


class Case:
    """One engine configuration.  owner: "periodic" (one slab, wraps onto itself), "slabs" (three slabs, device-copy
    halos) or "rank" (the rank API on a ring of one: LBM_FORCE_HALO=1, halo rows through RCCL, wrap = 0).  request: the
    plan asked for (PLAN_FIELDS); env: the LBM_* variables that ask for it; expect: the Engine.info() entries
    (INFO_FIELDS) plus "graph" -- whether graph_steps > 0; row: the row of EXACT_DISPATCH its full passes launch."""

    def __init__(self, row, owner, chunk=0, groups=1, graph=0, label=""):
        self.row, self.owner, self.nx, self.ny = row, owner, NX, NY
        self.slabs = SLABS if owner == "slabs" else 1
        self.request = r = request_of_row(row, chunk, groups, graph)
        self.k = r["pass_steps"]
        self.env = {"LBM_FUSE2": "1", "LBM_LANE_CELLS": str(r["lane_cells"]), "LBM_PACKED": str(r["packed"]),
                    "LBM_LDS_WINDOWS": str(r["lds_windows"]), "LBM_PASS_STEPS": str(r["pass_steps"]),
                    "LBM_PREFETCH": str(r["prefetch"]), "LBM_XCD_CHUNK": str(r["xcd_chunk"]), "LBM_STEPK": str(r["use_stepk"]),
                    "LBM_NTS": str(r["nts"]), "LBM_BAND_ROWS": str(r["band_rows"])}
        if owner == "periodic":
            # below 64 Ki cells graph replay is the default of a periodic slab: every case says which it wants
            self.env.update({"LBM_GRAPH": str(graph), "LBM_BAND_GROUPS": str(groups)})
            if graph:
                self.env["LBM_GRAPH_PASSES"] = "2"      # a chunk of two passes, so that 2K + 3 steps replay one
        elif owner == "slabs":
            self.env["LBM_HALO"] = "memcpy"
        else:
            self.env["LBM_FORCE_HALO"] = "1"
        assert owner == "periodic" or (groups == 1 and not graph)
        self.expect = {"steps_per_launch": self.k, "lane_cells": r["lane_cells"], "band_rows": BAND, "band_groups": groups,
                       "nontemporal": r["nts"], "n_slabs": self.slabs, "graph": bool(graph)}
        self.steps = 2 * self.k + 3
        self.calls = ((self.steps,), (self.k + 1, self.k + 2))
        extra = "".join(f"-{name}{value}" for name, value, dflt in (("chunk", chunk, 0), ("G", groups, 1), ("graph", graph, 0))
                        if value != dflt)
        self.id = f"{owner}-{'-'.join(str(x) for x in row)}{extra}" + (f"-{label}" if label else "")

    # geometry of the plan asked for (lbm_plan.h: plan_kernels)
    @property
    def halo_lanes(self):
        return -(-self.k // self.request["lane_cells"])

    @property
    def strip_lanes(self):
        return 64 - 2 * self.halo_lanes

    @property
    def lanes(self):
        return self.nx // self.request["lane_cells"]

    @property
    def n_strips(self):
        return -(-self.lanes // self.strip_lanes)

    def slab_rows(self):
        n = self.slabs
        return [self.ny // n + (1 if s < self.ny % n else 0) for s in range(n)]

    def band_counts(self):
        """Bands of every launch of a full pass (run_passes / issue_pass / issue_grouped_pass): the whole periodic slab;
        interior and the two boundary bands of a slab with halos; group interiors and the G seam bands."""
        k, g = self.k, self.request["band_groups"]
        if self.owner == "periodic" and g == 1:
            return [-(-self.ny // BAND)]
        if self.owner == "periodic":
            h = self.ny // g
            heights = [h] * (g - 1) + [self.ny - (g - 1) * h]
            return [-(-(x - 2 * k) // BAND) for x in heights] + [g]
        return [n for rows in self.slab_rows() for n in (-(-(rows - 2 * k) // BAND), 2)]

    def chunk_counts(self):
        c = self.request["xcd_chunk"]
        return [bands * -(-self.n_strips // c) for bands in self.band_counts()] if c else []


def _pick(rows, **want):
    """The first row of `rows` with these template arguments."""
    names = {"nts": 1, "k": 2, "prefetch": 3, "lds": 4}
    for row in rows:
        if all(row[names[key]] == value for key, value in want.items()):
            return row
    raise KeyError(want)


def _cases():
    out = []
    # every row, per owner
    for owner in ("periodic", "slabs"):
        out += [Case(row, owner) for row in ALL_ROWS]
    stepk, pk, pk1 = (EXACT_DISPATCH[f][0] for f in ("stepk_stream", "stepk_pk", "stepk_pk1"))
    # XCD chunks of two strips: 2 + 1 strips on four-cell lanes, 2 + 2 + 1 on two-cell lanes; per family, K and owner
    for owner in ("periodic", "slabs"):
        for k in (2, 3, 4):
            out.append(Case(_pick(stepk, nts=0, k=k, prefetch=1 if k < 4 else 0), owner, chunk=2))
            out.append(Case(_pick(pk, nts=0, k=k, prefetch=1, lds=min(2, k - 1)), owner, chunk=2))
            out.append(Case(_pick(pk1, nts=0, k=k, prefetch=1, lds=1), owner, chunk=2))
    # band groups on the periodic slab: the packed rows with no and with two windows in LDS, and the scalar K = 4 row.
    # G = 3 at K = 4 leaves the first two groups an interior of one row (29 / 3 - 8)
    for g in (2, 3):
        for k in (3, 4):
            out.append(Case(_pick(pk, nts=0, k=k, prefetch=0, lds=0), "periodic", groups=g))
            out.append(Case(_pick(pk, nts=0, k=k, prefetch=1, lds=2), "periodic", groups=g))
        out.append(Case(_pick(stepk, nts=0, k=4), "periodic", groups=g))
    # graph replay, one row of each family
    for row in (("step2_stream", 0, 2), _pick(stepk, nts=0, k=3, prefetch=1), _pick(pk, nts=0, k=4, prefetch=1, lds=2),
                _pick(pk1, nts=0, k=3, prefetch=1, lds=1)):
        out.append(Case(row, "periodic", graph=1))
    # the rank API on a ring of one, one row of each family
    for row in (("step2_stream", 0, 4), _pick(stepk, nts=0, k=3, prefetch=0), _pick(pk, nts=0, k=4, prefetch=1, lds=2),
                _pick(pk1, nts=0, k=3, prefetch=1, lds=0)):
        out.append(Case(row, "rank"))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), "case ids must be unique"
    return out


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------------
# the lattice
# ---------------------------------------------------------------------------------------------------------------------
def seam_columns():
    """The first column of every strip but the first, for each strip geometry a case has."""
    out = set()
    for lane_cells, strip_lanes in ((4, 62), (2, 62), (2, 60)):
        width = lane_cells * strip_lanes
        out |= set(range(width, NX, width))
    return sorted(out)


LID_ROW = NY - 2
# the lid row; the first and last row of a band (bands of 5 from row 0: 0-4, 5-9, ..., 25-28); the boundary rows of
# the slabs (0-9, 10-19, 20-28)
MARK_ROWS = (0, 4, 5, 9, 10, 19, 20, 25, LID_ROW, NY - 1)
# both sides of every seam, and the two ends of a row (neighbours through the wrap in x)
MARK_COLUMNS = tuple(sorted({x for s in seam_columns() for x in (s - 1, s)} | {0, NX - 1}))


@functools.lru_cache(maxsize=None)
def lattice():
    """(Params, obstacles, cells) every case starts from: test_gpu_parity.random_case without side walls, so both wraps
    are live, with blocked cells on both sides of every strip seam and at both ends of the row, on MARK_ROWS."""
    import conftest
    from test_gpu_parity import random_case
    p, ob, cells = random_case(conftest.load_package(), NX, NY, SEED, walls=False)
    for y in MARK_ROWS:
        ob[y, list(MARK_COLUMNS)] = 1
    ob.setflags(write=False)
    cells.setflags(write=False)
    return p, ob, cells


@functools.lru_cache(maxsize=None)
def model(steps):
    """The oracle's run of the lattice: (cells, av_vels, final_state), computed once per step count and never changed."""
    import oracle_binding
    oracle = oracle_binding.load()
    p, ob, cells = lattice()
    cur = cells.copy()
    av = oracle.run(p, cur, ob, steps)
    fields = oracle.final_state(p, cur, ob)
    for a in (cur, av, *fields.values()):
        a.setflags(write=False)
    return cur, av, fields
