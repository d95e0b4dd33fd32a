"""The one ring the four gather kinds share (obstacle forces, lattice statistics, velocity residuals, line profiles; on a
context Slab::gather_ring, on a batch lbm_batch::gather_ring): what the per-kind suites do not cross-check.  One owner
arms the kinds one after another -- their slots differ in size -- and every row it reads equals, byte for byte, the row
of a fresh owner that armed only that kind at the same step; a drain that crosses the ring's end gives the rows of a ring
that never wraps; a refused arming leaves a batch clean.  Lattices: 32 x 32 (nx % 4 == 0: four cells per lane) and
30 x 32 (one cell per lane), with the blocked cells of test_gpu_stats.test_lane_wave_and_workgroup_edges; owners: a
context of one slab, one of three (the most the multi-slab suites use) and a batch of three members."""
import numpy as np
import pytest

from test_gpu_forces import small

pytestmark = pytest.mark.gpu

LATTICES = [(32, 32), (30, 32)]
OWNERS = ["engine-1", "engine-3", "batch-3"]
EVERY = 2


def case(lbm, nx, ny):
    """(p, ob, [cells of three members], labels of two bodies)"""
    p, ob, _ = small(lbm, nx, ny, nx + ny)
    ob[1, 2:4] = 1
    ob[ny - 1, nx - 1] = 1
    labels = np.zeros((ny, nx), dtype=np.int32)
    labels[ny - 1, nx - 1] = 1                                # the corner cell is body 1, the pair in row 1 body 0
    return p, ob, [small(lbm, nx, ny, nx + ny + i)[2] for i in range(3)], labels


def make_owner(lbm, monkeypatch, owner, p, ob, cells):
    if owner == "batch-3":
        return lbm.Batch([p] * 3, [ob] * 3, cells)
    monkeypatch.setenv("LBM_HALO", "memcpy")
    eng = lbm.Engine(p, ob, cells[0], n_gpus=int(owner[-1]))
    assert eng.info()["n_slabs"] == int(owner[-1])
    return eng


def arm(o, kind, every, capacity, labels):
    if kind == "stats":
        o.set_stats(every, capacity)
    elif kind == "profiles":
        o.set_profiles(every, capacity)
    elif kind == "residuals":
        o.set_residual(every, capacity)
    else:
        members = len(o) if hasattr(o, "member") else 0
        o.set_forces(every, capacity, [labels] * members if members else labels, 2)


def read(o, kind, n=None):
    """(steps, [the bytes of each record])"""
    if kind == "profiles":
        steps, lines = o.profiles(n)                          # (disarmed: no axis, no record)
        assert len(steps) == 0 or sorted(lines) == ["columns", "rows"]
        return steps.tolist(), [lines["rows"][i].tobytes() + lines["columns"][i].tobytes() for i in range(len(steps))]
    steps, rows = getattr(o, kind)(n)
    assert len(rows) == len(steps)
    return steps.tolist(), [rows[i].tobytes() for i in range(len(steps))]


def fresh_rows(lbm, monkeypatch, owner, p, ob, cells, labels, kind, start, calls):
    """{step: bytes} of an owner that ran `start` steps unarmed, armed only `kind` (a ring of 16: no wrap) and read all
    its records in one go after `calls`"""
    with make_owner(lbm, monkeypatch, owner, p, ob, cells) as o:
        if start:
            o.run(start)
        arm(o, kind, EVERY, 16, labels)
        for n in calls:
            o.run(n)
        steps, rows = read(o, kind)
    assert len(steps) == len(set(steps)) > 0 and all(len(r) == len(rows[0]) > 0 for r in rows)
    return dict(zip(steps, rows))


@pytest.mark.parametrize("owner", OWNERS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_kinds_one_after_another_on_one_owner(lbm, monkeypatch, nx, ny, owner):
    p, ob, cells, labels = case(lbm, nx, ny)
    want = {"stats": fresh_rows(lbm, monkeypatch, owner, p, ob, cells, labels, "stats", 0, [3, 2]),
            "profiles": fresh_rows(lbm, monkeypatch, owner, p, ob, cells, labels, "profiles", 5, [3]),
            "forces": fresh_rows(lbm, monkeypatch, owner, p, ob, cells, labels, "forces", 8, [4]),
            "residuals": fresh_rows(lbm, monkeypatch, owner, p, ob, cells, labels, "residuals", 12, [3])}
    assert len({len(next(iter(w.values()))) for w in want.values()}) == 4          # four record sizes
    with make_owner(lbm, monkeypatch, owner, p, ob, cells) as o:
        arm(o, "stats", EVERY, 2, labels)
        o.run(3)                                              # records of steps 0 and 2: the ring is full
        steps, rows = read(o, "stats", 1)
        assert steps == [0] and rows[0] == want["stats"][0]
        o.run(2)                                              # step 4 goes into the slot that 0 left: the ring has wrapped
        steps, rows = read(o, "stats", 1)
        assert steps == [2] and rows[0] == want["stats"][2]
        arm(o, "stats", 0, 0, labels)                         # the record of step 4 goes unread
        for kind, calls, expect in (("profiles", [3], [6]), ("forces", [4], [8, 10]), ("residuals", [3], [12, 14])):
            arm(o, kind, EVERY, 3, labels)
            for n in calls:
                o.run(n)
            steps, rows = read(o, kind)
            assert steps == expect == sorted(want[kind]), kind
            for tt, row in zip(steps, rows):
                assert row == want[kind][tt], (kind, tt)
            arm(o, kind, 0, 0, labels)
            assert read(o, kind)[0] == []


@pytest.mark.parametrize("owner", OWNERS)
@pytest.mark.parametrize("kind", ["forces", "stats", "residuals", "profiles"])
def test_a_drain_across_the_rings_end(lbm, monkeypatch, kind, owner):
    """three slots, a record per step: after three steps and a read of two, two more steps put their records into slots
    0 and 1 behind the one waiting in slot 2, and the read of everything runs over the ring's end"""
    p, ob, cells, labels = case(lbm, 30, 32)
    with make_owner(lbm, monkeypatch, owner, p, ob, cells) as o:
        arm(o, kind, 1, 16, labels)
        o.run(3)
        o.run(2)
        want_steps, want = read(o, kind)
    assert want_steps == [0, 1, 2, 3, 4] and len(set(want)) == 5
    with make_owner(lbm, monkeypatch, owner, p, ob, cells) as o:
        arm(o, kind, 1, 3, labels)
        o.run(3)
        steps, rows = read(o, kind, 2)
        assert steps == [0, 1] and rows == want[:2]
        o.run(2)
        steps, rows = read(o, kind)
        assert steps == [2, 3, 4] and rows == want[2:]


def test_a_refused_arming_leaves_the_batch_clean(lbm, monkeypatch):
    """lbm_batch_set_forces refused for a blocked cell's label: lbm_batch_set_stats then arms and records as on a fresh batch"""
    p, ob, cells, labels = case(lbm, 30, 32)
    want = fresh_rows(lbm, monkeypatch, "batch-3", p, ob, cells, labels, "stats", 2, [4])
    bad = labels.copy()
    bad[1, 3] = 7
    with make_owner(lbm, monkeypatch, "batch-3", p, ob, cells) as o:
        o.run(2)
        with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_forces: member 1: the blocked cell \(3, 1\) has body 7, outside 0 \.\. 1"):
            o.set_forces(EVERY, 4, [labels, bad, labels], 2)
        assert read(o, "forces")[0] == []
        arm(o, "stats", EVERY, 4, labels)
        o.run(4)
        steps, rows = read(o, "stats")
        assert steps == [2, 4] == sorted(want) and rows == [want[2], want[4]]
