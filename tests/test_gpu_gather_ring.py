"""The one ring the seven gather kinds share (obstacle forces, lattice statistics, velocity residuals, line profiles,
enstrophy rows, stream-function rows, coarse frames; on a context Slab::gather_ring, on a batch lbm_batch::gather_ring):
what the per-kind suites do not cross-check.  One owner arms the kinds one after another -- their slots differ in size
-- and every row it reads equals, byte for byte, the row of a fresh owner that armed only that kind at the same step; a
drain that crosses the ring's end gives the rows of a ring that never wraps; a refused arming leaves a batch clean; the
refusals every kind's setter and reader make say, word for word, what they said when each kind had its own copy of them.
Lattices: 32 x 32 (nx % 4 == 0: four cells per lane) and 30 x 32 (one cell per lane), with the blocked cells of
test_gpu_stats.test_lane_wave_and_workgroup_edges; owners: a context of one slab, one of three (the most the multi-slab
suites use) and a batch of three members.  The coarse box, 7 x 3, is ragged in both axes on both lattices (32 = 4 * 7 + 4,
30 = 4 * 7 + 2, 32 = 10 * 3 + 2), and a box row straddles each boundary of the three slabs (rows 11 and 22 of 32)."""
import ctypes

import numpy as np
import pytest

from test_gpu_forces import small

pytestmark = pytest.mark.gpu

LATTICES = [(32, 32), (30, 32)]
OWNERS = ["engine-1", "engine-3", "batch-3"]
EVERY = 2
KINDS = ["forces", "stats", "residuals", "profiles", "enstrophy", "psi_rows", "coarse_frames"]
BOX = (7, 3)


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
    elif kind == "enstrophy":
        o.set_enstrophy(every, capacity)
    elif kind == "psi_rows":
        o.set_psi(every, capacity)
    elif kind == "coarse_frames":
        o.set_coarse_frames(every, capacity, BOX)
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
            "residuals": fresh_rows(lbm, monkeypatch, owner, p, ob, cells, labels, "residuals", 12, [3]),
            "enstrophy": fresh_rows(lbm, monkeypatch, owner, p, ob, cells, labels, "enstrophy", 15, [3]),
            "psi_rows": fresh_rows(lbm, monkeypatch, owner, p, ob, cells, labels, "psi_rows", 18, [4]),
            "coarse_frames": fresh_rows(lbm, monkeypatch, owner, p, ob, cells, labels, "coarse_frames", 22, [3])}
    assert sorted(want) == sorted(KINDS)
    # six record sizes: per lattice 32 bytes of two bodies' forces, 56 of statistics, 40 of a residual row and of an
    # enstrophy row alike, 48 of a stream-function row, (32 + nx) * 48 of the profiles, 11 * 5 * 48 of a coarse frame
    assert len({len(next(iter(w.values()))) for w in want.values()}) == 6
    with make_owner(lbm, monkeypatch, owner, p, ob, cells) as o:
        arm(o, "stats", EVERY, 2, labels)
        o.run(3)                                              # records of steps 0 and 2: the ring is full
        steps, rows = read(o, "stats", 1)
        assert steps == [0] and rows[0] == want["stats"][0]
        o.run(2)                                              # step 4 goes into the slot that 0 left: the ring has wrapped
        steps, rows = read(o, "stats", 1)
        assert steps == [2] and rows[0] == want["stats"][2]
        arm(o, "stats", 0, 0, labels)                         # the record of step 4 goes unread
        for kind, calls, expect in (("profiles", [3], [6]), ("forces", [4], [8, 10]), ("residuals", [3], [12, 14]), ("enstrophy", [3], [16]),
                                    ("psi_rows", [4], [18, 20]), ("coarse_frames", [3], [22, 24])):
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
@pytest.mark.parametrize("kind", KINDS)
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
    """lbm_batch_set_forces refused for a blocked cell's label: lbm_batch_set_stats, and likewise every other kind's setter,
    then arms and records as on a fresh batch"""
    p, ob, cells, labels = case(lbm, 30, 32)
    bad = labels.copy()
    bad[1, 3] = 7
    for kind in KINDS:
        want = fresh_rows(lbm, monkeypatch, "batch-3", p, ob, cells, labels, kind, 2, [4])
        with make_owner(lbm, monkeypatch, "batch-3", p, ob, cells) as o:
            o.run(2)
            with pytest.raises(lbm.LbmError, match=r"lbm_batch_set_forces: member 1: the blocked cell \(3, 1\) has body 7, outside 0 \.\. 1"):
                o.set_forces(EVERY, 4, [labels, bad, labels], 2)
            assert [read(o, k)[0] for k in KINDS] == [[]] * len(KINDS)
            arm(o, kind, EVERY, 4, labels)
            o.run(4)
            steps, rows = read(o, kind)
            assert steps == [2, 4] == sorted(want) and rows == [want[2], want[4]], kind


# ---- the refusals every kind makes in the same words ------------------------------------------------------------------
# what differs between the kinds in those words: (setter's stem, reader's stem, the setter's own arguments behind
# `every, capacity` -- the forces' stand in front --, "<name> are armed", the short name, one record, the disarming
# call's arguments, "<...> armed on the batch")
WORDS = {
    "forces": ("set_forces", "read_forces", (), "obstacle forces", "forces", "row", "0, NULL, 0, 0", "the forces of a batch are"),
    "stats": ("set_stats", "read_stats", (), "lattice statistics", "statistics", "row", "0, 0", "the statistics of a batch are"),
    "residuals": ("set_residual", "read_residual", (), "velocity residuals", "residuals", "row", "0, 0", "the residuals of a batch are"),
    "profiles": ("set_profiles", "read_profiles", (3,), "line profiles", "profiles", "record", "0, 0, 0", "the profiles of a batch are"),
    "enstrophy": ("set_enstrophy", "read_enstrophy", (), "enstrophy rows", "enstrophy", "row", "0, 0", "the enstrophy of a batch is"),
    "psi_rows": ("set_psi", "read_psi_rows", (), "stream function rows", "the stream function", "row", "0, 0",
                 "the stream function of a batch is"),
    "coarse_frames": ("set_coarse_frames", "read_coarse_frames", BOX, "coarse frames", "coarse frames", "frame", "0, 0, 0, 0",
                      "the coarse frames of a batch are"),
}


def c_arm(o, prefix, kind, every, capacity, handle=None):
    """the kind's setter of the library itself, with arguments that are in order apart from `every` and `capacity`:
    (status, message)"""
    setter, own = WORDS[kind][0], WORDS[kind][2]
    fn = getattr(o.lib, prefix + setter)
    h = handle if handle is not None else o.handle
    status = fn(h, 1, None, every, capacity) if kind == "forces" else fn(h, every, capacity, *own)
    return status, o.lib.lbm_last_error().decode()


@pytest.mark.parametrize("owner", ["context", "batch"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_common_refusals_word_for_word(lbm, monkeypatch, kind, owner):
    p, ob, cells, labels = case(lbm, 30, 32)
    setter, reader, _, name, noun, record, off, of_a_batch = WORDS[kind]
    other = "enstrophy" if kind == "stats" else "stats"
    o_setter, _, _, o_name, _, _, o_off, _ = WORDS[other]
    batch = owner == "batch"
    prefix, handle_word = ("lbm_batch_", "batch") if batch else ("lbm_", "ctx")
    with make_owner(lbm, monkeypatch, "batch-3" if batch else "engine-1", p, ob, cells) as o:
        assert c_arm(o, prefix, kind, -1, 4) == (1, f"{prefix}{setter}: negative interval -1")
        assert c_arm(o, prefix, kind, 1, 0) == (1, f"{prefix}{setter}: capacity 0, at least one {record} is needed")
        # another kind armed on the same owner
        arm(o, other, EVERY, 4, labels)
        if batch:
            assert c_arm(o, prefix, kind, EVERY, 4) == (1, f"lbm_batch_{setter}: this batch has {o_name} armed (lbm_batch_{o_setter}); a batch "
                                                         f"records one kind -- disarm them with lbm_batch_{o_setter}(batch, {o_off}) first")
            assert c_arm(o, prefix, kind, 0, 0)[0] == 0       # disarming this kind leaves the other alone
        else:
            assert c_arm(o, prefix, kind, EVERY, 4) == (1, f"lbm_{setter}: {o_name} are armed (lbm_{o_setter}) and a context has one recorder -- "
                                                         f"disarm them with lbm_{o_setter}(ctx, {o_off}) first")
        arm(o, other, 0, 0, labels)
        if batch:
            m = o.member(1)
            m.set_mean(10)                                    # a member armed while the batch arms
            assert c_arm(o, prefix, kind, EVERY, 4) == (1, f"lbm_batch_{setter}: member 1 has mean fields armed (lbm_set_mean); a batch records one "
                                                         "kind -- disarm them with lbm_set_mean(ctx, 0) first")
            m.set_mean(0)
            assert c_arm(o, "lbm_", kind, EVERY, 4, m.handle) == (
                1, f"lbm_{setter}: not available on a member of a batch (lbm_create_batch): the batched launches need common sample steps to "
                f"end at, so {of_a_batch} armed on the batch, with one `every` for all members (lbm_batch_{setter})")
        else:
            o.set_halo_mode("stale")
            assert c_arm(o, prefix, kind, EVERY, 4) == (
                1, f"lbm_{setter}: the context runs the stale halo mode, where splitting a call at a {record} would change the results "
                f"(every call starts from freshly exchanged halos); {noun} need LBM_HALO_SYNC")
            o.set_halo_mode("sync")
        read_fn = getattr(o.lib, prefix + reader)
        n, steps, out = ctypes.c_int(-1), (ctypes.c_int * 4)(), (ctypes.c_double * 4096)()
        assert read_fn(o.handle, 1, None, steps, ctypes.byref(n)) == 1
        assert o.lib.lbm_last_error().decode() == f"{prefix}{reader}: NULL {record} output"
        assert read_fn(o.handle, -1, out, None, ctypes.byref(n)) == 1
        assert o.lib.lbm_last_error().decode() == f"{prefix}{reader}: negative max_{record}s -1"
        assert read(o, kind)[0] == [] and o.info()["steps_done"] == 0
        arm(o, kind, EVERY, 2, labels)                        # ... and after all that the kind arms
        assert read(o, kind)[0] == []


@pytest.mark.parametrize("owner", ["context", "batch"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_run_that_would_overflow_the_ring_is_refused(lbm, monkeypatch, kind, owner):
    p, ob, cells, labels = case(lbm, 30, 32)
    reader, record = WORDS[kind][1], WORDS[kind][5]
    run, prefix = ("lbm_batch_run", "lbm_batch_") if owner == "batch" else ("lbm_run", "lbm_")
    with make_owner(lbm, monkeypatch, "batch-3" if owner == "batch" else "engine-1", p, ob, cells) as o:
        arm(o, kind, EVERY, 2, labels)
        assert getattr(o.lib, run)(o.handle, 5) == 1          # it would record steps 0, 2 and 4
        assert o.lib.lbm_last_error().decode() == (f"{run}: 5 steps would record 3 {record}s, but the {record} buffer holds 2 and 0 {record}s are "
                                                   f"waiting ({prefix}{reader} drains them)")
        assert o.info()["steps_done"] == 0 and read(o, kind)[0] == []
