"""The tracers' rows in the ring the gather kinds share (Slab::gather_ring, lbm_batch::gather_ring), as
test_gpu_gather_ring.py and test_gpu_stress_ring.py ask of the kinds before it: armed after other kinds on one owner, every
row equals, byte for byte, the row of a fresh owner that armed only the tracers at the same step; a drain that crosses the
ring's end gives the rows of a ring that never wraps; a run that would overflow the ring is refused before any work; and
the refusals the setter and the reader share with every gather kind say, word for word, what every kind says.  Owners and
lattices are test_gpu_gather_ring's, without the context of three slabs: the tracers refuse it (test_gpu_tracers.py)."""
import ctypes

import numpy as np
import pytest

from test_gpu_gather_ring import EVERY, LATTICES, case, make_owner, read
from test_gpu_parity import random_case

pytestmark = pytest.mark.gpu

OWNERS = ["engine-1", "batch-3"]
KIND = "tracer_rows"
# (setter's stem, reader's stem, "<name> are armed", the short name, one record, the disarming call's arguments, "<...> armed on the batch")
SETTER, READER, NAME, NOUN, RECORD, OFF, OF_A_BATCH = ("set_tracers", "read_tracers", "tracer particles", "tracers", "row", "0, NULL, 0, 0",
                                                       "the tracers of a batch are")
N = 70                                                                # tracers per lattice: a row of 1120 bytes


def start(o, nx, ny):
    """the owner's start positions: other ones for every member"""
    members = len(o) if hasattr(o, "member") else 0
    xy = np.random.default_rng(nx).random((max(members, 1), N, 2)) * (nx, ny)
    return xy if members else xy[0]


def c_arm(o, prefix, every, capacity, xy, handle=None):
    """the library's own setter: (status, message)"""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    status = getattr(o.lib, prefix + SETTER)(handle if handle is not None else o.handle, N, xy.ctypes.data, every, capacity)
    return status, o.lib.lbm_last_error().decode()


def fresh_rows(lbm, monkeypatch, owner, p, ob, cells, first, calls):
    """{step: bytes} of an owner that ran `first` steps unarmed, armed only the tracers (a ring of 16: no wrap) and read all
    its rows in one go after `calls`"""
    with make_owner(lbm, monkeypatch, owner, p, ob, cells) as o:
        if first:
            o.run(first)
        o.set_tracers(start(o, p.nx, p.ny), EVERY, 16)
        for n in calls:
            o.run(n)
        steps, rows = read(o, KIND)
    assert len(steps) == len(set(steps)) > 0 and all(len(r) == len(rows[0]) > 0 for r in rows)
    return dict(zip(steps, rows))


@pytest.mark.parametrize("owner", OWNERS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_the_tracers_after_other_kinds_on_one_owner(lbm, monkeypatch, nx, ny, owner):
    """statistics (a smaller slot) wrap their ring and leave a row unread, the stress follows, then the tracers: their rows
    are a fresh owner's"""
    p, ob, cells, labels = case(lbm, nx, ny)
    want = fresh_rows(lbm, monkeypatch, owner, p, ob, cells, 8, [4])
    members = 3 if owner == "batch-3" else 1
    assert sorted(want) == [8, 10] and all(len(r) == 16 * N * members for r in want.values()) and want[8] != want[10]
    with make_owner(lbm, monkeypatch, owner, p, ob, cells) as o:
        o.set_stats(EVERY, 2)
        o.run(3)
        assert read(o, "stats", 1)[0] == [0]
        o.run(2)                                              # step 4 goes into the slot that 0 left: the ring has wrapped
        o.set_stats(0)                                        # the rows of steps 2 and 4 go unread
        o.set_stress(EVERY, 3)
        o.run(3)
        assert read(o, "stress_rows")[0] == [6]
        o.set_stress(0)
        o.set_tracers(start(o, nx, ny), EVERY, 3)
        o.run(4)
        steps, rows = read(o, KIND)
        assert steps == [8, 10] and rows == [want[8], want[10]]
        o.set_tracers(start(o, nx, ny), 0)
        o.set_stats(EVERY, 2)                                 # disarmed: the next kind arms
        o.set_stats(0)


@pytest.mark.parametrize("owner", OWNERS)
def test_a_drain_across_the_rings_end(lbm, monkeypatch, owner):
    """three slots, a row per step: after three steps and a read of two, two more steps put their rows into slots 0 and 1
    behind the one waiting in slot 2, and the read of everything runs over the ring's end"""
    p, ob, cells, labels = case(lbm, 30, 32)
    with make_owner(lbm, monkeypatch, owner, p, ob, cells) as o:
        o.set_tracers(start(o, 30, 32), 1, 16)
        o.run(3)
        o.run(2)
        want_steps, want = read(o, KIND)
    assert want_steps == [0, 1, 2, 3, 4] and len(set(want)) == 5
    with make_owner(lbm, monkeypatch, owner, p, ob, cells) as o:
        o.set_tracers(start(o, 30, 32), 1, 3)
        o.run(3)
        steps, rows = read(o, KIND, 2)
        assert steps == [0, 1] and rows == want[:2]
        o.run(2)
        steps, rows = read(o, KIND)
        assert steps == [2, 3, 4] and rows == want[2:]


@pytest.mark.parametrize("owner", ["context", "batch"])
def test_a_run_that_would_overflow_the_ring_is_refused(lbm, monkeypatch, owner):
    p, ob, cells, labels = case(lbm, 30, 32)
    run, prefix = ("lbm_batch_run", "lbm_batch_") if owner == "batch" else ("lbm_run", "lbm_")
    with make_owner(lbm, monkeypatch, "batch-3" if owner == "batch" else "engine-1", p, ob, cells) as o:
        o.set_tracers(start(o, 30, 32), EVERY, 2)
        assert getattr(o.lib, run)(o.handle, 5) == 1          # it would record steps 0, 2 and 4
        assert o.lib.lbm_last_error().decode() == (f"{run}: 5 steps would record 3 {RECORD}s, but the {RECORD} buffer holds 2 and 0 {RECORD}s are "
                                                   f"waiting ({prefix}{READER} drains them)")
        assert o.info()["steps_done"] == 0 and read(o, KIND)[0] == []
        o.run(3)                                              # steps 0 and 2: the ring is full
        assert getattr(o.lib, run)(o.handle, 2) == 1
        assert "2 rows are waiting" in o.lib.lbm_last_error().decode() and o.info()["steps_done"] == 3
        # without a ring no run lacks room, and the reader says why it has nothing
        o.set_tracers(start(o, 30, 32), EVERY, 0)
        o.run(9)
        n = ctypes.c_int(-1)
        assert getattr(o.lib, prefix + READER)(o.handle, 0, None, None, ctypes.byref(n)) == 1
        assert o.lib.lbm_last_error().decode() == f"{prefix}{READER}: {NAME} are armed without a ring (capacity 0): no {RECORD} is recorded"
        assert o.info()["steps_done"] == 12 and np.all(np.isfinite(o.tracers())) and not np.array_equal(o.tracers(), start(o, 30, 32))


@pytest.mark.parametrize("owner", ["context", "batch"])
def test_the_common_refusals_word_for_word(lbm, monkeypatch, owner):
    p, ob, cells, labels = case(lbm, 30, 32)
    batch = owner == "batch"
    prefix = "lbm_batch_" if batch else "lbm_"
    with make_owner(lbm, monkeypatch, "batch-3" if batch else "engine-1", p, ob, cells) as o:
        xy = start(o, 30, 32)
        assert c_arm(o, prefix, -1, 4, xy) == (1, f"{prefix}{SETTER}: negative interval -1")
        assert c_arm(o, prefix, 1, -1, xy) == (1, f"{prefix}{SETTER}: negative capacity -1 (0: no ring)")
        assert c_arm(o, prefix, 1, 2 ** 24, xy)[1].startswith(f"{prefix}{SETTER}: a ring of 16777216 {RECORD}s ")
        assert "2 GiB or more" in o.lib.lbm_last_error().decode()
        # another kind armed on the same owner, in both directions
        o.set_stats(EVERY, 4)
        if batch:
            assert c_arm(o, prefix, EVERY, 4, xy) == (1, f"lbm_batch_{SETTER}: this batch has lattice statistics armed (lbm_batch_set_stats); a batch "
                                                       "records one kind -- disarm them with lbm_batch_set_stats(batch, 0, 0) first")
            assert c_arm(o, prefix, 0, 0, xy)[0] == 0         # disarming this kind leaves the other alone
        else:
            assert c_arm(o, prefix, EVERY, 4, xy) == (1, f"lbm_{SETTER}: lattice statistics are armed (lbm_set_stats) and a context has one recorder -- "
                                                       "disarm them with lbm_set_stats(ctx, 0, 0) first")
        o.set_stats(0)
        o.set_tracers(xy, EVERY, 4)
        if batch:
            assert o.lib.lbm_batch_set_stats(o.handle, EVERY, 4) == 1
            assert o.lib.lbm_last_error().decode() == (f"lbm_batch_set_stats: this batch has {NAME} armed (lbm_batch_{SETTER}); a batch records one "
                                                       f"kind -- disarm them with lbm_batch_{SETTER}(batch, {OFF}) first")
            with pytest.raises(lbm.LbmError, match=r"this batch has %s armed \(lbm_batch_%s\)" % (NAME, SETTER)):
                o.member(1).set_frames(10, 2)                 # a kind a member may arm on its own
            with pytest.raises(lbm.LbmError, match="lbm_batch_run_until: %s are armed" % NAME):
                o.run_until(100, 10)
            with pytest.raises(lbm.LbmError, match="lbm_batch_run_until_residual: %s are armed" % NAME):
                o.run_until_residual(100, 10)
        else:
            assert o.lib.lbm_set_stats(o.handle, EVERY, 4) == 1
            assert o.lib.lbm_last_error().decode() == (f"lbm_set_stats: {NAME} are armed (lbm_{SETTER}) and a context has one recorder -- disarm "
                                                       f"them with lbm_{SETTER}(ctx, {OFF}) first")
            with pytest.raises(lbm.LbmError, match="lbm_run_until: %s are armed" % NAME):
                o.run_until(100, 10)
            with pytest.raises(lbm.LbmError, match="lbm_run_until_residual: %s are armed" % NAME):
                o.run_until_residual(100, 10)
            with pytest.raises(lbm.LbmError, match=r"lbm_set_halo_mode: %s are armed \(lbm_%s\)" % (NAME, SETTER)):
                o.set_halo_mode("stale")
        o.set_tracers(xy, 0)
        if batch:
            m = o.member(1)
            m.set_mean(10)                                    # a member armed while the batch arms
            assert c_arm(o, prefix, EVERY, 4, xy) == (1, f"lbm_batch_{SETTER}: member 1 has mean fields armed (lbm_set_mean); a batch records one "
                                                       "kind -- disarm them with lbm_set_mean(ctx, 0) first")
            m.set_mean(0)
            assert c_arm(o, "lbm_", EVERY, 4, xy[1], m.handle) == (
                1, f"lbm_{SETTER}: not available on a member of a batch (lbm_create_batch): the batched launches need common sample steps to "
                f"end at, so {OF_A_BATCH} armed on the batch, with one `every` for all members (lbm_batch_{SETTER})")
        else:
            for mode in ("stale", "freshest"):
                o.set_halo_mode(mode)
                assert c_arm(o, prefix, EVERY, 4, xy) == (
                    1, f"lbm_{SETTER}: the context runs the {mode} halo mode, where splitting a call at a {RECORD} would change the results "
                    f"(every call starts from freshly exchanged halos); {NOUN} need LBM_HALO_SYNC")
            o.set_halo_mode("sync")
        read_fn = getattr(o.lib, prefix + READER)
        n, steps, out = ctypes.c_int(-1), (ctypes.c_int * 4)(), (ctypes.c_double * 4096)()
        assert read_fn(o.handle, 1, None, steps, ctypes.byref(n)) == 1
        assert o.lib.lbm_last_error().decode() == f"{prefix}{READER}: NULL {RECORD} output"
        assert read_fn(o.handle, -1, out, None, ctypes.byref(n)) == 1
        assert o.lib.lbm_last_error().decode() == f"{prefix}{READER}: negative max_{RECORD}s -1"
        assert read(o, KIND)[0] == [] and o.info()["steps_done"] == 0
        o.set_tracers(xy, EVERY, 2)                           # ... and after all that the kind arms
        assert read(o, KIND)[0] == []


def test_rank_contexts_are_refused(lbm):
    """a rank context (one rank, host message passing that is never called)"""
    p, ob, cells = random_case(lbm, 128, 128, 4, walls=False)
    with lbm.Engine(p, ob, cells, rank=0, world_size=1, device=0, host_comm=(lambda plan, bufs: None, lambda v: None)) as eng:
        assert c_arm(eng, "lbm_", 10, 4, np.ones((N, 2))) == (
            1, f"lbm_{SETTER}: not available in a multi-process (rank) context: a tracer's cells would be spread over the ranks")
