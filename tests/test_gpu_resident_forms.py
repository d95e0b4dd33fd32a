"""Every one of the resident kernel's 50 forms -- 2 (BATCH) x 5 (REC) x 5 shapes of lbm::resident_band -- launched against
the oracle.  tests/resident_forms.py holds the cases; tests/test_resident_forms.py shows on the CPU, from the planner, that
each case launches the form it claims.  Here every case runs calls of 1, 2, 19 and 5 steps and is compared as bit
patterns, without tolerances:

* the lattice with the oracle's, and with the same engine or batch run unarmed;
* av_vels with the unarmed run's (the plain forms: with the derived bound of tests/av_model.py);
* every record with the model of its kind -- frames: the oracle's final_state u (test_gpu_frames.oracle_frames); probes:
  final_state at the cell (test_gpu_probes.oracle_series); mean fields: the float64 loops of tests/mean_model.py and
  tests/moments_model.py; field frames: tests/fields_model.py;
* a batch arms its first member (every 3) and its last (every 4, another ring size) and leaves the one between unarmed:
  that one records nothing and equals a single Engine; in the two-launch cases the last member runs in the second launch
  of the chunk and gives exactly the records of a single Engine armed alike.
"""
import numpy as np
import pytest

import av_model
import mean_model
import moments_model
import resident_forms as rf
from fields_model import FIELDS, assert_field_frames, oracle_field_frames
from test_gpu_frames import assert_frames, oracle_frames
from test_gpu_mean import assert_sums
from test_gpu_moments import assert_sums2
from test_gpu_probes import assert_series, oracle_series

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Shared:
    """Oracle runs and unarmed engine runs, computed once per lattice (and recorder request) and shared by the cases of
    that lattice; nothing changes them."""
    cache = {}

    @classmethod
    def get(cls, key, make):
        if key not in cls.cache:
            cls.cache[key] = make()
        return cls.cache[key]


@pytest.fixture(scope="module")
def cus():
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert n == rf.CUS, (f"the device reports {n} CUs; the cases of tests/resident_forms.py are planned for {rf.CUS} "
                         "(tests/test_resident_forms.py), so they would launch other forms here")
    return n


# ---------------------------------------------------------------------------------------------------------------------
# one recorder request: arm, drain after every call, the model's answer, the comparison
# ---------------------------------------------------------------------------------------------------------------------
class Request:
    def __init__(self, rec, every, capacity=0, probes=None, order=1, fields=FIELDS, window=None, name=""):
        self.rec, self.every, self.capacity, self.order, self.fields, self.window = rec, every, capacity, order, tuple(fields), window
        self.probes = None if probes is None else tuple(probes)
        self.name = name

    def key(self):
        return (self.rec, self.every, self.probes, self.order if self.rec == "mean" else 0, self.fields, self.window)

    def arm(self, eng):
        if self.rec == "frames":
            eng.set_frames(self.every, self.capacity)
        elif self.rec == "probes":
            eng.set_probes(list(self.probes), self.every, self.capacity)
        elif self.rec == "mean":
            eng.set_mean_order(self.every, self.order)
        else:
            eng.set_field_frames(self.every, self.capacity, self.fields, self.window)

    def drain(self, eng, acc):
        """After every call; the mean fields accumulate and are read at the end."""
        if self.rec == "frames":
            acc.append(eng.frames())
        elif self.rec == "probes":
            acc.append(eng.probes())
        elif self.rec == "fields":
            acc.append(eng.field_frames())

    def records(self, eng, acc):
        if self.rec == "mean":
            sums, n = eng.mean_sums()
            sums2, n2 = eng.moment_sums() if self.order == 2 else (None, n)
            assert n2 == n
            return sums, sums2, n
        steps = np.concatenate([s for s, _ in acc])
        if self.rec == "fields":
            return steps, {k: np.concatenate([f[k] for _, f in acc]) for k in acc[0][1]}
        return steps, np.concatenate([v for _, v in acc])

    def want(self, oracle, case, member):
        p, ob, cells = rf.inputs(case, member)

        def make():
            if self.rec == "frames":
                return oracle_frames(oracle, p, ob, cells, 0, rf.STEPS, self.every)
            if self.rec == "probes":
                return oracle_series(oracle, p, ob, cells, 0, rf.STEPS, self.every, self.probes)
            if self.rec == "mean":
                ref, sums, sums2, n = moments_model.oracle_sums2(oracle, p, ob, cells, 0, rf.STEPS, self.every)
                ref1, sums1, n1 = mean_model.oracle_sums(oracle, p, ob, cells, 0, rf.STEPS, self.every)
                assert n == n1 and np.array_equal(ref, ref1) and all(np.array_equal(sums[k], sums1[k]) for k in sums1)
                return ref, (sums, sums2, n)
            return oracle_field_frames(oracle, p, ob, cells, 0, rf.STEPS, self.every, self.fields, self.window)
        ref, want = Shared.get(("want", case.nx, case.ny, case.members, member) + self.key(), make)
        assert np.array_equal(bits(ref), bits(rf.model(case, member)[0]))
        return want

    def check(self, got, want, what):
        if self.rec == "frames":
            assert_frames(got[0], got[1], want)
        elif self.rec == "probes":
            assert got[0].tolist() == list(range(0, rf.STEPS, self.every)), what
            assert_series(got[0], got[1], want)
        elif self.rec == "mean":
            sums, sums2, n = got
            assert_sums(sums, n, want[0], want[2], what)
            if self.order == 2:
                assert_sums2(sums2, n, want[1], want[2], what)
        else:
            assert_field_frames(got[0], got[1], want, self.fields)

    def same(self, got, other, what):
        """Two engines' records of this request, bit for bit."""
        if self.rec == "mean":
            assert got[2] == other[2], what
            for a, b in ((got[0], other[0]), (got[1] or {}, other[1] or {})):
                assert list(a) == list(b) and all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in a), what
        elif self.rec == "fields":
            assert got[0].tolist() == other[0].tolist() and list(got[1]) == list(other[1]), what
            assert all(np.array_equal(bits(got[1][k]), bits(other[1][k])) for k in got[1]), what
        else:
            assert got[0].tolist() == other[0].tolist() and np.array_equal(bits(got[1]), bits(other[1])), what

    def nothing_recorded(self, eng):
        if self.rec == "frames":
            assert eng.frames()[0].size == 0
        elif self.rec == "probes":
            assert eng.probes()[0].size == 0
        elif self.rec == "fields":
            assert eng.field_frames()[0].size == 0
        else:
            with pytest.raises(Exception, match="not armed"):
                eng.mean_sums()


def requests(case):
    """The rounds of a case: each a pair (the first armed member's request, the second's).  A single engine runs every
    request of every round; the two-launch cases run the first round."""
    (e0, e1), (c0, c1), (pc0, pc1) = rf.EVERY, rf.CAPACITY, rf.PROBE_CAPACITY
    rec, nx, ny = case.rec, case.nx, case.ny
    if rec == "frames":
        rounds = [(Request(rec, e0, c0), Request(rec, e1, c1))]
    elif rec == "probes":
        lid, off = rf.probe_sets(nx, ny)
        rounds = [(Request(rec, e0, c0, probes=lid, name="lid"), Request(rec, e1, c1, probes=off, name="off-lid")),
                  (Request(rec, 1, pc0, probes=off, name="off-lid"), Request(rec, e1, pc1, probes=lid, name="lid"))]
    elif rec == "mean":
        rounds = [(Request(rec, e0, order=1), Request(rec, e1, order=2)), (Request(rec, e0, order=2), Request(rec, e1, order=1))]
    else:
        w = rf.field_windows(nx, ny)
        rounds = [(Request(rec, e0, c0, window=w["whole"], name="whole"), Request(rec, e1, c1, window=w["lid-seam"], name="lid-seam")),
                  (Request(rec, e0, c0, window=w["rows-1-2"], name="rows-1-2"),
                   Request(rec, e1, c1, fields=rf.SUBSET, window=w["subset"], name="subset")),
                  (Request(rec, e0, c0, window=w["lid-seam"], name="lid-seam"), Request(rec, e1, c1, window=w["rows-1-2"], name="rows-1-2"))]
    return rounds[:1] if case.kind == "two-launch" else rounds


# ---------------------------------------------------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------------------------------------------------
def check_info(info, case):
    assert info["resident_steps"] > 0 and info["resident_min_steps"] == 1, info
    assert {k: info[k] for k in case.expect} == case.expect, info


def run_single(lbm, case, member, request=None):
    """One Engine on a member's inputs through CALLS: (lattice, av_vels, records, info)."""
    p, ob, cells = rf.inputs(case, member)
    acc = []
    with lbm.Engine(p, ob, cells) as eng:
        if request:
            request.arm(eng)
        for n in rf.CALLS:
            eng.run(n)
            if request:
                request.drain(eng, acc)
        return eng.cells(), eng.av_vels(rf.STEPS), request.records(eng, acc) if request else None, eng.info()


def single_unarmed(lbm, case, member):
    return Shared.get(("single", case.geometry, case.members, member), lambda: run_single(lbm, case, member))


def run_batch(lbm, case, armed=None):
    """One Batch through CALLS, `armed`: {member: request}.  ({member: (lattice, av_vels, records)}, member 0's info,
    Batch.info()); the members without a request must have recorded nothing."""
    params, obstacles, cells = rf.member_inputs(case.nx, case.ny, case.members)
    armed = armed or {}
    acc = {i: [] for i in armed}
    with lbm.Batch(params, obstacles, cells) as batch:
        for i, request in armed.items():
            request.arm(batch.member(i))
        for n in rf.CALLS:
            batch.run(n)
            for i, request in armed.items():
                request.drain(batch.member(i), acc[i])
        out = {}
        for i in range(case.members):
            m = batch.member(i)
            out[i] = (m.cells(), m.av_vels(rf.STEPS), armed[i].records(m, acc[i]) if i in armed else None)
            if armed and i not in armed:
                next(iter(armed.values())).nothing_recorded(m)
        return out, batch.member(0).info(), batch.info()


def check_av_bound(av, info, ob, moment, what):
    """The plain forms: every step's av_vels against the float64 sum of the per-cell values the kernel adds."""
    bound = av_model.bound(info)
    want = np.array([av_model.want_av(m, ob) for m in moment])
    err = np.abs(np.asarray(av, dtype=np.float64) - want)
    bad = np.nonzero(err > bound * want + av_model.FLUSH_ALLOWANCE)[0]
    assert len(bad) == 0, f"{what}: av_vels off by more than {bound:.3e} relative at steps {bad.tolist()}"


def check_single(lbm, oracle, case):
    ref, moment = rf.model(case)
    base, base_av, _, info = single_unarmed(lbm, case, 0)
    check_info(info, case)
    assert np.array_equal(bits(ref), bits(base)), "the unarmed lattice differs from the oracle's"
    if case.rec == "none":
        check_av_bound(base_av, info, rf.inputs(case)[1], moment, case.id)
        return
    for round_ in requests(case):
        for request in round_:
            what = f"{case.id} {request.name} every {request.every}"
            got, av, records, info = run_single(lbm, case, 0, request)
            check_info(info, case)
            request.check(records, request.want(oracle, case, 0), what)
            assert np.array_equal(bits(ref), bits(got)), f"{what}: the lattice differs from the oracle's"
            assert np.array_equal(bits(base_av), bits(av)), f"{what}: recording changed av_vels"


def check_batch(lbm, oracle, case):
    plain, info, binfo = Shared.get(("batch", case.geometry, case.members), lambda: run_batch(lbm, case))
    check_info(info, case)
    assert binfo["members"] == case.members and binfo["resident_steps"] > 0
    assert (binfo["members_per_launch"], binfo["launches_per_chunk"]) == (case.per_launch, case.launches), binfo
    if case.kind == "two-launch":
        assert binfo["launches_per_chunk"] == 2 and case.armed[1] >= binfo["members_per_launch"]
    for i in range(case.members):
        assert np.array_equal(bits(rf.model(case, i)[0]), bits(plain[i][0])), f"member {i}: the unarmed lattice differs from the oracle's"
    for i in (case.unarmed if case.rec != "none" else range(case.members)):       # ... equal a single Engine's
        one, one_av, _, one_info = single_unarmed(lbm, case, i)
        check_info(one_info, case)
        assert np.array_equal(bits(one), bits(plain[i][0])) and np.array_equal(bits(one_av), bits(plain[i][1])), f"member {i}"
    if case.rec == "none":
        for i in range(case.members):
            check_av_bound(plain[i][1], info, rf.inputs(case, i)[1], rf.model(case, i)[1], f"{case.id} member {i}")
        return
    for round_ in requests(case):
        armed = dict(zip(case.armed, round_))
        got, info, binfo = run_batch(lbm, case, armed)                 # (the members between record nothing: run_batch)
        check_info(info, case)
        for i in range(case.members):
            assert np.array_equal(bits(plain[i][0]), bits(got[i][0])), f"member {i}: recording changed the lattice"
            assert np.array_equal(bits(plain[i][1]), bits(got[i][1])), f"member {i}: recording changed av_vels"
        for i, request in armed.items():
            what = f"{case.id} member {i} {request.name} every {request.every}"
            request.check(got[i][2], request.want(oracle, case, i), what)
            if case.kind == "two-launch":
                one, one_av, one_records, _ = run_single(lbm, case, i, request)
                request.same(got[i][2], one_records, what + ": the batch member's records differ from a single Engine's")
                assert np.array_equal(bits(one), bits(got[i][0])) and np.array_equal(bits(one_av), bits(got[i][1])), what


@pytest.mark.parametrize("case", rf.CASES, ids=lambda c: c.id)
def test_form_against_the_oracle(lbm, oracle, monkeypatch, cus, case):
    """One form of lbm::resident_band (tests/resident_forms.py names which, tests/test_resident_forms.py proves it): the
    lattice, av_vels and every record of every armed engine or member, bit for bit."""
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if case.batch:
        check_batch(lbm, oracle, case)
    else:
        check_single(lbm, oracle, case)
