"""The refused lid acceleration and the edges of the exactness guards, on every kernel family: the lattices of
tests/edge_lattice.py (a lid row whose cells accept, refuse and half-refuse accelerate_flow before every step; cells at
2^-60, 2^60 and their predecessors, negative density, |u|^2 on both sides of 5e28, numerators below 2^-103, denormals -- at
every position of a four-cell lane, next to a blocked cell, on the lid row) run for 13 steps through each kernel and
compared with the CPU oracle bit for bit.  tests/test_edge_lattice.py shows, by the oracle alone, that the inputs reach
what they aim at.

Every case asserts through Engine.info() that the intended kernel served it.  av_vels is asserted finite only: the
multi-step and resident kernels take |u| from the pre-collision moments, which means nothing under the cancellation
these cells have."""
import numpy as np
import pytest

import double_model
import edge_lattice as el
import mean_model
import steady_model
import test_frames_format as frames_model
from fields_model import FIELDS, assert_field_frames

pytestmark = pytest.mark.gpu

STEPS = el.STEPS
CALLS = ([5, 8], [13])        # in pieces: the second call's first-step accelerate pass meets a mixed lattice too


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


_shared = {}


def reference(lbm, oracle, nx, ny, accel=el.ACCEL):
    """The lattice, the oracle's lattice and final_state after each of the 13 steps, its mean sums at every = 1; computed
    once per shape and never changed."""
    key = (nx, ny, accel)
    if key not in _shared:
        p, ob, cells, _ = el.build(lbm, nx, ny, accel=accel)
        ref, states, av = cells.copy(), {}, []
        for t in range(1, STEPS + 1):
            av.append(oracle.run(p, ref, ob, 1)[0])
            states[t] = oracle.final_state(p, ref, ob)
        _, sums, n = mean_model.oracle_sums(oracle, p, ob, cells, 0, STEPS, 1)
        assert np.isfinite(ref).all()
        for a in (ob, cells, ref, *sums.values(), *(f for s in states.values() for f in s.values())):
            a.setflags(write=False)
        _shared[key] = dict(p=p, ob=ob, cells=cells, ref=ref, states=states, sums=sums, n=n, av=np.array(av, dtype=np.float32))
    return _shared[key]


def assert_is_oracle(eng, want, what):
    assert eng.info()["steps_done"] == STEPS, what
    assert np.array_equal(bits(eng.cells()), bits(want["ref"])), f"{what}: lattice differs from the oracle"
    fields = eng.final_state()
    for k in FIELDS:
        assert np.array_equal(bits(fields[k]), bits(want["states"][STEPS][k])), f"{what}: {k} differs"
    assert np.isfinite(eng.av_vels(STEPS)).all(), what


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", el.KERNEL_CASES, ids=[c["id"] for c in el.KERNEL_CASES])
def test_kernel_matches_the_oracle(lbm, oracle, monkeypatch, case):
    setenv(monkeypatch, case["env"])
    want = reference(lbm, oracle, *case["shape"])
    for calls in CALLS:
        with lbm.Engine(want["p"], want["ob"], want["cells"], n_gpus=case["n_gpus"]) as eng:
            el.assert_pinned(eng.info(), case["pin"], case["id"])
            for n in calls:
                eng.run(n)
            assert_is_oracle(eng, want, f"{case['id']}, calls {calls}")


RESIDENT = {"LBM_RESIDENT_MIN_STEPS": "1"}
RECORDER_SHAPES = [{}, {"LBM_RESIDENT_ROWS": "4"}]       # the lid row in a two-row band, and in a four-row band


@pytest.mark.parametrize("env", RECORDER_SHAPES, ids=["rows2", "rows4"])
@pytest.mark.parametrize("recorder", ["frames", "field frames", "mean"])
def test_resident_deferred_acceleration(lbm, oracle, monkeypatch, recorder, env):
    """A step that is sampled defers the lid's acceleration behind the sample (resident_band: take_frame and its two
    twins).  Armed at every = 1 each of the three recorders must leave the lattice the oracle's and record the
    oracle's final_state of every step, bit for bit."""
    setenv(monkeypatch, {**RESIDENT, **env})
    want = reference(lbm, oracle, 256, 40)
    sample_steps = frames_model.frame_steps(0, STEPS, 1)
    for calls in CALLS:
        with lbm.Engine(want["p"], want["ob"], want["cells"]) as eng:
            info = eng.info()
            assert info["resident_steps"] > 0 and info["resident_rows"] == (4 if env else 2), info
            if recorder == "frames":
                eng.set_frames(1, STEPS + 1)
            elif recorder == "field frames":
                eng.set_field_frames(1, STEPS + 1, FIELDS, None)
            else:
                eng.set_mean(1)
            for n in calls:
                eng.run(n)
            assert_is_oracle(eng, want, f"{recorder}, calls {calls}")
            if recorder == "frames":
                steps, frames = eng.frames()
                assert steps.tolist() == sample_steps
                for i, tt in enumerate(sample_steps):
                    assert np.array_equal(bits(frames[i]), bits(want["states"][tt + 1]["u"])), f"frame tt={tt} differs"
            elif recorder == "field frames":
                steps, frames = eng.field_frames()
                assert_field_frames(steps, frames, {tt: want["states"][tt + 1] for tt in sample_steps})
            else:
                sums, n = eng.mean_sums()
                assert n == want["n"] == STEPS
                for k in FIELDS:
                    assert np.array_equal(bits(sums[k]), bits(want["sums"][k])), f"sum of {k} differs"


def test_resident_batch_members_have_their_own_threshold(lbm, oracle, monkeypatch):
    """Two members on the same ramp with accel 0.005 and 0.02: the refusal is decided with the member's own a1, a2."""
    setenv(monkeypatch, RESIDENT)
    members = [reference(lbm, oracle, 256, 40, accel) for accel in (el.ACCEL, 0.02)]
    for calls in CALLS:
        with lbm.Batch([m["p"] for m in members], [m["ob"] for m in members], [m["cells"] for m in members]) as batch:
            info = batch.info()
            assert info["members"] == 2 and info["resident_steps"] > 0 and info["resident_min_steps"] == 1, info
            for n in calls:
                batch.run(n)
            batch.sync()
            for i, m in enumerate(members):
                assert_is_oracle(batch.member(i), m, f"member {i}, calls {calls}")


@pytest.mark.parametrize("env", RECORDER_SHAPES, ids=["rows2", "rows4"])
def test_run_until_accelerates_like_run(lbm, oracle, monkeypatch, env):
    """A tolerance the series cannot meet, checked every 4 steps: three segments whose first-step acceleration goes through
    accelerate_row_unless (the second one issued before the first verdict is in), then the odd last step."""
    setenv(monkeypatch, {**RESIDENT, **env})
    want = reference(lbm, oracle, 256, 40)
    steady = dict(max_steps=STEPS, check_every=4, tol=1e-30, patience=1)
    model = steady_model.run_until(want["av"], **steady)
    assert not model["steady"] and min(model["rels"]) > 1e-3, model      # the oracle's series: 27 decades from tol
    with lbm.Engine(want["p"], want["ob"], want["cells"]) as eng:
        assert eng.info()["resident_steps"] > 0
        got = eng.run_until(**steady)
        assert (got["steps_run"], got["steady"], got["checks"]) == (STEPS, False, 2), got
        assert_is_oracle(eng, want, "run_until")


def test_double_engine_refusal(lbm):
    """The double engine's own copy of the condition: the ramp and the lid specials (its arithmetic has no guards),
    128 x 16, against the float64 model -- after the model has shown the lid row covered before every step."""
    nx, ny = 128, 16
    ob, start = el.build_double(nx, ny)
    a1, a2 = el.accel_terms(el.DENSITY, el.ACCEL, np.float64)
    ref = start.copy()
    for t in range(STEPS):
        el.assert_covered(el.coverage(ref[ny - 2], ob[ny - 2], a1, a2), ("double", t))
        double_model.timestep(ref, ob, el.DENSITY, el.ACCEL, el.OMEGA)
    assert np.isfinite(ref).all()
    final = double_model.final_state(ref, ob, el.DENSITY)
    p = lbm.ParamsDouble(nx, ny, STEPS, 10, el.DENSITY, el.ACCEL, el.OMEGA)
    for calls in CALLS:
        with lbm.DoubleEngine(p, ob, start) as eng:
            assert eng.info()["lane_cells"] == 2
            for n in calls:
                eng.run(n)
            assert eng.info()["steps_done"] == STEPS
            assert np.array_equal(bits(eng.cells()), bits(ref)), f"calls {calls}: lattice differs from the float64 model"
            got = eng.final_state()
            for k in FIELDS:
                assert np.array_equal(bits(got[k]), bits(final[k])), k
            assert np.isfinite(eng.av_vels()).all()


# ---- the one input that shows the |u|^2 guard: a quotient that overflows ---------------------------------------------
OVERFLOW_CASES = ["step_vec4 neigh0", "step_scalar 130x12", "step_scalar", "step_tile 16x8 x4", "step_tile 32x16 x3",
                  "step2_stream 4 cells", "step2_stream 2 cells", "stepk_stream K=2", "stepk_stream K=4",
                  "stepk_pk 1 pair K=2", "stepk_pk 1 pair K=3", "stepk_pk 2 pairs K=2 lds0 pf0 band2",
                  "stepk_pk 2 pairs K=2 lds1 pf1 band7", "stepk_pk 2 pairs K=4 lds2 pf1 band7", "2 slabs packed K=4",
                  "resident", "resident rows4 joint0", "resident rows4 joint1"]


def overflow_reference(lbm, oracle, nx, ny, when):
    key = ("overflow", nx, ny, when)
    if key not in _shared:
        p, ob, cells, placed = el.build_overflow(lbm, nx, ny, when)
        ref = cells.copy()
        oracle.run(p, ref, ob, when)
        assert not np.isnan(ref).any() and np.isposinf(ref).sum() == len(el.OVERFLOWS) * len(placed)
        state = oracle.final_state(p, ref, ob)
        for a in (ob, cells, ref, *state.values()):
            a.setflags(write=False)
        _shared[key] = dict(p=p, ob=ob, cells=cells, ref=ref, state=state)
    return _shared[key]


@pytest.mark.parametrize("when", [1, 2])
@pytest.mark.parametrize("name", OVERFLOW_CASES)
def test_overflowing_quotient_is_the_oracles_inf(lbm, oracle, monkeypatch, name, when):
    """|u|^2 = 8.5e37: (u_x^2) / (2 c_sq^2) overflows.  IEEE division gives +Inf, the fast constant divide would give NaN
    (Inf - Inf) -- the only finite input on which the |u|^2 < 5e28 guard shows (edge_lattice.build_overflow).  The cell
    meets its collision in the first step of a one-step call (when = 1: one-step kernels, the tile and the resident
    kernel) or in the second step of a two-step call (when = 2: one two-step pass of the stream kernels), after which
    the oracle's lattice holds +Inf but no NaN.  Lattice bit for bit; the fields wherever the oracle's are numbers, and NaN
    where they are not (the overflowed cells themselves)."""
    case = next(c for c in el.KERNEL_CASES if c["id"] == name)
    setenv(monkeypatch, case["env"])
    want = overflow_reference(lbm, oracle, *case["shape"], when)
    with lbm.Engine(want["p"], want["ob"], want["cells"], n_gpus=case["n_gpus"]) as eng:
        el.assert_pinned(eng.info(), case["pin"], name)
        eng.run(when)
        got, fields = eng.cells(), eng.final_state()
    assert not np.isnan(got).any(), "NaN where the oracle has +Inf or a number"
    assert np.array_equal(bits(got), bits(want["ref"]))
    for k in FIELDS:
        number = ~np.isnan(want["state"][k])
        assert np.array_equal(np.isnan(fields[k]), ~number), k
        assert np.array_equal(bits(fields[k])[number], bits(want["state"][k])[number]), k
