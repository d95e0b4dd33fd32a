"""Every fast-math kernel (math="fast"), pinned bit for bit to the oracle's fast collision.

The fast kernels all relax a cell through the one collide<false> (lbm_kernels.hip.h:279-306).  oracle/lbm_oracle.c restates
it operation for operation (held to the rational BGK collision by tests/test_fast_model.py), so a fast lattice has one
right answer bit for bit, from every kernel family and every call splitting.  The cases (tests/fast_model.py: CASES) name
every row of the fast dispatch tables of lbm_hip.hip; each asserts through Engine.info() that its kernel was selected, runs
its calls in one piece and split, and checks

* the lattice: cells() bit-identical to Oracle.run_fast;
* the fields: final_state() bit-identical to the oracle's final_state of that lattice (the reader has one arithmetic);
* av_vels: every step within (depth + 2) 2^-24 + 2^-23 relative (+ 2^-63) of the float64 mean over the fluid cells of
  sqrt(u_sq) from the model's map -- in fast mode every family takes |u| from the pre-collision moments with the
  native sqrt (s = 1).  Each case prints its largest error / bound; the figure never feeds back into the bound.
"""
import numpy as np
import pytest

import av_model
import fast_model
from av_model import FLUSH_ALLOWANCE, U
from fast_model import CASES

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_selected(expect, slabs, info):
    for key, want in expect.items():
        if key == "resident_steps":
            assert (info[key] > 0) == (want > 0), (key, info)
        else:
            assert info[key] == want, (key, info)
    assert info["n_slabs"] == slabs
    assert info["math_mode"] == 1                       # LBM_MATH_FAST


def run_fast_engine(lbm, p, ob, cells, calls, expect, slabs=1):
    with lbm.Engine(p, ob, cells.copy(), n_gpus=slabs, math="fast") as eng:
        info = eng.info()
        assert_selected(expect, slabs, info)
        for n in calls:
            eng.run(n)
        return info, eng.cells(), eng.av_vels(sum(calls)).astype(np.float64), eng.final_state()


def check_av(case, info, ob, usq, got_av, what):
    assert av_model.speed_mode(info, fast=True) == 1
    bound = case.bound(info)
    assert bound == case.bound()                        # the bound the CPU checks were made with
    want = np.array([fast_model.want_av(m, ob) for m in usq])
    err = np.abs(got_av - want)
    allowed = bound * want + FLUSH_ALLOWANCE
    print(f"fast_av_ratio {case.id} {what}: bound {bound / U:.0f} u, largest error / bound {float(np.max(err / allowed)):.3f} "
          f"at step {int(np.argmax(err / allowed))}")
    bad = np.nonzero(err > allowed)[0]
    assert len(bad) == 0, (f"{case.id} {what}: av_vels off the float64 mean of sqrt(u_sq) by more than {bound:.3e} relative "
                           f"at steps {bad[:16].tolist()}: {(err / want)[bad[:16]].tolist()}")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_fast_kernel_is_the_oracles_fast_collision(lbm, oracle, monkeypatch, case):
    for key, value in case.env.items():
        monkeypatch.setenv(key, value)
    p, ob, cells = av_model.lattice(case.nx, case.ny)
    want = fast_model.model(case.nx, case.ny, case.steps)
    want_fields = oracle.final_state(p, want.cells, ob)
    for calls in case.calls:
        info, got_cells, got_av, fields = run_fast_engine(lbm, p, ob, cells, calls, case.expect, case.slabs)
        differ = int((bits(got_cells) != bits(want.cells)).sum())
        assert differ == 0, f"{case.id} {list(calls)}: {differ} populations differ from the oracle's fast run"
        for k in ("u_x", "u_y", "u", "pressure"):
            assert np.array_equal(bits(fields[k]), bits(want_fields[k])), (case.id, list(calls), k)
        check_av(case, info, ob, want.usq, got_av, list(calls))


def test_fast_is_not_exact_on_the_gpu(lbm, oracle, monkeypatch):
    """The mode was really on: the fast lattice of the 320x12 case differs from the exact oracle's."""
    case = CASES[0]
    assert (case.nx, case.ny) == (320, 12)
    for key, value in case.env.items():
        monkeypatch.setenv(key, value)
    p, ob, cells = av_model.lattice(case.nx, case.ny)
    _, got_cells, _, _ = run_fast_engine(lbm, p, ob, cells, (13,), case.expect)
    exact = cells.copy()
    oracle.run(p, exact, ob, 13)
    assert not np.array_equal(bits(got_cells), bits(exact))
    assert np.array_equal(bits(got_cells), bits(fast_model.model(case.nx, case.ny, 13).cells))


def test_default_packed_plan_in_fast_mode(lbm, oracle, monkeypatch):
    """The packed stream kernels have one arithmetic, the exact one, and serve both modes (lbm_hip.hip:729): twelve steps
    of four-step passes in fast mode are bit-identical to the EXACT oracle.  A thirteenth step, in a second call, is one
    launch of step_vec4<1> (launch_step, :616-628): twelve exact steps followed by one fast step.  A single call of 13
    steps is issued the same way -- run_passes (:1609-1612) runs pass_steps per pass while that many remain and the odd
    last step through launch_step -- so it must give the same lattice."""
    for key, value in fast_model.PACKED_ENV.items():
        monkeypatch.setenv(key, value)
    nx, ny = fast_model.PACKED_SHAPE
    p, ob, cells = av_model.lattice(nx, ny)
    twelve = cells.copy()
    oracle.run(p, twelve, ob, 12)
    thirteen = twelve.copy()
    oracle.run_fast(p, thirteen, ob, 1)
    with lbm.Engine(p, ob, cells.copy(), math="fast") as eng:
        assert_selected(fast_model.PACKED_EXPECT, 1, eng.info())
        eng.run(12)
        assert np.array_equal(bits(eng.cells()), bits(twelve))
        eng.run(1)
        assert np.array_equal(bits(eng.cells()), bits(thirteen))
    _, got, _, _ = run_fast_engine(lbm, p, ob, cells, (13,), fast_model.PACKED_EXPECT)
    assert np.array_equal(bits(got), bits(thirteen))
    exact13 = twelve.copy()
    oracle.run(p, exact13, ob, 1)
    assert not np.array_equal(bits(thirteen), bits(exact13))
