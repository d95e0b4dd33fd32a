"""Steady-state runs (lbm_run_until / lbm_batch_run_until): the verdict is taken on the device after every check_every
steps.  Each run stops where tests/steady_model.py says it must -- computed from a plain run's av_vels (exact: same
kernels, deterministic sums) and from the oracle's series (tests/test_steady_model.py shows every decision of these
cases is a factor >= 3 from tol) -- and leaves exactly the lattice, av_vels and steps_done of lbm_run(steps_run).
"resident": 64x16, resident kernel, one segment of look-ahead (dropped after the stop); "per_pass": 100x16."""

import numpy as np
import pytest

import steady_model as sm
from cli_case import obstacles_text, params_text, run_cli
from test_gpu_parity import AV_RTOL

pytestmark = pytest.mark.gpu

# (shape, environment): the resident shape also with four-row bands
VARIANTS = [("resident", {}), ("resident", {"LBM_RESIDENT_ROWS": "4"}), ("per_pass", {})]
FIELDS = ("u_x", "u_y", "u", "pressure")


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def oracle_after(lbm, oracle, p, ob, n):
    cells = oracle.init_cells(p)
    av = oracle.run(p, cells, ob, n)
    return cells, av, oracle.final_state(p, cells, ob)


def assert_state_is_oracle(eng, oracle_state, steps):
    cells, _, fields = oracle_state
    assert eng.info()["steps_done"] == steps
    assert np.array_equal(eng.cells().view(np.uint32), cells.view(np.uint32))
    got = eng.final_state()
    for k in FIELDS:
        assert np.array_equal(got[k].view(np.uint32), fields[k].view(np.uint32)), k


def assert_result_is_model(got, want):
    for k in ("steps_run", "steady", "steady_step", "checks", "last_rel", "last_mean"):
        print(k, got[k], want[k])
    for k in ("steps_run", "steady", "steady_step", "checks", "last_rel", "last_mean"):
        assert got[k] == want[k], k


def check_path(eng, shape):
    info = eng.info()
    assert (info["resident_steps"] > 0) == (shape == "resident"), info
    if shape == "resident":
        assert info["resident_min_steps"] <= 512


@pytest.mark.parametrize("shape,env", VARIANTS)
def test_stops_where_the_model_says_and_goes_on(lbm, oracle, monkeypatch, shape, env):
    """Checks 1 - 3: the stop, the state after it, run(k) after it, a second call with its own segment count."""
    setenv(monkeypatch, env)
    p, ob = sm.case_params(lbm, shape)
    N = sm.STEADY["max_steps"]
    with lbm.Engine(p, ob) as plain, lbm.Engine(p, ob) as eng:
        check_path(eng, shape)
        plain.run(sm.CAPACITY)
        plain_av = plain.av_vels()
        got = eng.run_until(**sm.STEADY)
        want = sm.run_until(plain_av, **sm.STEADY)
        assert_result_is_model(got, want)
        _, oracle_av, _ = oracle_after(lbm, oracle, p, ob, N)
        from_oracle = sm.run_until(oracle_av, **sm.STEADY)
        assert (got["steps_run"], got["steady_step"], got["checks"]) == \
            (from_oracle["steps_run"], from_oracle["steady_step"], from_oracle["checks"]) == (2048, 2048, 3)
        steps = got["steps_run"]
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, steps), steps)
        av = eng.av_vels()
        assert av.size == steps and np.array_equal(av.view(np.uint32), plain_av[:steps].view(np.uint32))

        # going on: the dropped look-ahead segment left nothing behind
        eng.run(sm.GO_ON)
        steps += sm.GO_ON
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, steps), steps)
        # a second call counts its own segments
        # (its series is the engine's own: on the per-pass kernels the last bits of a step's sum depend on where the
        # passes of a call begin, and run(37) has moved that against the plain engine's single call)
        got2 = eng.run_until(**sm.SECOND)
        assert_result_is_model(got2, sm.run_until(eng.av_vels()[steps:], **sm.SECOND))
        want2 = sm.run_until(plain_av[steps:], **sm.SECOND)
        assert (got2["steps_run"], got2["steady_step"], got2["checks"]) == \
            (want2["steps_run"], want2["steady_step"], want2["checks"]) == (1536, 1536, 2)
        steps += got2["steps_run"]
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, steps), steps)
        av = eng.av_vels()
        assert av.size == steps
        np.testing.assert_allclose(av, plain_av[:steps], rtol=AV_RTOL)
        if shape == "resident":       # per-band sums: the same whatever the calls
            assert np.array_equal(av.view(np.uint32), plain_av[:steps].view(np.uint32))
        # and an ordinary run after that
        eng.run(20)
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, steps + 20), steps + 20)


@pytest.mark.parametrize("shape,env", VARIANTS)
def test_not_steady_runs_to_the_cap(lbm, oracle, monkeypatch, shape, env):
    """Check 4: a tol the series does not meet, max_steps not a multiple of check_every."""
    setenv(monkeypatch, env)
    p, ob = sm.case_params(lbm, shape)
    N = sm.NOT_STEADY["max_steps"]
    with lbm.Engine(p, ob) as plain, lbm.Engine(p, ob) as eng:
        plain.run(N)
        got = eng.run_until(**sm.NOT_STEADY)
        assert_result_is_model(got, sm.run_until(plain.av_vels(), **sm.NOT_STEADY))
        assert not got["steady"] and got["steps_run"] == N and got["steady_step"] == -1 and got["checks"] == 1
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, N), N)
        assert np.array_equal(eng.av_vels().view(np.uint32), plain.av_vels().view(np.uint32))


@pytest.mark.parametrize("shape,env", VARIANTS)
def test_every_segment_length_keeps_the_lattice(lbm, oracle, monkeypatch, shape, env):
    """Short segments (also below resident_min_steps) and a stop at the very first possible check (patience 1, a tol
    everything meets): the call ends after two segments although a third was already enqueued."""
    setenv(monkeypatch, env)
    p, ob = sm.case_params(lbm, shape)
    for E in (3, 50, 64):
        with lbm.Engine(p, ob) as eng:
            got = eng.run_until(10 * E, E, 1e30, 1)
            assert (got["steady"], got["steps_run"], got["steady_step"], got["checks"]) == (True, 2 * E, 2 * E, 1)
            assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, 2 * E), 2 * E)
            eng.run(E + 1)
            assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, 3 * E + 1), 3 * E + 1)
            assert eng.av_vels().size == 3 * E + 1


def test_long_segments_span_launches(lbm, oracle):
    """A segment longer than one resident launch (4096 steps) runs without look-ahead."""
    p, ob = sm.case_params(lbm, "resident")
    with lbm.Engine(p, ob) as eng:
        got = eng.run_until(8192, 4100, 1e30, 1)
        assert (got["steady"], got["steps_run"], got["checks"]) == (False, 8192, 0)
    with lbm.Engine(p, ob) as eng:
        got = eng.run_until(8192, 4000, 1e30, 1)
        assert (got["steady"], got["steps_run"], got["checks"]) == (True, 8000, 1)
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, 8000), 8000)


def test_batch_members_stop_at_their_own_checks(lbm, oracle):
    """Check 5: eight 64x16 members with different omega / accel."""
    made = [sm.case_params(lbm, "resident", omega, accel) for omega, accel in sm.BATCH]
    params, obstacles = [m[0] for m in made], [m[1] for m in made]
    N = sm.BATCH_STEADY["max_steps"]
    with lbm.Batch(params, obstacles) as plain, lbm.Batch(params, obstacles) as batch:
        assert batch.info()["resident_steps"] > 0
        plain.run(N)
        series = [plain.member(i).av_vels() for i in range(len(params))]
        got = batch.run_until(**sm.BATCH_STEADY)
        steps, want = sm.batch_run_until(series, **sm.BATCH_STEADY)
        assert steps == 2560 == max(g["steady_step"] for g in got)
        assert sorted(set(g["steady_step"] for g in got)) == [2048, 2560]
        assert batch.info()["steps_done"] == steps
        for i, (g, w) in enumerate(zip(got, want)):
            assert_result_is_model(g, w)
            m = batch.member(i)
            assert_state_is_oracle(m, oracle_after(lbm, oracle, params[i], obstacles[i], steps), steps)
            assert np.array_equal(m.av_vels().view(np.uint32), series[i][:steps].view(np.uint32))
        # not steady within the cap: all members run to it
        got = batch.run_until(1300, 512, 1e-12, 2)
        assert all(not g["steady"] and g["steps_run"] == 1300 and g["steady_step"] == -1 for g in got)
        steps += 1300
        for i in (0, 5):
            assert_state_is_oracle(batch.member(i), oracle_after(lbm, oracle, params[i], obstacles[i], steps), steps)


def test_batch_on_the_per_pass_kernels(lbm, oracle):
    made = [sm.case_params(lbm, "per_pass", omega, 0.005) for omega in (1.0, 0.8)]
    params, obstacles = [m[0] for m in made], [m[1] for m in made]
    with lbm.Batch(params, obstacles) as batch:
        assert batch.info()["resident_steps"] == 0
        got = batch.run_until(1000, 100, 1e30, 2)
        assert all(g["steady"] and g["steady_step"] == 300 and g["steps_run"] == 300 for g in got)
        for i in range(2):
            assert_state_is_oracle(batch.member(i), oracle_after(lbm, oracle, params[i], obstacles[i], 300), 300)


@pytest.mark.parametrize("shape", ["resident", "per_pass"])
def test_refusals_leave_the_context_usable(lbm, oracle, shape):
    """Check 6."""
    import ctypes
    p, ob = sm.case_params(lbm, shape)
    lib = lbm.load_library()
    res = lbm._CSteadyResult()

    def c_call(eng, max_steps, check_every, tol, patience):
        rc = lib.lbm_run_until(eng.handle, max_steps, check_every, ctypes.c_double(tol), patience, ctypes.byref(res))
        return rc, lib.lbm_last_error().decode()

    with lbm.Engine(p, ob) as eng:
        eng.run(10)
        for args, match in (((p.max_iters, 16, 1e-3, 2), "the av_vels record holds"), ((100, 0, 1e-3, 2), "check_every"),
                            ((100, 16, 1e-3, 0), "patience"), ((100, 16, -1.0, 2), "tol"),
                            ((100, 16, float("nan"), 2), "tol"), ((-1, 16, 1e-3, 2), "negative step count")):
            rc, err = c_call(eng, *args)
            assert rc != 0 and match in err, (args, err)
            assert eng.info()["steps_done"] == 10
        with pytest.raises(lbm.LbmError, match="the av_vels record holds"):
            eng.run_until(p.max_iters, 16)
        eng.set_frames(5, 4)
        with pytest.raises(lbm.LbmError, match="frames are armed"):
            eng.run_until(100, 16)
        eng.set_frames(0, 0)
        for mode in ("stale", "freshest"):
            eng.set_halo_mode(mode)
            with pytest.raises(lbm.LbmError, match="LBM_HALO_SYNC"):
                eng.run_until(100, 16)
        eng.set_halo_mode("sync")
        assert eng.info()["steps_done"] == 10
        got = eng.run_until(64, 16, 1e30, 1)
        assert got["steps_run"] == 32
        assert_state_is_oracle(eng, oracle_after(lbm, oracle, p, ob, 42), 42)


def test_refusals_of_slabs_ranks_and_members(lbm):
    p, ob = sm.case_params(lbm, "resident")
    with lbm.Engine(p, ob, n_gpus=2) as eng:
        with pytest.raises(lbm.LbmError, match="slabs"):
            eng.run_until(100, 16)
        assert eng.info()["steps_done"] == 0
        eng.run(5)
    calls = ([], [])
    comm = (lambda plan, views: calls[0].append(1), lambda values: calls[1].append(1))
    with lbm.Engine(p, ob, rank=0, world_size=1, host_comm=comm) as eng:
        with pytest.raises(lbm.LbmError, match="multi-process"):
            eng.run_until(100, 16)
        assert eng.info()["steps_done"] == 0
    with lbm.Batch([p, p], [ob, ob]) as batch:
        import ctypes
        lib = lbm.load_library()
        res = lbm._CSteadyResult()
        assert lib.lbm_run_until(batch.member(1).handle, 100, 16, ctypes.c_double(1e-3), 2, ctypes.byref(res)) != 0
        assert "member of a batch" in lib.lbm_last_error().decode()
        with pytest.raises(lbm.LbmError, match="member of a batch"):
            batch.member(1).run_until(100, 16)
        batch.member(0).set_frames(10, 4)
        with pytest.raises(lbm.LbmError, match="frames are armed"):
            batch.run_until(100, 16)
        with pytest.raises(lbm.LbmError, match="the av_vels record holds"):
            batch.run_until(p.max_iters + 1, 16)
        assert batch.info()["steps_done"] == 0
        batch.member(0).set_frames(0, 0)
        assert batch.run_until(64, 16, 1e30, 1)[1]["steps_run"] == 32


def test_cli_runs_to_the_steady_state(lbm, oracle, tmp_path):
    """Check 7: LBM_STEADY=1e-3:512:2 on the 64x16 case; without the variable the program runs maxIters steps as ever."""
    p, ob = sm.case_params(lbm, "resident")
    p.max_iters = 4096
    want_steps = {"steady": 2048, "plain": 4096}
    for label, env in (("steady", {"LBM_STEADY": "1e-3:512:2"}), ("plain", {})):
        out = run_cli(lbm, tmp_path / label, params_text(p), obstacles_text(ob), **env)
        assert out.returncode == 0, out.stderr
        stdout = out.stdout
        n = want_steps[label]
        cells, av, fields = oracle_after(lbm, oracle, p, ob, n)
        twin = tmp_path / (label + "_final_state.dat")
        lbm.write_final_state(str(twin), fields, ob)
        assert (tmp_path / label / "final_state.dat").read_bytes() == twin.read_bytes()
        lines = (tmp_path / label / "av_vels.dat").read_text().splitlines()
        assert len(lines) == n and lines[-1].startswith("%d:\t" % (n - 1))
        steady_lines = [l for l in stdout.splitlines() if "teady after" in l]
        if label == "steady":
            assert len(steady_lines) == 1 and steady_lines[0].startswith("Steady after 2048 steps (rel. change ")
            assert stdout.index(steady_lines[0]) < stdout.index("==done==")
        else:
            assert steady_lines == []
            assert stdout.startswith("==done==\n")
    # the cap: not steady within maxIters
    p.max_iters = 1300
    out = run_cli(lbm, tmp_path / "cap", params_text(p), obstacles_text(ob), LBM_STEADY="1e-9:512")
    assert out.returncode == 0, out.stderr
    stdout = out.stdout
    assert "Not steady after 1300 steps (rel. change " in stdout
    assert len((tmp_path / "cap" / "av_vels.dat").read_text().splitlines()) == 1300
