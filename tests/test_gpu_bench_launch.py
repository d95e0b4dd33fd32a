"""First contact with a multi-GPU node, rehearsed on the one-GPU box: bench.py launches its own
ranks as a child process, the record says which RCCL served the run and how many ranks it saw, an over-subscribed
launch fails fast, and the RCCL self-exchange is bit-exact under both libraries a process can end up with."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def run_bench(args, env_extra, timeout):
    env = dict(os.environ, LBM_BENCH_ALSO="0", LBM_BENCH_REPEATS="1", LBM_BENCH_PREWARM_S="0", **env_extra)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--no-cpu-baseline"], env=env,
                         capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    return out, time.time() - t0


def test_bench_launches_its_own_ranks_and_reports_rccl():
    """`python bench.py --gpus 1` through the child-launch path (torch.distributed.run started by bench.py itself):
    exactly one JSON line, a communicator of one rank, library and version named."""
    out, _ = run_bench(["--gpus", "1", "--steps", "8", "--warmup", "4", "--grid", "2048x2048"],
                       {"LBM_BENCH_SELF_LAUNCH": "1"}, 400)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["results_finite"]
    rc = line["rccl"]
    assert rc["loaded"] and rc["nranks"] == 1 and rc["rank"] == 0 and rc["n_comms"] == 1
    assert rc["nranks_min_over_ranks"] == rc["nranks_max_over_ranks"] == 1
    assert rc["version"] >= 22000 and "librccl" in rc["library"]
    assert "rank API" in line["config"]["decomposition"]


def test_bench_oversubscribed_launch_fails_fast(lbm):
    """`python bench.py --gpus 2` on a one-GPU box: non-zero exit, no JSON line, no hang."""
    if lbm.device_count() >= 2:
        pytest.skip("needs a box with a single GPU")
    out, secs = run_bench(["--gpus", "2", "--steps", "4", "--warmup", "2", "--grid", "1024x1024"], {}, 300)
    assert out.returncode != 0
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert "needs 2 devices" in out.stderr
    assert "LBM_THREADS=0" in out.stderr          # the failure message names the single-thread override
    assert secs < 180


@pytest.mark.parametrize("ranks", [2, 3])
def test_bench_multi_rank_path_rehearsed_on_one_gpu(ranks):
    """`python bench.py --gpus N` with N ranks sharing the one GPU and their halo rows travelling through the host
    (LBM_BENCH_REHEARSAL=hosted): the launch by bench.py itself, the agreement of the ranks on step counts, the
    max-over-ranks timing, the bitwise self-check against a single-GPU run and the exit status -- every line of the
    multi-rank path of bench.py except the RCCL transport -- run before the first real multi-GPU node sees them."""
    out, _ = run_bench(["--gpus", str(ranks), "--steps", "8", "--warmup", "4", "--grid", "2048x1536", "--full"],
                       {"LBM_BENCH_REHEARSAL": "hosted"}, 600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == ranks and line["results_finite"]
    assert "REHEARSAL" in line["config"]["decomposition"]
    chk = line["multi_gpu_check"]
    assert chk["fields_bitwise_equal_to_single_gpu_run"] is True and chk["ranks_checked"] == ranks, chk
    assert chk["av_vels_max_rel_diff"] < 1e-4


@pytest.mark.parametrize("torch_first,forced", [(False, None), (True, None), (True, "/opt/rocm/lib/librccl.so.1")])
def test_rccl_self_exchange_under_both_libraries(torch_first, forced):
    """The engine binds the librccl already in the process (torch's bundled one when torch was imported first -- the
    situation of bench.py and of this test suite) or ROCm's own (the C host program), or the file LBM_RCCL_LIB names
    (here: ROCm's next to torch's HIP runtime): the ring of one must be bit-identical to the plain periodic run under
    each, and the record must name the library."""
    env = dict(os.environ)
    env.pop("LBM_RCCL_LIB", None)
    if forced:
        if not os.path.exists(forced):
            pytest.skip(f"{forced} not present")
        env["LBM_RCCL_LIB"] = forced
    cmd = [sys.executable, os.path.join(ROOT, "tools", "rccl_self.py")] + (["--torch-first"] if torch_first else [])
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["fields_equal"], rec
    assert not rec["single_slab_loaded_rccl"]                     # a single slab binds no RCCL
    rc = rec["rccl"]
    assert rc["loaded"] and rc["nranks"] == 1 and rc["n_comms"] == 1
    if torch_first and not forced:
        assert "/torch/lib/" in rc["library"], rc
    else:
        assert rc["library"].startswith("/opt/rocm"), rc
    # one RCCL per process unless a second one was asked for by name
    assert len([m for m in rec["mapped"] if "librccl" in m]) == (2 if forced else 1), rec["mapped"]


def test_bench_dump_outputs_repeat_exactly(lbm, tmp_path):
    """`bench.py --dump-outputs DIR`: a plain run times exactly --steps steps and writes the headline's results after its
    last timed step -- float32, within 64 MB, bit-identical from run to run with the same arguments; the sampled
    lattice and the sampled final-state fields belong to the same cells."""
    dumps = []
    for name in ("a", "b"):
        env = dict(os.environ)
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--grid", "2048x1024", "--steps", "12",
                              "--warmup", "3", "--dump-outputs", str(tmp_path / name)],
                             env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, out.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["steps"] == 12 and len(line["timing"]["repeats_ms_per_step"]) == 1 and line["ms_per_step"] > 0
        assert "also" not in line and "cpu_baseline" not in line
        files = sorted(os.listdir(tmp_path / name))
        assert files == sorted(f"{k}.npy" for k in ("av_vels", "cells", "u_x", "u_y", "u", "pressure"))
        assert sum(os.path.getsize(tmp_path / name / f) for f in files) <= 64 << 20
        dumps.append({f[:-4]: np.load(tmp_path / name / f) for f in files})
    a, b = dumps
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    n = 1 << 20                                       # 2048 x 1024 cells: half of them sampled
    assert a["cells"].shape == (n, 9) and all(a[k].shape == (n,) for k in ("u_x", "u_y", "u", "pressure"))
    assert a["av_vels"].shape[0] > 3 + 12 and np.isfinite(a["av_vels"]).all()
    idx = np.sort(np.random.default_rng(20261016).choice(2048 * 1024, size=n, replace=False))
    tile = lbm.read_obstacles(os.path.join(ROOT, "tests", "golden", "inputs", "obstacles_1024x1024.dat"), 1024, 1024)
    blocked = tile[(idx // 2048) % 1024, (idx % 2048) % 1024] == 1
    rho = a["cells"][:, 0].copy()
    for k in range(1, 9):
        rho += a["cells"][:, k]
    want_p = np.where(blocked, np.float32(0.1) * np.float32(1.0 / 3.0), rho * np.float32(1.0 / 3.0)).astype(np.float32)
    assert np.array_equal(a["pressure"].view(np.uint32), want_p.view(np.uint32))
    assert not a["u"][blocked].any()
