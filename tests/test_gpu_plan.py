"""create_common runs on the planner's answer: for six contexts, what lbm_get_info reports equals what
tests/plan_dump.cpp (lbm_plan.h, host arithmetic only) decides for this device's CU count -- the resident candidate
included, which the engine confirms with the device's occupancy query -- and four steps of each are bit-identical to
the CPU oracle, compared as test_gpu_parity.py compares them.
"""
import os

import numpy as np
import pytest
import torch

import plan_tool
from test_gpu_parity import AV_RTOL, random_case

pytestmark = pytest.mark.gpu

RESIDENT_CHUNK = 4096       # timesteps one resident launch advances at most (kResidentChunk)

# nx, ny, slabs
CONTEXTS = [(128, 128, 1), (100, 64, 1), (256, 64, 1), (640, 640, 1), (2048, 2048, 1), (1024, 64, 2)]


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return plan_tool.build(tmp_path_factory.mktemp("plan_dump"))


def info_of(plan, halo_on):
    """lbm_get_info's view of a plan (synchronous halos)."""
    tile = plan["tile_steps"] if not halo_on else 0
    stream = bool(plan["fuse2"]) and not tile
    resident = plan["resident"]
    return dict(steps_per_launch=tile or (plan["pass_steps"] if plan["fuse2"] else 1),
                band_rows=plan["band_rows"] if stream else 0,
                lane_cells=plan["lane_cells"] if stream else 0,
                band_groups=plan["band_groups"] if stream else 1,
                nontemporal=plan["nts"],
                resident_steps=RESIDENT_CHUNK if resident else 0,
                resident_min_steps=plan["resident_min_steps"] if resident else 0,
                resident_rows=plan["resident_rows"] if resident else 0,
                resident_group=plan["resident_group"] if resident else 0,
                resident_one_xcd=plan["resident_one_xcd"] if resident else 0)


@pytest.mark.parametrize("nx,ny,slabs", CONTEXTS)
def test_context_runs_on_the_planners_answer(lbm, oracle, plan_dump, monkeypatch, nx, ny, slabs):
    for name in [k for k in os.environ if k.startswith("LBM_")]:
        monkeypatch.delenv(name)
    env = {}
    if slabs > 1:
        env["LBM_HALO"] = "memcpy"            # slabs that share a device exchange by device copies
        monkeypatch.setenv("LBM_HALO", "memcpy")
    n_devices = lbm.device_count()
    want = plan_tool.run(plan_dump, nx=nx, ny=ny, n_slabs=slabs, halo=plan_tool.HALO["memcpy" if slabs > 1 else "none"],
                         cus=torch.cuda.get_device_properties(0).multi_processor_count, n_devices=n_devices,
                         distinct_devices=1 < slabs <= n_devices, env=env)
    p, ob, cells = random_case(lbm, nx, ny, 31 + nx + ny + slabs)
    steps = 4
    ref = cells.copy()
    ref_av = oracle.run(p, ref, ob, steps)
    with lbm.Engine(p, ob, cells, n_gpus=slabs) as eng:
        info = eng.info()
        expected = info_of(want["plan"], halo_on=slabs > 1)
        assert {k: info[k] for k in expected} == expected
        assert (info["graph_steps"] > 0) == bool(want["plan"]["use_graph"])
        assert info["n_slabs"] == slabs == len(want["slabs"])
        assert info["row_count"] == sum(s["rows"] for s in want["slabs"])
        eng.run(steps)
        got = eng.cells()
        got_av = eng.av_vels(steps)
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL, atol=0)
