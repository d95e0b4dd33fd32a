"""Band groups (LBM_BAND_GROUPS): the full-depth passes of a single periodic slab issued as G row groups on their own
streams, interiors and seams ordered by events only, so that successive passes overlap.  The split changes which
wave relaxes which row and nothing else: the lattice must stay bit-identical to one launch per pass (G = 1), and
av_vels, summed over a different partition of waves, within 1e-6 relative.  Everything through the C ABI."""
import hashlib
import os

import numpy as np
import pytest

from test_gpu_parity import AV_RTOL, random_case, run_both
from test_gpu_stream_k import force_stream

pytestmark = pytest.mark.gpu

GROUP_RTOL = 1e-6


def run_engine(lbm, monkeypatch, groups, p, ob, cells, calls, tiled=False, every=0):
    """(lattice, av_vels, frames, info) after `calls` from step 0 with LBM_BAND_GROUPS=groups."""
    monkeypatch.setenv("LBM_BAND_GROUPS", str(groups))
    frames = []
    with lbm.Engine(p, ob, cells, tiled=tiled) as eng:
        if every:
            eng.set_frames(every, 1 + sum(calls) // every)
        for n in calls:
            eng.run(n)
            if every:
                frames.append(eng.frames()[1])
        return eng.cells(), eng.av_vels(sum(calls)), frames, eng.info()


def assert_same(base, got, what):
    assert np.array_equal(base[0].view(np.uint32), got[0].view(np.uint32)), f"{what}: lattice differs"
    np.testing.assert_allclose(got[1], base[1], rtol=GROUP_RTOL, atol=0, err_msg=what)
    for i, (fb, fg) in enumerate(zip(base[2], got[2])):
        assert np.array_equal(fb.view(np.uint32), fg.view(np.uint32)), f"{what}: frames of call {i} differ"


def test_flagship_grid_bit_identical(lbm, monkeypatch):
    """8192^2 (the bench's grid, tiled obstacle map) after 50 steps: 12 four-step passes and a two-step tail."""
    inputs = os.path.join(os.path.dirname(__file__), "golden", "inputs")
    tile = lbm.read_obstacles(os.path.join(inputs, "obstacles_1024x1024.dat"), 1024, 1024)
    p = lbm.Params(8192, 8192, 50, 10, 0.1, 0.01, 1.85)
    digests = {}
    for groups in (1, 2, 3):
        cells, av, _, info = run_engine(lbm, monkeypatch, groups, p, tile, None, [50], tiled=True)
        assert info["band_groups"] == groups and info["steps_per_launch"] == 4, info
        assert np.all(np.isfinite(av))
        digests[groups] = (hashlib.sha256(cells.view(np.uint8)).hexdigest(), av)
        del cells
    for groups in (2, 3):
        assert digests[groups][0] == digests[1][0], f"G = {groups}: lattice differs"
        np.testing.assert_allclose(digests[groups][1], digests[1][1], rtol=GROUP_RTOL, atol=0)


@pytest.mark.parametrize("nx,ny,steps", [(2048, 2048, 30), (4096, 1024, 31)])
def test_default_sizes_bit_identical(lbm, monkeypatch, nx, ny, steps):
    """Random populations and obstacles, no side walls (both wraps live); 30 = 7 passes + a two-step tail,
    31 = 7 passes + two steps + one step."""
    p, ob, cells = random_case(lbm, nx, ny, nx + ny, walls=False)
    base = run_engine(lbm, monkeypatch, 1, p, ob, cells, [steps])
    assert base[3]["band_groups"] == 1
    for groups in (2, 3):
        got = run_engine(lbm, monkeypatch, groups, p, ob, cells, [steps])
        assert got[3]["band_groups"] == groups
        assert_same(base, got, f"{nx}x{ny}, G = {groups}")
    # the default is two groups
    monkeypatch.delenv("LBM_BAND_GROUPS")
    with lbm.Engine(p, ob, cells) as eng:
        assert eng.info()["band_groups"] == 2


def test_run_in_pieces(lbm, monkeypatch):
    """run(7); run(13): each call forks and joins the group streams, with tails of 3 and 1 steps."""
    p, ob, cells = random_case(lbm, 2048, 2048, 11, walls=False)
    base = run_engine(lbm, monkeypatch, 1, p, ob, cells, [20])
    for groups in (2, 3):
        got = run_engine(lbm, monkeypatch, groups, p, ob, cells, [7, 13])
        assert_same(base, got, f"pieces, G = {groups}")


def test_frames_every_six_steps(lbm, monkeypatch):
    """Frames cut every call into segments that end at a frame step; every segment ends behind a join."""
    p, ob, cells = random_case(lbm, 2048, 2048, 12)
    base = run_engine(lbm, monkeypatch, 1, p, ob, cells, [40, 9], every=6)
    assert sum(len(f) for f in base[2]) == 9
    for groups in (2, 3):
        got = run_engine(lbm, monkeypatch, groups, p, ob, cells, [40, 9], every=6)
        assert_same(base, got, f"frames, G = {groups}")


@pytest.mark.parametrize("nx,ny,groups,band", [(256, 128, 2, 7), (256, 130, 3, 5), (128, 200, 3, 64), (512, 96, 2, 3)])
def test_small_grids_against_oracle(lbm, oracle, monkeypatch, nx, ny, groups, band):
    """Forced groups on small grids against the CPU oracle.  The lid row ny-2 lies in the wrapping seam (within K
    rows of row 0); 130 and 200 rows do not divide by three (the last group takes the remainder); band 64 is taller
    than a group's interior."""
    force_stream(monkeypatch, 4, band, prefetch=1, packed=12)
    monkeypatch.setenv("LBM_GRAPH", "0")          # (graph replay is the default below 64 Ki cells)
    monkeypatch.setenv("LBM_BAND_GROUPS", str(groups))
    p, ob, cells = random_case(lbm, nx, ny, nx * ny, walls=False)
    for steps in (24, 26, 27):
        ref_cells, ref_av, got_cells, got_av, _ = run_both(lbm, oracle, p, ob, cells, steps)
        assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32)), steps
        np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)
    with lbm.Engine(p, ob, cells) as eng:
        assert eng.info()["band_groups"] == groups


@pytest.mark.parametrize("groups", [2, 3])
@pytest.mark.parametrize("k,packed,band,prefetch", [(4, 12, 7, 1), (4, 1, 5, 0), (3, 12, 9, 1)])
def test_reference_dataset_on_stream_kernel(lbm, oracle, datasets, monkeypatch, groups, k, packed, band, prefetch):
    """The reference's 128x256 data set (wall row in the middle) forced onto the stream kernel with groups."""
    force_stream(monkeypatch, k, band, prefetch, packed=packed)
    monkeypatch.setenv("LBM_GRAPH", "0")
    monkeypatch.setenv("LBM_BAND_GROUPS", str(groups))
    p, ob = datasets("128x256")
    cells = oracle.init_cells(p)
    for steps in (76, 77, 79):
        ref_cells, ref_av, got_cells, got_av, fields = run_both(lbm, oracle, p, ob, cells, steps)
        assert np.array_equal(ref_cells.view(np.uint32), got_cells.view(np.uint32)), steps
        np.testing.assert_allclose(got_av, ref_av, rtol=AV_RTOL)
        ref_f = oracle.final_state(p, ref_cells, ob)
        assert np.array_equal(ref_f["pressure"].view(np.uint32), fields["pressure"].view(np.uint32))
    with lbm.Engine(p, ob, cells) as eng:
        assert eng.info()["band_groups"] == groups
