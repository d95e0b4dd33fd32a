"""Every exact instantiation of the multi-step stream kernels, bit for bit against the oracle, with strip seams.

The cases (tests/stream_rows.py: CASES) name each of the 64 rows of the exact dispatch tables of lbm_hip.hip on one
periodic slab and again on three slabs with device-copy halos, at 516 x 29 with bands of 5 rows: three strips on
four-cell lanes, five on two-cell lanes, a ragged last strip, a row pitch that is not nx, and blocked cells on both sides
of every seam.  Beyond that: XCD chunks of two strips (a ragged last chunk, trailing workgroups that return early) per
family, K and owner; band groups of two and three with interiors down to one row; graph replay; the rank API on a ring of
one.  tests/test_stream_rows.py shows on the CPU that each case is planned as asked and launches its row.

Each case runs 2K + 3 steps -- full passes, a two-step pass, a one-step launch -- in one call and split as (K + 1, K + 2):

* Engine.info() shows the kernel asked for (and graph replay exactly where asked);
* the lattice is bit-identical to oracle.run;
* the four final_state fields are bit-identical to the oracle's final_state of that lattice;
* av_vels is within test_gpu_parity.AV_RTOL of the oracle's sequential fp32 sums (tests/test_gpu_av_vels.py holds the
  kernel families to the derived bound).
"""
import numpy as np
import pytest

import stream_rows
from stream_rows import CASES, INFO_FIELDS
from test_gpu_parity import AV_RTOL

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_stream_row_is_the_oracle(lbm, monkeypatch, case):
    for key, value in case.env.items():
        monkeypatch.setenv(key, value)
    p, ob, cells = stream_rows.lattice()
    want_cells, want_av, want_fields = stream_rows.model(case.steps)
    for calls in case.calls:
        kwargs = {"n_gpus": case.slabs}
        if case.owner == "rank":                # a communicator of its own per engine: a unique id serves one
            kwargs = {"rank": 0, "world_size": 1, "unique_id": lbm.rccl_unique_id(), "device": 0}
        with lbm.Engine(p, ob, cells.copy(), **kwargs) as eng:
            info = eng.info()
            assert {k: info[k] for k in INFO_FIELDS} == {k: case.expect[k] for k in INFO_FIELDS}, info
            assert (info["graph_steps"] > 0) == case.expect["graph"], info
            for n in calls:
                eng.run(n)
            assert eng.info()["steps_done"] == case.steps
            got_cells, got_av, fields = eng.cells(), eng.av_vels(case.steps), eng.final_state()
        differ = bits(got_cells) != bits(want_cells)
        if differ.any():
            ys, xs, _ = np.nonzero(differ)
            raise AssertionError(f"{case.id} {list(calls)}: {int(differ.sum())} populations differ from the oracle's; rows "
                                 f"{sorted(set(ys.tolist()))[:12]}, columns {sorted(set(xs.tolist()))[:16]}")
        for name in ("u_x", "u_y", "u", "pressure"):
            assert np.array_equal(bits(fields[name]), bits(want_fields[name])), (case.id, list(calls), name)
        np.testing.assert_allclose(got_av, np.asarray(want_av)[:case.steps], rtol=AV_RTOL, atol=0)
