"""CPU checks of the obstacle forces of a batch (lbm_batch_set_forces, lbm_batch_read_forces, lbm_batch_forces_links):
exported and declared with their signatures, a NULL batch refused by each, the info structs' sizes, and the argument
checks of Batch.set_forces that need no device.  Host-only: passes on a box without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("lbm_batch_set_forces", "lbm_batch_read_forces", "lbm_batch_forces_links")


def test_symbols_are_exported_and_declared(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lbm_hip.h")).read())
    for name in NAMES:
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)
    assert re.search(r"int lbm_batch_set_forces\(lbm_batch\* batch, int n_bodies, const int\* body_of_cell[^,]*, int every, int capacity\);", header)
    assert re.search(r"int lbm_batch_read_forces\(lbm_batch\* batch, int max_rows, double\* out[^,]*, int\* steps, int\* n_read\);", header)
    assert re.search(r"int lbm_batch_forces_links\(lbm_batch\* batch, int\* links[^,)]*\);", header)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4   # the info structs keep their layout


def test_null_batch_is_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_int(-1)
    assert lib.lbm_batch_set_forces(None, 1, None, 10, 4) != 0
    assert b"lbm_batch_set_forces: null batch" in lib.lbm_last_error()
    assert lib.lbm_batch_read_forces(None, 0, None, None, ctypes.byref(n)) != 0
    assert b"lbm_batch_read_forces" in lib.lbm_last_error()
    assert lib.lbm_batch_forces_links(None, None) != 0
    assert b"lbm_batch_forces_links" in lib.lbm_last_error()


def maps(n, shape=(8, 16), dtype=np.int32):
    return [np.zeros(shape, dtype=dtype) for _ in range(n)]


@pytest.mark.parametrize("every,capacity,bodies,n_bodies,match", [
    (10, 4, maps(2), None, "2 label maps for 3 members"), (10, 4, maps(4), None, "4 label maps for 3 members"),
    (10, 4, np.zeros((2, 8, 16), dtype=np.int32), None, "2 label maps for 3 members"),
    (10, 4, 7, None, "one integer array of shape"),
    (10, 4, maps(2) + maps(1, (8, 15)), None, "integer array of shape"), (10, 4, maps(3, (16, 8)), None, "integer array of shape"),
    (10, 4, maps(3, dtype=np.float32), None, "integer array of shape"), (10, 4, np.zeros((3, 128), dtype=np.int32)[:, :64], None, "integer array of shape"),
    (10, 4, None, 0, "0 bodies, between 1 and"), (10, 4, None, 65, "65 bodies"), (10, 4, maps(3), 65, "65 bodies"),
    (10, 4, maps(2) + [maps(1)[0] + 64], None, "65 bodies, between 1 and LBM_MAX_BODIES = 64"),
    (-1, 4, None, None, r"every must lie in \[0, 2\^31\)"), (-1, 4, maps(3), None, r"every must lie in \[0, 2\^31\)"),
    (10, 0, maps(3), None, "at least one row")])
def test_python_argument_checks_need_no_device(lbm, every, capacity, bodies, n_bodies, match):
    with pytest.raises(lbm.LbmError, match=match):
        lbm._batch_forces_args(every, capacity, bodies, n_bodies, 3, 16, 8)


def test_python_argument_checks_pass_good_values_through(lbm):
    assert lbm._batch_forces_args(0, 0, None, None, 3, 16, 8) == (0, 0, 1, None)
    assert lbm._batch_forces_args(3, 7, None, 64, 3, 16, 8) == (3, 7, 64, None)
    labels = maps(3)
    labels[1][2, 3] = 5                        # n_bodies is taken over all members
    labels[2][0, 0] = -1                       # outside the range: the engine refuses it if the cell is blocked
    every, capacity, n_bodies, flat = lbm._batch_forces_args(7, 2, labels, None, 3, 16, 8)
    assert (every, capacity, n_bodies) == (7, 2, 6)
    assert flat.dtype == np.int32 and flat.flags.c_contiguous and flat.shape == (3, 128)
    assert flat[1, 2 * 16 + 3] == 5 and flat[2, 0] == -1 and flat[0].max() == 0
    stacked = lbm._batch_forces_args(7, 2, np.stack(labels).astype(np.int64), 9, 3, 16, 8)
    assert stacked[2] == 9 and np.array_equal(stacked[3], flat)


def test_batch_signatures(lbm):
    sig = inspect.signature(lbm.Batch.set_forces)
    assert list(sig.parameters) == ["self", "every", "capacity", "bodies", "n_bodies"]
    assert sig.parameters["capacity"].default == 4096 and sig.parameters["bodies"].default is None
    assert sig.parameters["n_bodies"].default is None
    assert list(inspect.signature(lbm.Batch.forces).parameters) == ["self", "max_rows"]
    assert list(inspect.signature(lbm.Batch.force_links).parameters) == ["self"]
