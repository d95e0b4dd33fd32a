"""CPU checks of the batch entry points (lbm_create_batch and friends): everything lbm_create_batch can reject without a
device is rejected before any device call, with a message that names the offending member; without a device creation
fails like lbm_create.  Host-only: passes on a box without a GPU."""
import ctypes

import numpy as np
import pytest


def cparams(lbm, plist):
    return (lbm._CParams * len(plist))(*[p._c() for p in plist])


def create(lbm, plist, obstacles=True, math=0):
    lib = lbm.load_library()
    n = len(plist)
    nx, ny = (plist[0].nx, plist[0].ny) if plist else (1, 2)
    ob = np.zeros((max(n, 1), ny, nx), dtype=np.int32)
    arr = cparams(lbm, plist) if plist else None
    h = lib.lbm_create_batch(n, arr, ob.ctypes.data if obstacles else None, None, math)
    return h, lib.lbm_last_error().decode()


def test_batch_symbols_are_exported(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    for name in ("lbm_create_batch", "lbm_batch_member", "lbm_batch_run", "lbm_batch_sync", "lbm_batch_get_info",
                 "lbm_destroy_batch"):
        assert name in lbm.ABI_SYMBOLS
        assert hasattr(lib, name)


def test_create_batch_rejects_mismatched_shape_naming_the_member(lbm):
    p = lbm.Params(128, 128, 100, 128, 0.1, 0.005, 1.85)
    q = lbm.Params(128, 256, 100, 128, 0.1, 0.005, 1.85)
    h, err = create(lbm, [p, p, p, q, p])
    assert not h
    assert "member 3 is 128x256, member 0 is 128x128" in err


def test_create_batch_rejects_mismatched_max_iters(lbm):
    p = lbm.Params(64, 64, 100, 64, 0.1, 0.005, 1.85)
    q = lbm.Params(64, 64, 200, 64, 0.1, 0.005, 1.85)
    h, err = create(lbm, [p, q])
    assert not h
    assert "member 1 has max_iters 200" in err


def test_create_batch_rejects_bad_counts_pointers_and_modes(lbm):
    p = lbm.Params(64, 64, 100, 64, 0.1, 0.005, 1.85)
    h, err = create(lbm, [])
    assert not h and "n_members" in err
    h, err = create(lbm, [p, p], obstacles=False)
    assert not h and "obstacles is NULL" in err
    h, err = create(lbm, [p, p], math=7)
    assert not h and "math mode" in err
    bad = lbm.Params(0, 64, 100, 64, 0.1, 0.005, 1.85)
    h, err = create(lbm, [p, bad])
    assert not h and "member 1" in err


def test_create_batch_without_device_fails_loudly(lbm):
    p = lbm.Params(64, 64, 100, 64, 0.1, 0.005, 1.85)
    if lbm.device_count() == 0:
        h, err = create(lbm, [p, p, p])
        assert not h
        assert "no HIP device" in err
        with pytest.raises(lbm.LbmError, match="no HIP device"):
            lbm.Batch([p, p], [np.zeros((64, 64), np.int32)] * 2)


def test_batch_handles_null_arguments(lbm):
    lib = lbm.load_library()
    assert not lib.lbm_batch_member(None, 0)
    assert lib.lbm_batch_run(None, 1) != 0
    assert lib.lbm_batch_sync(None) != 0
    info = lbm._CBatchInfo()
    assert lib.lbm_batch_get_info(None, ctypes.byref(info)) != 0
    lib.lbm_destroy_batch(None)    # a no-op, like lbm_destroy(NULL)


def test_python_batch_checks_shapes_and_counts(lbm):
    p = lbm.Params(64, 64, 100, 64, 0.1, 0.005, 1.85)
    q = lbm.Params(64, 128, 100, 64, 0.1, 0.005, 1.85)
    ob = np.zeros((64, 64), np.int32)
    with pytest.raises(lbm.LbmError, match="member 2 is 64x128, member 0 is 64x64"):
        lbm.Batch([p, p, q], [ob] * 3)
    with pytest.raises(lbm.LbmError, match="2 obstacle maps for 3 members"):
        lbm.Batch([p, p, p], [ob, ob])
    with pytest.raises(lbm.LbmError, match="2 obstacle maps for 3 members"):
        lbm.Batch([p, p, p], np.zeros((2, 64, 64), np.int32))
    with pytest.raises(lbm.LbmError, match="member 1: obstacle map"):
        lbm.Batch([p, p], [ob, np.zeros((32, 64), np.int32)])
    with pytest.raises(lbm.LbmError, match="1 initial lattices for 2 members"):
        lbm.Batch([p, p], [ob, ob], cells=[np.zeros((64, 64, 9), np.float32)])
    with pytest.raises(lbm.LbmError, match="at least 1"):
        lbm.Batch([], [])
    with pytest.raises(lbm.LbmError, match="math mode"):
        lbm.Batch([p], [ob], math="sloppy")
