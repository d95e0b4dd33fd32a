"""CPU checks of the second moments of the mean fields (lbm_set_mean_order, lbm_read_mean2): exported, declared, the
argument checks that need no device, the rms_state.dat writer, the command line's LBM_MEAN_ORDER, the exactness the
definition rests on, and the host formulas of Engine.fluctuations.  Host-only: passes on a box without a GPU."""
import ctypes
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from cli_case import MALFORMED, run_cli


def test_moment_symbols_are_exported_and_declared(lbm):
    lib = ctypes.CDLL(lbm.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name in ("lbm_set_mean_order", "lbm_read_mean2"):
        assert name in lbm.ABI_SYMBOLS + lbm.ABI_SYMBOLS_NUMBERED
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, header)
    assert re.search(r"lbm_set_mean_order\(lbm_ctx\* ctx, int every, int order\)", header)
    assert re.search(r"lbm_read_mean2\(lbm_ctx\* ctx, double\* sum_uxux, double\* sum_uyuy, double\* sum_uxuy, "
                     r"double\* sum_pp,\s*long long\* n_samples\)", header)
    assert ctypes.sizeof(lbm._CInfo) == 20 * 4 and ctypes.sizeof(lbm._CBatchInfo) == 6 * 4


def test_null_context_is_refused(lbm):
    lib = lbm.load_library()
    n = ctypes.c_longlong(-1)
    for order in (1, 2):
        assert lib.lbm_set_mean_order(None, 10, order) != 0
        assert b"lbm_set_mean" in lib.lbm_last_error()
    assert b"lbm_set_mean_order: null context" in lib.lbm_last_error()
    assert lib.lbm_read_mean2(None, None, None, None, None, ctypes.byref(n)) != 0
    assert b"lbm_read_mean2: null context" in lib.lbm_last_error()


@pytest.mark.parametrize("order", [0, 3, 1.5, "2", "two", None, True, -1])
def test_python_order_check_needs_no_device(lbm, order):
    with pytest.raises(lbm.LbmError, match="order must be 1"):
        lbm._mean_order_arg(order)


def test_python_order_check_passes_good_values_through(lbm):
    assert lbm._mean_order_arg(1) == 1 and lbm._mean_order_arg(2) == 2
    out = lbm._mean_order_arg(np.int64(2))
    assert out == 2 and type(out) is int
    assert list(inspect.signature(lbm._mean_args).parameters) == ["every"]
    assert list(inspect.signature(lbm.Engine.set_mean_order).parameters) == ["self", "every", "order"]
    assert inspect.signature(lbm.Engine.set_mean_order).parameters["order"].default == 2
    for name in ("set_mean_order", "moment_sums", "fluctuations"):
        assert list(inspect.signature(getattr(lbm.Engine, name)).parameters)[0] == "self"
        assert getattr(lbm.BatchMember, name) is getattr(lbm.Engine, name)
    assert lbm.MOMENT_FIELDS == ("u_x u_x", "u_y u_y", "u_x u_y", "pressure pressure")
    assert list(inspect.signature(lbm.write_rms_state).parameters) == ["path", "fluct", "obstacles"]


def test_write_rms_state_round_trips(lbm, tmp_path):
    """final_state.dat's line format, columns rms_u_x rms_u_y cov_u_x_u_y rms_pressure, float64 rounded to float."""
    fluct = {"rms_u_x": np.array([[1.5e-3, 0.0], [0.123456789, 1.0]]), "rms_u_y": np.array([[2.5e-4, 0.0], [1.0, 2.0]]),
             "cov_u_x_u_y": np.array([[-1e-40, -0.0], [-1.0, 3.0]]), "rms_pressure": np.array([[1.0 / 3.0, 0.1 / 3.0], [2.0, 4.0]]),
             "var_u_x": np.full((2, 2), 99.0), "tke": np.full((2, 2), 99.0), "samples": 3}
    ob = np.array([[0, 1], [0, 0]], dtype=np.int32)
    path = tmp_path / "rms_state.dat"
    lbm.write_rms_state(str(path), fluct, ob)
    want = ("0 0 1.500000013039E-03 2.500000118744E-04 -9.999946101115E-41 3.333333432674E-01 0\n"
            "1 0 0.000000000000E+00 0.000000000000E+00 -0.000000000000E+00 3.333333507180E-02 1\n"
            "0 1 1.234567910433E-01 1.000000000000E+00 -1.000000000000E+00 2.000000000000E+00 0\n"
            "1 1 1.000000000000E+00 2.000000000000E+00 3.000000000000E+00 4.000000000000E+00 0\n")
    assert path.read_text() == want
    back = np.loadtxt(str(path)).reshape(2, 2, 7)
    cols = ("rms_u_x", "rms_u_y", "cov_u_x_u_y", "rms_pressure")
    for j, k in enumerate(cols):
        assert np.array_equal(back[:, :, 2 + j].astype(np.float32), fluct[k].astype(np.float32)), k
    assert np.array_equal(back[:, :, 6].astype(np.int32), ob)


@pytest.mark.parametrize("value", [""] + MALFORMED["LBM_MEAN_ORDER"])
def test_cli_dies_on_a_malformed_lbm_mean_order(lbm, tmp_path, value):
    """A message and exit(EXIT_FAILURE) before any device is touched.  (An empty value counts as unset, so the run goes
    on: on a box without a device to lbm_create's error.)"""
    out = run_cli(lbm, tmp_path, LBM_MEAN="10:2", LBM_MEAN_ORDER=value)
    if value == "":
        assert "LBM_MEAN_ORDER" not in out.stderr
        return
    assert out.returncode == 1
    assert "could not read LBM_MEAN_ORDER" in out.stderr
    for name in ("av_vels.dat", "final_state.dat", "mean_state.dat", "rms_state.dat"):
        assert not (tmp_path / name).exists()


@pytest.mark.parametrize("value", ["1", "2"])
def test_cli_dies_on_lbm_mean_order_without_lbm_mean(lbm, tmp_path, value):
    for extra in ({}, {"LBM_MEAN": ""}):
        out = run_cli(lbm, tmp_path, LBM_MEAN_ORDER=value, **extra)
        assert out.returncode == 1
        assert "LBM_MEAN_ORDER needs LBM_MEAN" in out.stderr
        for name in ("av_vels.dat", "final_state.dat", "mean_state.dat", "rms_state.dat"):
            assert not (tmp_path / name).exists()


def test_the_product_of_two_floats_is_exact_in_a_double():
    """The definition's premise: float64(a) * float64(b) IS a * b for floats a, b (48 significant bits at most, exponents
    within the double's range), so acc + (double)a * (double)b rounds once.  1e5 random pairs over the whole float range,
    with subnormals, values next to FLT_MAX and the smallest subnormal squared (2^-298, a normal double)."""
    rng = np.random.default_rng(2024)
    n = 100000
    bits = rng.integers(0, 2 ** 32, size=(2, n), dtype=np.uint64).astype(np.uint32)
    vals = bits.view(np.float32)
    vals[:, :2000] = (rng.integers(1, 2 ** 23, size=(2, 2000), dtype=np.uint32)).view(np.float32)      # subnormals
    vals[0, 1000:2000] *= np.float32(-1.0)
    fmax = np.finfo(np.float32).max
    vals[:, 2000:4000] = (np.float32(fmax).view(np.uint32) - rng.integers(0, 64, size=(2, 2000), dtype=np.uint32)).view(np.float32)
    vals[0, 4000] = vals[1, 4000] = np.float32(1e-45)                                                   # 2^-149, squared
    vals[0, 4001], vals[1, 4001] = fmax, np.float32(1e-45)
    vals[0, 4002], vals[1, 4002] = -fmax, fmax
    keep = np.isfinite(vals).all(axis=0)
    a, b = vals[0, keep], vals[1, keep]
    assert a.size > 0.98 * n and (np.abs(a) < np.finfo(np.float32).tiny).sum() >= 2000
    prod = a.astype(np.float64) * b.astype(np.float64)
    assert np.isfinite(prod).all()
    for x, y, z in zip(a.tolist(), b.tolist(), prod.tolist()):
        assert Fraction(x) * Fraction(y) == Fraction(z), (x, y, z)


def test_fluctuations_formulas_against_numpy(lbm):
    """fluctuations_of over the sums of a 50-sample synthetic float32 series against np.var / np.cov of the series in
    float64.

    Tolerance, with u = eps / 2 the unit roundoff of a double, n = 50 samples, q = S2 / n (for the covariance
    sqrt(q_xx q_yy) >= |q_xy| stands for q):
      S2 is a sum of n exact non-negative products, each addition rounded: relative error <= (n - 1) u; / n: + u;
      S1 likewise, error <= n u mean|x|, so m^2 is off by <= (2 n + 1) u mean|x|^2 + u m^2 <= (2 n + 2) u q (mean|x|^2 <= q);
      the subtraction rounds once more: <= u q.  Ours: <= (3 n + 3) u q.
      np.var / np.cov sum n squared deviations of a mean with error <= n u mean|x|: <= (n + 3) u var + terms of second
      order, and var <= q: <= (n + 3) u q.
    Sum: (4 n + 6) u q = (2 n + 3) eps q; asserted with (2 n + 4) eps q.  A square root halves a relative error, so the
    rms values are held to the same absolute bound divided by (2 rms) -- checked through their squares."""
    rng = np.random.default_rng(7)
    n, shape = 50, (6, 10)
    series = {k: (c + a * rng.standard_normal((n,) + shape)).astype(np.float32)
              for k, c, a in (("u_x", 0.05, 0.01), ("u_y", -0.002, 0.004), ("pressure", 0.0333, 1e-4))}
    series["u_y"] = (series["u_y"] + np.float32(0.3) * (series["u_x"] - np.float32(0.05))).astype(np.float32)   # correlated
    series["u_x"][:, 0, 0] = np.float32(0.05)                 # a constant cell: variance 0, the clamp's case
    series["u"] = np.hypot(series["u_x"], series["u_y"])
    sums = {k: np.zeros(shape) for k in ("u_x", "u_y", "u", "pressure")}
    sums2 = {k: np.zeros(shape) for k in lbm.MOMENT_FIELDS}
    for i in range(n):
        for k in sums:
            sums[k] = sums[k] + series[k][i].astype(np.float64)
        for k in sums2:
            a, b = k.split(" ")
            sums2[k] = sums2[k] + series[a][i].astype(np.float64) * series[b][i].astype(np.float64)
    f = lbm.fluctuations_of(sums, sums2, n)
    assert f["samples"] == n and set(f) == {"var_u_x", "var_u_y", "cov_u_x_u_y", "var_pressure", "rms_u_x", "rms_u_y",
                                            "rms_pressure", "tke", "samples"}
    eps = np.finfo(np.float64).eps
    x64 = {k: v.astype(np.float64) for k, v in series.items()}
    q = {k: sums2[k] / n for k in sums2}
    for k in ("u_x", "u_y", "pressure"):
        tol = (2 * n + 4) * eps * q[k + " " + k]
        want = np.var(x64[k], axis=0)
        assert (f["var_" + k] >= 0).all() and f["var_" + k].dtype == np.float64
        assert (np.abs(f["var_" + k] - want) <= tol).all(), k
        assert (np.abs(f["rms_" + k] ** 2 - want) <= tol + 2 * eps * want).all(), k
        assert np.array_equal(f["rms_" + k], np.sqrt(f["var_" + k]))
    assert f["var_u_x"][0, 0] <= (2 * n + 4) * eps * q["u_x u_x"][0, 0]
    want = np.mean((x64["u_x"] - x64["u_x"].mean(axis=0)) * (x64["u_y"] - x64["u_y"].mean(axis=0)), axis=0)
    flat = np.array([np.cov(x64["u_x"][:, j, i], x64["u_y"][:, j, i], bias=True)[0, 1] for j in range(shape[0]) for i in range(shape[1])])
    tol = (2 * n + 4) * eps * np.sqrt(q["u_x u_x"] * q["u_y u_y"])
    assert (np.abs(want.ravel() - flat) <= tol.ravel()).all()
    assert (np.abs(f["cov_u_x_u_y"] - want) <= tol).all()
    assert (f["cov_u_x_u_y"][1:, 1:] > 0).all()                # the series was built correlated
    assert np.array_equal(f["tke"], 0.5 * (f["var_u_x"] + f["var_u_y"]))
    with pytest.raises(lbm.LbmError, match="no sample"):
        lbm.fluctuations_of(sums, sums2, 0)
