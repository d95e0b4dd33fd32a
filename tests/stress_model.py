"""The stress fields and the stress row of include/lbm_hip.h (lbm_read_stress, lbm_set_stress) in numpy float32, for the
tests: per cell the definition of the header in its order (stats_model.moments for rho, jx, jy, ux, uy, usq; every
operation rounded to float32, none contracted), blocked cells 0, the sums exact (math.fsum: the correctly rounded sum of
the exact terms), the maximum with its first cell.  `evaluate` runs the same expression tree in any dtype, so the float64
evaluation the accuracy bounds are stated against is the same text."""
import math

import numpy as np

import stats_model

FIELDS = ("sum_q", "sum_txy", "nonfinite", "max_q", "max_x", "max_y", "fluid")
U = 2.0 ** -24                                     # the unit roundoff of float32


def evaluate(f, dtype=np.float32):
    """{name: [ny, nx] of dtype} of the definition's every named value, from populations f[..., 9] taken as `dtype`"""
    f = np.asarray(f, dtype=dtype)
    with np.errstate(all="ignore"):
        rho = f[..., 0]
        for k in range(1, 9):
            rho = rho + f[..., k]
        jx = ((f[..., 1] + f[..., 5]) + f[..., 8]) - ((f[..., 3] + f[..., 6]) + f[..., 7])
        jy = ((f[..., 2] + f[..., 5]) + f[..., 6]) - ((f[..., 4] + f[..., 7]) + f[..., 8])
        ux = jx / rho
        uy = jy / rho
        usq = (ux * ux) + (uy * uy)
        a56 = f[..., 5] + f[..., 6]
        a78 = f[..., 7] + f[..., 8]
        mxx = ((f[..., 1] + f[..., 3]) + a56) + a78
        myy = ((f[..., 2] + f[..., 4]) + a56) + a78
        mxy = (f[..., 5] + f[..., 7]) - (f[..., 6] + f[..., 8])
        third = rho / dtype(3.0)
        pxx = (mxx - third) - (jx * ux)
        pyy = (myy - third) - (jy * uy)
        pxy = mxy - (jx * uy)
        txx = pxx / rho
        tyy = pyy / rho
        txy = pxy / rho
        q = ((txx * txx) + (tyy * tyy)) + (dtype(2.0) * (txy * txy))
    out = dict(rho=rho, jx=jx, jy=jy, ux=ux, uy=uy, usq=usq, a56=a56, a78=a78, mxx=mxx, myy=myy, mxy=mxy, third=third,
               pxx=pxx, pyy=pyy, pxy=pxy, txx=txx, tyy=tyy, txy=txy, q=q)
    for name, v in out.items():
        assert v.dtype == dtype, name            # every intermediate stays in the format: nothing was promoted
    return out


def field(cells_aos, obstacles):
    """({"txx", "txy", "tyy", "q"}: float32 [ny, nx] -- 0 on blocked cells, non-finite values as computed --, counted bool
    [ny, nx]: the finite fluid cells, bad bool [ny, nx]: the fluid cells that are not finite)"""
    ob = np.asarray(obstacles) != 0
    cells = np.asarray(cells_aos, dtype=np.float32).reshape(ob.shape + (9,))
    v = evaluate(cells)
    s_rho, s_jx, s_jy, _, _, s_usq, _ = stats_model.moments(cells)      # "exactly as in the statistics' text"
    for a, b in ((v["rho"], s_rho), (v["jx"], s_jx), (v["jy"], s_jy), (v["usq"], s_usq)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finite = np.ones(ob.shape, dtype=bool)
    for name in ("rho", "jx", "jy", "usq", "txx", "tyy", "txy", "q"):
        finite &= np.isfinite(v[name])
    zero = np.float32(0.0)
    t = {name: np.where(ob, zero, v[name]) for name in ("txx", "txy", "tyy", "q")}
    return t, ~ob & finite, ~ob & ~finite


def row(cells_aos, obstacles):
    """{field: value} of one lattice: the sums exact and rounded once"""
    t, counted, bad = field(cells_aos, obstacles)
    q = t["q"]
    out = {"sum_q": math.fsum(float(v) for v in q[counted]), "sum_txy": math.fsum(float(v) for v in t["txy"][counted]),
           "nonfinite": int(bad.sum()), "fluid": int(counted.sum())}
    if counted.any():
        key = np.where(counted, q, np.float32(-1.0)).reshape(-1)
        at = int(np.argmax(key))                                         # the first of the largest: the smallest y * nx + x
        out.update(max_q=np.float32(key[at]), max_x=at % q.shape[1], max_y=at // q.shape[1])
    else:
        out.update(max_q=np.float32(0.0), max_x=-1, max_y=-1)
    return out


def q_of_planes(txx, txy, tyy):
    """q recomputed in float32 from returned planes: the definition's last line"""
    txx, txy, tyy = (np.asarray(a, dtype=np.float32) for a in (txx, txy, tyy))
    with np.errstate(all="ignore"):
        q = ((txx * txx) + (tyy * tyy)) + (np.float32(2.0) * (txy * txy))
    assert q.dtype == np.float32
    return q


def oracle_rows(oracle, p, ob, cells, first, total, every, fields_at=()):
    """(final lattice, {tt: row}, {tt: fields}) of the oracle run from global step `first` for `total` steps, sampled after
    every tt with tt % every == 0; the fields after the steps tt of fields_at"""
    ref = cells.copy()
    out, fields = {}, {}
    for tt in range(first, first + total):
        with np.errstate(all="ignore"):
            oracle.run(p, ref, ob, 1)
        if tt % every == 0:
            out[tt] = row(ref, ob)
        if tt in fields_at:
            fields[tt] = field(ref, ob)[0]
    return ref, out, fields


def same_bits(got, want):
    """a row of the engine (numpy record of lbm.STRESS_DTYPE) against a model row, bit for bit; returns what differs"""
    diff = []
    for k in ("sum_q", "sum_txy"):
        if np.float64(got[k]).view(np.uint64) != np.float64(want[k]).view(np.uint64):
            diff.append((k, float(got[k]), want[k]))
    if np.float32(got["max_q"]).view(np.uint32) != np.float32(want["max_q"]).view(np.uint32):
        diff.append(("max_q", float(got["max_q"]), float(want["max_q"])))
    for k in ("nonfinite", "max_x", "max_y", "fluid"):
        if int(got[k]) != int(want[k]):
            diff.append((k, int(got[k]), int(want[k])))
    return diff


def same_field(got, want):
    """an engine's plane against the model's: the same cells NaN (a NaN's payload is not the arithmetic's to keep), the
    rest bit for bit"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(nan, np.isnan(got)) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def same_fields(got, want):
    """[plane names that differ] of Engine.stress() against field()'s planes"""
    return [name for name in ("txx", "txy", "tyy") if not same_field(got[name], want[name])]


# ---- a lattice with a prescribed stress ---------------------------------------------------------------------------------
W = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])


def constructed(rho, ux, uy, axx, axy, ayy):
    """float64 populations f_k = feq_k(rho, u) + (9/2) w_k (c_ka c_kb - delta_ab / 3) rho A_ab: rho and j are the
    equilibrium's and t_ab = A_ab, since sum_k w_k (c_a c_b - delta_ab / 3) c_c c_d = (delta_ac delta_bd + delta_ad delta_bc) / 9"""
    cu = CX * ux + CY * uy
    feq = W * rho * (1.0 + 3.0 * cu + 4.5 * cu * cu - 1.5 * (ux * ux + uy * uy))
    quad = (CX * CX - 1 / 3) * axx + 2.0 * (CX * CY) * axy + (CY * CY - 1 / 3) * ayy
    return feq + 4.5 * W * quad * rho


# ---- the fp32 accuracy of t ("Stress and dissipation") ---------------------------------------------------------
SECOND_ORDER = 1.0 + 2.0 ** -18    # every first-order term below is a product of at most four factors (1 + d), |d| <= 9 U


def t_bounds(exact):
    """(e_xx, e_yy, e_xy): per cell the most |t_ab(float32) - t_ab(exact)| can be for populations >= 0, from the values
    of `exact` (evaluate(..., np.float64)); the counts are DESIGN's, term by term:
      mxx: 5 additions of non-negative terms, each partial sum <= mxx                     5 U mxx
      third: rho's 8 additions (8 U rho), carried through / 3, and the divide's rounding      (8/3 + 1/3) U rho = 3 U rho
      mxx - third: exact (Sterbenz: mxx / 2 <= third <= 2 mxx)                                0
      jx: 2 + 2 additions of non-negative terms and one subtraction                           2 U mxx + U |jx|   =: e_jx
      ux = jx / rho: e_jx / rho + (8 + 1) U |ux|
      jx * ux: |jx| e_ux + |ux| e_jx + U |jx ux|                                              4 U |ux| mxx + 12 U rho ux^2
      the last subtraction                                                                    U |pxx|
      / rho: rho's 8 U and the divide's U, on txx                                             9 U |txx|
    and for txy: mxy = (f5 + f7) - (f6 + f8): U (f5 + f6 + f7 + f8) + U |mxy|; jx * uy with e_uy = (2 U myy + U |jy|) / rho
    + 9 U |uy|: 2 U (|ux| myy + |uy| mxx) + 12 U rho |ux uy|; then U |pxy| and 9 U |txy|."""
    rho, ux, uy = exact["rho"], np.abs(exact["ux"]), np.abs(exact["uy"])
    mxx, myy = exact["mxx"], exact["myy"]

    def diagonal(m, u, p, t):
        return (5 * m + 3 * rho + 4 * u * m + 12 * rho * u * u + np.abs(p)) / rho + 9 * np.abs(t)

    e_xx = diagonal(mxx, ux, exact["pxx"], exact["txx"])
    e_yy = diagonal(myy, uy, exact["pyy"], exact["tyy"])
    m4 = exact["a56"] + exact["a78"]
    e_xy = (m4 + np.abs(exact["mxy"]) + 2 * (ux * myy + uy * mxx) + 12 * rho * ux * uy + np.abs(exact["pxy"])) / rho + 9 * np.abs(exact["txy"])
    return tuple(U * SECOND_ORDER * e for e in (e_xx, e_yy, e_xy))


def q_bound(exact, e_xx, e_yy, e_xy):
    """per cell the most |q(float32) - q(exact)| can be: (|t| + e)^2 - t^2 for each square (the off-diagonal one twice),
    then the three squares' and the two additions' roundings of non-negative terms, at most 3 U q (2.0f * is exact)"""
    grow = lambda t, e: 2 * np.abs(t) * e + e * e
    d = grow(exact["txx"], e_xx) + grow(exact["tyy"], e_yy) + 2 * grow(exact["txy"], e_xy)
    return d + 3 * U * SECOND_ORDER * (exact["q"] + d)
