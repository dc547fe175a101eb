"""rtm_kernel, rtm_scan_kernel and rtm_jac_kernel against the extended-precision truth of tests/rtm_truth.py, on optical depths
that stress how the kernels regroup the reference's RAD_UP_DN / CALCTMR / RTM loop (layer groups per workgroup, the optical depth
above a group as ODTOT - below - part, upward terms added top-down, exp_cw / rcp2 / planck of device_common.hpp): opaque layers
under, over and between thin ones, layers so thin that 1 - exp(-tau) cancels, transmittances that underflow, groups without layers
(nlay < G), the padded layers of a ragged batch, +inf and NaN layers.  Contexts without TAPE3: RTM needs no line table.

Bounds (none is fitted to the kernels; E and the classes are defined in tests/rtm_truth.py, E_orc = E(oracle, truth) is taken on the
same inputs in the same test):
  1. E(kernel, truth) <= 4 E_orc + 64 eps (real_kind 8) or + 2^-24 (real_kind 4: one rounding of the output).  4: exp_cw is documented
     at 1-2 ulp against libm's <= 1, and the sums run in another order.
  2. E(kernel, oracle) <= 1e-6 (real_kind 4: SGL_VS_DBL of tests/test_hip_parity.py) wherever E_orc <= 1e-7.
  3. `degenerate` (zeros, denormals, 1e-300 .. 1e-10): the oracle's NaN and zero pattern, finite values within 1e-6 of it.
Every call is made twice, the padding beyond nlay[p] once zero and once NaN: the results must be identical.

Launch instantiations (real_kind R): A64, L200 -> <R, 16>; B30, D48 -> <R, 8>; C12 -> <R, 2>; the Jacobians <double, 8> and <double, 2>.
tests/test_adjoint_extremes.py holds the adjoints (rtm_jac_kernel in both real kinds and on A64, rtm_scan_jac_kernel, rtm_obs_jac_kernel)
and rtm_obs_kernel to the same truth and its closed-form adjoint, with this module's batches, classes and raw_* helpers.
Run with -s for every figure; MONORTM_TRUTH_RECORD names a file that collects the worst of each."""
import ctypes as C

import numpy as np
import pytest

import common  # noqa: F401  (puts the repository root on sys.path)
import rtm_truth as tr
from monortm_amd import api

pytestmark = pytest.mark.gpu

OUT = tr.OUT
EPS = 2.0 ** -52
SGL_VS_DBL = 5e-5                                  # tests/test_hip_parity.py
FACTORS = [1.0, 0.7, 5.76, 19.1, 1e-3]             # two path tiles (4 + 1)
SMALL = ("A64", "B30", "C12", "L200")              # run once per class; D48 (140 profiles) cycles the classes over its profiles


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    yield True
    tr.dump_record()


@pytest.fixture(scope="module")
def ctx(gpu):
    c = {8: api.MonoRTM("", 0.0, 0.0), 4: api.MonoRTM("", 0.0, 0.0, real_kind=4)}
    yield c
    for r in c.values():
        r.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def raw_rtm(r, b, a):
    """monortm_hip_rtm on the arrays a (tests/rtm_truth.py Batch.rounded) -> dict of [nprof, nwn], tmpsfc as written back."""
    outs = {k: np.full((b.nprof, b.nwn), -7.0, r.dtype) for k in OUT}
    ts = a["ts"].copy()
    rc = r.lib.monortm_hip_rtm(r.ctx, b.nprof, b.nwn, _p(b.wn), _p(b.nlay), b.lm, _p(b.irt), 1, _p(a["T"]), _p(a["TZ"]), _p(a["O"]), _p(ts),
                               _p(a["em"]), _p(a["rf"]), *[_p(outs[k]) for k in OUT])
    assert rc == 0, r.lib.monortm_hip_last_error(r.ctx)
    return outs, ts


def raw_scan(r, b, a, path):
    outs = {k: np.full((b.nprof, path.shape[1], b.nwn), -7.0, r.dtype) for k in OUT}
    ts = a["ts"].copy()
    rc = r.lib.monortm_hip_rtm_scan(r.ctx, b.nprof, path.shape[1], b.nwn, _p(b.wn), _p(b.nlay), b.lm, _p(b.irt), 1, _p(a["T"]), _p(a["TZ"]),
                                    _p(a["O"]), _p(path), _p(ts), 0, _p(a["em"]), _p(a["rf"]), *[_p(outs[k]) for k in OUT])
    assert rc == 0, r.lib.monortm_hip_last_error(r.ctx)
    return outs, ts


def raw_jac(r, b, a, quantity):
    sh = dict(rad=(b.nprof, b.nwn), tb=(b.nprof, b.nwn), k_o=(b.nprof, b.lm, b.nwn), k_t=(b.nprof, b.lm, b.nwn),
              k_tz=(b.nprof, b.lm + 1, b.nwn), k_sfc=(b.nprof, 3, b.nwn))
    out = {k: np.full(s, -7.0, r.dtype) for k, s in sh.items()}
    rc = r.lib.monortm_hip_rtm_jac(r.ctx, b.nprof, b.nwn, _p(b.wn), _p(b.nlay), b.lm, _p(b.irt), int(quantity == "tb"), _p(a["T"]), _p(a["TZ"]),
                                   _p(a["O"]), _p(a["ts"]), _p(a["em"]), _p(a["rf"]), *[_p(out[k]) for k in sh])
    assert rc == 0, r.lib.monortm_hip_last_error(r.ctx)
    return out


def same(x, y):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in x)


make_batch = tr.make_batch


def check_against_truth(what, kind, b, got, truth, orc):
    """Assertions 1-3 of the module docstring per class present in the batch and per field; every figure is printed and recorded
    first.  got / truth / orc: dicts of arrays whose first axis is the profile."""
    fails = []
    for cls in tr.CLASSES:
        sel = b.profiles_of(cls)
        if not sel:
            continue
        for k in OUT:
            g, t, o = got[k][sel], truth[k][sel], orc[k][sel]
            sl = k == "trtot"   # the one field that is denormal outside `degenerate`
            e_orc, e_t, e_o = tr.E(o, t, o, 8, sl), tr.E(g, t, o, kind, sl), tr.E(g, o, o, kind, sl)
            print(f"{what} {cls:14s} {k:5s} E_orc {e_orc:.1e}  E(kernel, truth) {e_t:.1e}  E(kernel, oracle) {e_o:.1e}")
            for tag, v in (("E_orc", e_orc), ("E_truth", e_t), ("E_oracle", e_o)):
                tr.record(f"{what.split()[0]}/{tag}/{cls}/{kind}/{k}", v)
            if not e_t <= 4 * e_orc + (64 * EPS if kind == 8 else 2.0 ** -24):
                fails.append(f"{cls} {k}: E(kernel, truth) {e_t:.2e} > 4 x {e_orc:.2e} + rounding")
            if e_orc <= 1e-7 and not e_o <= (1e-6 if kind == 8 else SGL_VS_DBL):
                fails.append(f"{cls} {k}: E(kernel, oracle) {e_o:.2e}")
            if cls == "degenerate":
                o_k = o.astype(np.float32) if kind == 4 else o
                if not tr.same_pattern(g, o_k):
                    fails.append(f"{cls} {k}: NaN / zero pattern differs from the oracle's")
                fin = np.isfinite(o_k) & (o_k != 0)
                if not np.all(np.abs(g[fin] - o_k[fin]) <= (1e-6 if kind == 8 else SGL_VS_DBL) * np.abs(o_k[fin])):
                    fails.append(f"{cls} {k}: finite values further than 1e-6 from the oracle")
    assert not fails, f"{what}: " + "; ".join(fails)


def cases():
    return [(n, c) for n in SMALL for c in tr.CLASSES] + [("D48", "cycled")]


# ---- monortm_hip_rtm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("name,cls", cases())
def test_rtm_against_truth(ctx, name, cls, kind):
    r = ctx[kind]
    b = make_batch(name, cls)
    a0, an = b.rounded(r.dtype, 0.0), b.rounded(r.dtype, np.nan)
    got, ts = raw_rtm(r, b, a0)
    got_n, ts_n = raw_rtm(r, b, an)
    assert same(got, got_n) and np.array_equal(ts, ts_n), "padding beyond nlay[p] is read"
    # 5. TMPSFC is in/out: 2.75 for irt 2 and 3, untouched for irt 1
    assert np.all(ts[b.irt != 1] == 2.75) and np.array_equal(ts[b.irt == 1], a0["ts"][b.irt == 1])
    orc, ts_o = tr.oracle(*b.args(a0))
    assert np.array_equal(ts.astype(np.float64), ts_o)
    check_against_truth(f"rtm {name}", kind, b, got, tr.truth(*b.args(a0)), orc)


@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("nlay", [7, 30, 64])
def test_rtm_inf_and_nan_layers_match_the_oracle_pattern(ctx, nlay, kind):
    """A +inf and a NaN optical depth in the middle layer, irt 1, 2, 3 each (G = 2, 8, 16): the NaN pattern of every field is the
    oracle's (exp_cw(-inf) is NaN where libm gives 0, but the optical depth inf - inf is NaN in both; TRTOT = exp(-inf) = 0 in both)
    and whatever the oracle leaves finite agrees with it."""
    r = ctx[kind]
    b = tr.Batch([nlay] * 6, "lognormal", 8100 + nlay)
    O = b.O.copy()
    O[:3, nlay // 2, :] = np.inf
    O[3:, nlay // 2, :] = np.nan
    O[3:, nlay // 2, ::2] = np.inf          # and the two side by side in one wave
    a = b.rounded(r.dtype, 0.0, O=O)
    got, ts = raw_rtm(r, b, a)
    orc, ts_o = tr.oracle(*b.args(a))
    assert np.array_equal(ts.astype(np.float64), ts_o)
    for k in OUT:
        o_k = orc[k].astype(r.dtype)
        assert np.array_equal(np.isnan(got[k]), np.isnan(o_k)), f"{k}: NaN pattern differs from the oracle's"
        fin = ~np.isnan(o_k)
        np.testing.assert_allclose(got[k][fin], o_k[fin], rtol=1e-6 if kind == 8 else SGL_VS_DBL, atol=0, err_msg=k)
    assert np.all(np.isnan(got["rdn"])) and np.all(got["trtot"][:3] == 0) and np.all(got["rup"][b.irt == 3] == 0)


# ---- monortm_hip_rtm_scan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("name,cls", cases())
def test_scan_against_truth(ctx, name, cls, kind):
    """Five paths (tiles of 4 + 1), the same factor for every layer of a path.  The kernel forms tau = (double)O x (double)factor,
    rounded once to double, in both real kinds (rtm_scan_kernel.hip); the truth and the oracle get exactly that product.  The path
    with factor 1 equals monortm_hip_rtm bitwise."""
    r = ctx[kind]
    b = make_batch(name, cls)
    a0, an = b.rounded(r.dtype, 0.0), b.rounded(r.dtype, np.nan)
    f = np.asarray(FACTORS, r.dtype)
    path = np.ascontiguousarray(np.broadcast_to(f[None, :, None], (b.nprof, len(f), b.lm)))
    path_n = path.copy()
    path_n[np.broadcast_to(~b.lay[:, None, :], path.shape)] = np.nan
    got, ts = raw_scan(r, b, a0, path)
    got_n, ts_n = raw_scan(r, b, an, path_n)
    assert same(got, got_n) and np.array_equal(ts, ts_n), "padding beyond nlay[p] is read"
    assert np.all(ts[b.irt != 1] == 2.75) and np.array_equal(ts[b.irt == 1], a0["ts"][b.irt == 1])
    one, ts_1 = raw_rtm(r, b, a0)
    for k in OUT:
        assert np.array_equal(got[k][:, 0], one[k], equal_nan=True), f"{k}: the path with factor 1 is not monortm_hip_rtm's result"
    assert np.array_equal(ts, ts_1)
    truth, orc = {k: [] for k in OUT}, {k: [] for k in OUT}
    for j in range(len(f)):
        Oj = a0["O"].astype(np.float64) * np.float64(f[j])
        t, (o, _) = tr.truth(*b.args(a0, O=Oj)), tr.oracle(*b.args(a0, O=Oj))
        for k in OUT:
            truth[k].append(t[k])
            orc[k].append(o[k])
    truth, orc = {k: np.stack(v, axis=1) for k, v in truth.items()}, {k: np.stack(v, axis=1) for k, v in orc.items()}
    check_against_truth(f"scan {name}", kind, b, got, truth, orc)


# ---- monortm_hip_rtm_jac -----------------------------------------------------------------------------------------------------------
_DERIV = {}


def derivatives(name, cls):
    if (name, cls) not in _DERIV:
        b = make_batch(name, cls)
        a = b.rounded(np.float64, 0.0)
        _DERIV[(name, cls)] = (b, a, tr.truth_derivatives(b, a))
    return _DERIV[(name, cls)]


@pytest.mark.parametrize("quantity", ["rad", "tb"])
@pytest.mark.parametrize("cls", tr.CLASSES)
@pytest.mark.parametrize("name", ["B30", "C12"])
def test_jacobian_against_truth_differences(ctx, name, cls, quantity):
    """rtm_jac_kernel<double, 8> (B30) and <double, 2> (C12): K_O, K_T, K_TZ against Richardson-extrapolated central differences of
    the truth's RAD (good to ~1e-11; for TB times the closed-form dTB/dRAD - tests/rtm_truth.py truth_derivatives says why TB itself
    is not differenced), per (profile, channel) relative to the larger of the column's
    largest derivative and 1e-6 |q| - below that floor a column has no derivative above the rounding of q.  Bound 1e-6 (the bound of
    tests/test_jacobian.py) on every class but `thinnest` and `degenerate`, whose figures are only printed and recorded.  K_SFC
    against the analytic derivatives for irt 1, exactly zero for irt 2 and 3."""
    r = ctx[8]
    b, a, ref = derivatives(name, cls)
    ref = ref[quantity]
    got = raw_jac(r, b, a, quantity)
    got_n = raw_jac(r, b, b.rounded(np.float64, np.nan), quantity)
    assert same(got, got_n), "padding beyond nlay[p] is read"
    fwd, _ = raw_rtm(r, b, a)
    asserted = cls not in tr.CANCELLING
    for k in ("rad", "tb"):   # every class; the same NaNs, and a denormal RAD (`degenerate` only) to 2 of its spacings, not to 1e-12 of it
        np.testing.assert_allclose(got[k], fwd[k], rtol=1e-12, atol=2 * tr.DBL_DENORM, err_msg=k)
    fails = []
    for k in ("k_o", "k_t", "k_tz"):
        e = tr.k_error(got[k], ref[k], ref["q"])
        print(f"jac {name} {cls:14s} {quantity:3s} {k:4s} {e:.1e}")
        tr.record(f"jac/{k}/{cls}/{quantity}", e)
        if asserted and not e <= 1e-6:
            fails.append(f"{k} {e:.2e}")
        assert np.all(got[k][~(b.lev if k == "k_tz" else b.lay)] == 0), f"{k}: padding is not zero"
    one = b.irt == 1
    assert np.all(got["k_sfc"][~one] == 0)
    ks, kr = got["k_sfc"][one].astype(np.longdouble), ref["k_sfc"][one]
    with np.errstate(all="ignore"):
        e = float(np.max(np.abs(ks - kr) / np.maximum(np.abs(kr), np.longdouble(1e-290))))
    print(f"jac {name} {cls:14s} {quantity:3s} k_sfc {e:.1e}")
    tr.record(f"jac/k_sfc/{cls}/{quantity}", e)
    if asserted and not e <= 1e-6:
        fails.append(f"k_sfc {e:.2e}")
    assert not fails, f"{name} {cls} {quantity}: " + ", ".join(fails)
