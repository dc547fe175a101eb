"""Function-level known answers: W4 and SD_Humlicek on grids that straddle every
region boundary (S = 15, 5.5 / 6, y = 0.195|x| - 0.176, +- 2 ulp), SDVOIGT incl. the speed-dependent branch and the
zeta == 1 shortcut, the three RADFN branches with their thresholds, AtoB's end intervals and nodes, ODCLW_TKC.
Expected values: the reference's own functions (tests/golden/make_kat.py compiles src/modm.f90 with its PRIVATE line
removed in a scratch copy).  A region-boundary regression shows up here, localised, before it shows up as one bad
end-to-end fixture.

The reference's "dbl" build evaluates these in REAL*8 / COMPLEX*16 with its literal 7-digit Humlicek coefficients; the
restatements use the same literals, so agreement is at rounding level except where the reference's own formulas cancel
(region IV: cexp(u) - rational)."""
import os

import numpy as np
import pytest

from common import GOLDEN_DIR

KAT = np.load(os.path.join(GOLDEN_DIR, "functions", "kat_functions.npz"))
CASES = [(1, "w4", 2e-12), (2, "sdh", 2e-10), (3, "sdv", 2e-10), (4, "radfn", 1e-14), (5, "atob", 1e-12), (6, "tkc", 1e-12), (7, "tips", 1e-12),
         (8, "hwd", 1e-14), (9, "bbfn", 1e-12)]
# functions with long argument lists (12 per row), held on the CPU restatement only - the device forms the same quantities
# inside line_physics_core() / the class loops, which the fixtures and the fuzz hold to the restatement
WIDE = [(10, "intens", 1e-13), (11, "hwc", 1e-14), (12, "lortz", 1e-12), (13, "sdvlsf", 2e-10)]


def _check(got, key, tol):
    exp = KAT[key + "_out"]
    scale = np.maximum(np.abs(exp), 1e-300)
    if key in ("w4", "sdh"):  # complex: error relative to |w|
        mag = np.maximum(np.hypot(exp[:, 0], exp[:, 1]), 1e-300)[:, None]
        err = np.abs(got - exp) / mag
    else:
        err = np.abs(got[:, :1] - exp[:, :1]) / scale[:, :1]
    if key == "sdv":
        # speed-dependent branch far from the centre: the reference forms w(z1) - w(z2) with |z| ~ sqrt(deltnu / (alphal sdep))
        # and z2 - z1 = 2 sqrt(delta) << |z| (modm.f90:1049-1058) - a cancellation that amplifies the last bit of sqrt by
        # up to ~1e10.  The reference's own value carries that noise, so those rows are held to 1e-4, the rest to `tol`
        a = KAT["sdv_in"]
        ill = (np.abs(a[:, 3]) > 1e-4) & (np.abs(a[:, 0]) > 1e3 * a[:, 1] * np.abs(a[:, 3]))
        err = err / np.where(ill, 1e-4 / tol, 1.0)[:, None]
    worst = int(np.argmax(err.max(axis=1)))
    assert err.max() <= tol, f"{key}: max rel err {err.max():.3g} at args {KAT[key + '_in'][worst]} (got {got[worst]}, want {exp[worst]})"


def test_tips_fixture_covers_every_slot():
    """TIPS_2003(39, T, scor) of the compiled reference at 12 temperatures (limits 70 / 3000 K, nodes, end intervals): every
    (molecule, isotopologue <= 9); molecule 39 comes back as exactly 1 (stale-QT path, src/tips_2003.f90:260-266 + :287-288),
    molecule 34 as 1, slots beyond ISONM untouched (0 in the fixture)."""
    from common import TIPS_ISONM

    a, o = KAT["tips_in"], KAT["tips_out"][:, 0]
    assert len(np.unique(a[:, 0])) >= 8 and {70.0, 296.0, 3000.0} <= set(a[:, 0])
    for mol in range(1, 40):
        for iso in range(1, 10):
            v = o[(a[:, 1] == mol) & (a[:, 2] == iso)]
            assert len(v) >= 8
            if iso <= min(9, TIPS_ISONM[mol - 1]):
                assert (v > 0).all()
                if mol in (34, 39):
                    assert (v == 1.0).all()
            else:
                assert (v == 0).all()
    h2o = o[(a[:, 1] == 1) & (a[:, 2] == 1)]
    assert h2o.max() / h2o.min() > 100     # a real temperature dependence, not a table of ones


def test_fixture_covers_every_region():
    x, y = KAT["w4_in"][:, 0], KAT["w4_in"][:, 1]
    s = np.abs(x) + y
    r4 = (s < 5.5) & (y < 0.195 * np.abs(x) - 0.176)
    assert (s >= 15).sum() >= 20 and ((s >= 5.5) & (s < 15)).sum() >= 20 and ((s < 5.5) & ~r4).sum() >= 20 and r4.sum() >= 20
    # points exactly on and one ulp either side of each boundary
    assert (s == 15.0).any() and (s == 5.5).any() and (s == np.nextafter(15.0, 0)).any() and (s == np.nextafter(5.5, 0)).any()
    sd = KAT["sdv_in"]
    assert (np.abs(sd[:, 3]) > 1e-4).sum() >= 30 and (sd[:, 2] == 0).sum() >= 5
    xr = KAT["radfn_in"]
    q = np.where(xr[:, 1] > 0, xr[:, 0] / np.where(xr[:, 1] > 0, xr[:, 1], 1), np.inf)
    assert (q <= 0.01).sum() >= 3 and ((q > 0.01) & (q <= 10)).sum() >= 3 and (q > 10).sum() >= 3 and (xr[:, 1] <= 0).sum() >= 3


def test_doppler_fixture_covers_every_mass_slot():
    """HALFWHM_D of the compiled reference for every (molecule, isotopologue) TIPS knows: 98 slots (src/isotope.incl:51-167), two
    temperatures - the check that the product's generated mass table is the reference's, without a human in the loop."""
    from common import TIPS_ISONM

    a = KAT["hwd_in"]
    slots = {(int(m), int(i)) for m, i in a[:, :2]}
    assert slots == {(m, i) for m in range(1, 40) for i in range(1, min(9, TIPS_ISONM[m - 1]) + 1)} and len(slots) == 98
    assert (KAT["hwd_out"][:, 0] > 0).all()


@pytest.mark.parametrize("which,key,tol", WIDE)
def test_oracle_wide_functions_match_reference(which, key, tol):
    from oracle import pyoracle

    got, exp = pyoracle.kat_wide(which, KAT[key + "_in"]), KAT[key + "_out"][:, 0]
    if key == "sdvlsf":
        # LSF_SDVOIGT = differences of Voigt values (resonance - pedestal): rows where they cancel are compared relative to the
        # larger of the value and 1e-6 of the central shape
        scale = np.maximum(np.abs(exp), 1e-6 * np.max(np.abs(exp)))
    else:
        scale = np.maximum(np.abs(exp), 1e-300)
    err = np.abs(got - exp) / scale
    worst = int(np.argmax(err))
    assert err.max() <= tol, f"{key}: max rel err {err.max():.3g} at row {worst}: {KAT[key + '_in'][worst]} (got {got[worst]}, want {exp[worst]})"
    if key == "lortz":  # every branch of the shape function is in the fixture: both signs, zeros from the 25 cm-1 rule
        assert (exp == 0).sum() >= 10 and (exp > 0).sum() >= 100 and (exp < 0).sum() >= 1


@pytest.mark.parametrize("which,key,tol", CASES)
def test_oracle_functions_match_reference(which, key, tol):
    from oracle import pyoracle

    _check(pyoracle.kat(which, KAT[key + "_in"], KAT["atob_tab"]), key, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("which,key,tol", CASES)
def test_device_functions_match_reference(which, key, tol):
    from monortm_amd import api

    rt = api.MonoRTM("", 0.0, 0.0)
    try:
        _check(rt.kat(which, KAT[key + "_in"], KAT["atob_tab"]), key, max(tol, 1e-11))
    finally:
        rt.close()


# ---- exp_cw and rcp2 (device_common.hpp): the exp() and 1 / x of the radiance and continuum kernels, KAT rows 10 and 11 ---------------
def _ulps(got, args, fn):
    """|got - fn(arg)| in ulps of the true value (mpmath, 50 digits); a true value below the smallest normal double is measured in
    denormal spacings.  -> (errors, true values as floats)."""
    import mpmath

    err, true = np.zeros(len(args)), np.zeros(len(args))
    with mpmath.workdps(50):
        for i, (g, x) in enumerate(zip(got, args)):
            t = fn(mpmath.mpf(float(x)))
            e = max(int(mpmath.floor(mpmath.log(abs(t), 2))), -1022) - 52
            err[i] = float(abs(mpmath.mpf(float(g)) - t) / mpmath.ldexp(1, e)) if np.isfinite(g) else np.inf
            true[i] = float(t)
    return err, true


def exp_cw_arguments():
    rng = np.random.default_rng(1010)
    ln2 = np.log(2.0)
    ties = []
    for k in range(-1075, 1024):   # the rounding ties of the reduction n = rint(x / ln 2), +- 4 neighbouring doubles
        x = (k + 0.5) * ln2
        lo = x
        for _ in range(4):
            lo = np.nextafter(lo, -np.inf)
        for _ in range(9):
            ties.append(lo)
            lo = np.nextafter(lo, np.inf)
    small = 10.0 ** rng.uniform(-300.0, 0.0, 1000)
    return np.concatenate([rng.uniform(-745.2, 709.78, 4000), small, -small, np.array(ties), [0.0, -0.0, -745.13, -745.2, 709.78]])


@pytest.mark.gpu
def test_device_exp_cw_within_two_ulp():
    """exp_cw is documented at 1-2 ulp: 2 ulp of the true value over the whole range of finite results, 2 denormal spacings below
    2.2e-308; exactly 0 from -745.2 down to -1e9, +inf from 709.79 to 1000, NaN for NaN."""
    import mpmath

    from monortm_amd import api

    x = exp_cw_arguments()
    x = x[(x >= -745.2) & (x <= 709.78)]
    rng = np.random.default_rng(1011)
    zero = np.concatenate([[-745.2, -746.0, -800.0, -1e9], -10.0 ** rng.uniform(np.log10(745.2), 9.0, 500)])
    inf = np.concatenate([[709.79, 1000.0], rng.uniform(709.79, 1000.0, 200)])
    args = np.zeros((len(x) + len(zero) + len(inf) + 1, 4))
    args[:, 0] = np.concatenate([x, zero, inf, [np.nan]])
    rt = api.MonoRTM("", 0.0, 0.0)
    try:
        got = rt.kat(10, args)[:, 0]
    finally:
        rt.close()
    err, true = _ulps(got[:len(x)], x, mpmath.exp)
    w = int(np.argmax(err))
    print(f"\nexp_cw: worst {err.max():.3f} ulp at x = {x[w]!r} ({len(x)} arguments); worst for results below 2.2e-308: "
          f"{err[true < 2.2250738585072014e-308].max():.3f} denormal spacings")
    assert err.max() <= 2.0, f"exp_cw({x[w]!r}) = {got[w]!r}: {err.max():.3f} ulp from {true[w]!r}"
    z, i = got[len(x):len(x) + len(zero)], got[len(x) + len(zero):-1]
    assert np.all(z == 0) and not np.any(np.signbit(z)), "exp_cw below -745.2 is not exactly +0"
    assert np.all(i == np.inf), "exp_cw above 709.79 is not +inf"
    assert np.isnan(got[-1])


@pytest.mark.gpu
def test_device_rcp2_within_one_ulp():
    """rcp2 (v_rcp_f64 and two Newton steps) is documented at 1 ulp: +-10^U(-300, 300), and 1 + 10^U(-16, 0), the range of the
    radiance kernels' 1 + pade."""
    import mpmath

    from monortm_amd import api

    rng = np.random.default_rng(1012)
    big = 10.0 ** rng.uniform(-300.0, 300.0, 3000)
    x = np.concatenate([big, -big, 1.0 + 10.0 ** rng.uniform(-16.0, 0.0, 3000), [1.0, 2.0, 3.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52]])
    args = np.zeros((len(x), 4))
    args[:, 0] = x
    rt = api.MonoRTM("", 0.0, 0.0)
    try:
        got = rt.kat(11, args)[:, 0]
    finally:
        rt.close()
    err, true = _ulps(got, x, lambda v: 1 / v)
    w = int(np.argmax(err))
    print(f"\nrcp2: worst {err.max():.3f} ulp at x = {x[w]!r} ({len(x)} arguments)")
    assert err.max() <= 1.0, f"rcp2({x[w]!r}) = {got[w]!r}: {err.max():.3f} ulp from {true[w]!r}"
    assert np.all(got[-5:-2] == [1.0, 0.5, 1.0 / 3.0])
