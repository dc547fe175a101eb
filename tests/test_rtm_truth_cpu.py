"""What tests/test_rtm_extremes.py leans on, checked without a GPU: the CPU oracle's RTM / CALCTMR (the project's restatement of the
reference loop, in double) against the extended-precision truth of tests/rtm_truth.py on every input class.

E_orc = E(oracle, truth) is the REFERENCE's own error on a class.  It must be small (<= 1e-7, a tenth of the project's 1e-6 criterion)
wherever the GPU tests hold the kernels to the oracle at 1e-6; only `thinnest` and `degenerate` may lie outside - there the reference's
1 - exp(-tau) cancels (tau = 1e-12 keeps 4 digits).  And what tests/test_adjoint_extremes.py leans on: the truth's closed-form adjoint
(truth_adjoint) against Richardson differences of the truth.  Run with -s for the tables."""
import numpy as np
import pytest

import common  # noqa: F401  (puts the repository root on sys.path)
import rtm_truth as rt

# layer counts 1 .. 200: 12 profiles x 70 wavenumbers = 840 columns per class and kind, irt cycling 1, 2, 3
NLAY = [1, 2, 3, 5, 8, 13, 24, 48, 64, 100, 150, 200]


def e_orc(cls, kind, seed=1000):
    b = rt.Batch(NLAY, cls, seed + rt.CLASSES.index(cls))
    a = b.rounded(np.float64 if kind == 8 else np.float32)     # kind 4: the oracle and the truth get what a float context receives
    tr = rt.truth(*b.args(a))
    orc, ts = rt.oracle(*b.args(a))
    assert np.all(ts[b.irt != 1] == 2.75) and np.array_equal(ts[b.irt == 1], np.float64(a["ts"])[b.irt == 1])
    return {k: rt.E(orc[k], tr[k], orc[k], denormal_slack=k == "trtot") for k in rt.OUT}, b, tr, orc


@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("cls", rt.CLASSES)
def test_oracle_error_per_class(cls, kind):
    errs, b, tr, orc = e_orc(cls, kind)
    print(f"\nE_orc {cls:14s} inputs of real_kind {kind}: " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        rt.record(f"E_orc/{cls}/{kind}/{k}", v)
    rt.dump_record()
    if cls not in rt.CANCELLING:
        bad = {k: v for k, v in errs.items() if not v <= 1e-7}
        assert not bad, f"{cls}: the oracle is further than 1e-7 from the truth: {bad}"
    if cls == "thinnest":   # the cancellation is where it is expected, and nowhere else: TRTOT, TB and TMR's ratio keep their digits
        assert errs["trtot"] <= 1e-12 and 1e-7 < errs["rup"] <= 1e-3 and 1e-7 < errs["rdn"] <= 1e-3


def test_restatement_is_the_same_operation():
    """The extended-precision restatement agrees with the oracle to 1e-12 on well-conditioned columns (lognormal, 1e-5 .. 5), all
    six fields, every irt: it states the operation of RTMmono.f90:13-325 and no other."""
    errs, b, tr, orc = e_orc("lognormal", 8, seed=2000)
    assert max(errs.values()) <= 1e-12, errs
    assert set(b.irt) == {1, 2, 3} and np.all(tr["rup"][b.irt == 3] == 0) and np.all(orc["rup"][b.irt == 3] == 0)


def test_truth_ignores_padding_and_takes_extended_inputs():
    b = rt.Batch(rt.BATCHES["A64"], "mixed", 5)
    z, n = b.rounded(np.float64, 0.0), b.rounded(np.float64, np.nan)
    tz, tn = rt.truth(*b.args(z)), rt.truth(*b.args(n))
    for k in rt.OUT:
        assert np.array_equal(tz[k], tn[k]) and tz[k].dtype == np.longdouble
    # a perturbation below double resolution changes the result: the inputs are not rounded to double on the way in
    O = np.asarray(z["O"], np.longdouble)
    O2 = O.copy()
    O2[:, 0] = O2[:, 0] * (1 + np.longdouble(1e-18))
    assert np.any(rt.truth(*b.args(z, O=O2))["rdn"] != rt.truth(*b.args(z, O=O))["rdn"])


def test_error_measure_rules():
    ld = np.longdouble
    t = np.array([1.0, 1e-320, 0.0, np.nan], ld)
    orc = np.array([1.0, 1e-320, 0.0, np.nan])
    assert rt.E(np.array([1.0 + 1e-9, 1e-320, 0.0, np.nan]), t, orc) == pytest.approx(1e-9, rel=1e-3)
    assert rt.E(np.array([1.0, 0.0, 0.0, np.nan]), t, orc, denormal_slack=True) > 0.99   # 1e-320 is 2000 denormal spacings from 0
    two = np.array([1.0, 1e-320 + 1e-323, 0.0, np.nan])
    assert rt.E(two, t, orc, denormal_slack=True) == 0.0 and rt.E(two, t, orc) > 9e-4    # two of them are free for TRTOT alone
    assert rt.E(np.array([1.0, 1e-320, 1e-300, np.nan]), t, orc) == np.inf     # truth 0: must equal the oracle
    assert rt.E(np.array([1.0, 1e-320, 0.0, 0.0]), t, orc) == np.inf           # NaN where the oracle has NaN
    assert rt.E(np.array([np.nan, 1e-320, 0.0, np.nan]), t, orc) == np.inf
    t4 = np.array([1.0, 1e-33], ld)
    assert rt.E(np.array([1.0, 0.0], np.float32), t4, np.array([1.0, 1e-33]), 4) == 0.0
    assert rt.E(np.array([1.0, 3e-30], np.float32), t4, np.array([1.0, 1e-33]), 4) == np.inf


def test_classes_are_what_they_say():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 30):
        o = {c: rt.optical_depths(c, rng, n) for c in rt.CLASSES}
        assert all(v.shape == (n, rt.NWN) and np.all(v >= 0) for v in o.values())
        third = (n + 2) // 3
        assert np.all(o["opaque_bottom"][:third] >= 100) and np.all(o["opaque_top"][n - third:] >= 100)
        assert np.all(o["opaque_middle"][n // 2] == 1e6) and np.all(o["underflow"] >= 745)
        assert o["thinnest"].max() <= 1e-8 and o["thin"].max() <= 1e-4 and o["mixed"].min() >= 1e-8
    d = rt.optical_depths("degenerate", rng, 30)
    assert (d == 0).any() and ((d > 0) & (d < rt.DBL_TINY)).any() and (d >= 1e-300).any()
    assert len(rt.WN) == 70 and rt.WN[0] == 0.5 and abs(rt.WN[-1] - 57000.0) < 1e-9
    cyc = rt.cycled_classes(140)
    assert {(c, i % 3) for i, c in enumerate(cyc)} == {(c, i) for c in rt.CLASSES for i in range(3)}


def test_closed_form_dtb_drad_matches_differences_of_tb():
    """truth_derivatives forms the derivatives of TB as those of RAD times dTB/dRAD in closed form.  That factor is held here to
    Richardson-extrapolated central differences of TB(RAD) = RADCN2 v / log1p(c3 / RAD) itself, step 1e-4 RAD (relative, so it
    resolves at every magnitude of RAD), over every class's radiances.  Bound 1e-10: the differences round at eps / h x ln(1 + c3 / RAD)
    <= 1.1e-19 / 1e-4 x 1e3 = 1e-12 and truncate at h^4 = 1e-16 times a modest constant; the GPU test's bound is 1e-6."""
    ld = np.longdouble
    for cls in rt.CLASSES:
        b = rt.Batch(rt.BATCHES["B30"], cls, 3000 + rt.CLASSES.index(cls))
        a = b.rounded(np.float64)
        t0 = rt.truth(*b.args(a))
        rad, c3, v = t0["rad"], t0["c3"], np.asarray(b.wn, ld)[None, :]
        ok = np.isfinite(rad) & (rad > 0)
        tb = lambda r: rt.RADCN2 * v / np.log1p(c3 / r)  # noqa: E731
        with np.errstate(all="ignore"):
            d = [(tb(rad * (1 + h)) - tb(rad * (1 - h))) / (2 * h * rad) for h in (ld(1e-4), ld(2e-4))]
            want = (4 * d[0] - d[1]) / 3
            got = rt.dtb_drad(rad, c3, v)
            err = np.abs(got - want)[ok] / np.abs(want)[ok]
        assert ok.sum() > 0.3 * ok.size and err.max() <= 1e-10, (cls, float(err.max()))


# ---- the analytic adjoint of the truth ---------------------------------------------------------------------------------------------
# The worst k_error of truth_adjoint against truth_derivatives over k_o, k_t, k_tz, RAD and TB, B30 and C12, measured on the CPU
# (LABNOTES section 23 has the table by field).  What is measured is the DIFFERENCES' error: 1e-10 is their truncation
# (x / T)^5 h^4 on k_t / k_tz, 1e-9 the rounding eps RAD / h of k_o where an opaque layer leaves a column's largest dRAD/dtau at
# 1e-3 RAD.  The two functions share truth() and dtb_drad and nothing else.
ADJOINT_MEASURED = {"lognormal": 1.1e-10, "thin": 1.6e-10, "thinnest": 1.2e-10, "opaque_bottom": 1.3e-9, "opaque_top": 1.5e-9,
                    "opaque_middle": 6.9e-11, "mixed": 1.6e-9, "underflow": 8.0e-10, "degenerate": 9.6e-11}


@pytest.mark.parametrize("cls", rt.CLASSES)
@pytest.mark.parametrize("name", ["B30", "C12"])
def test_truth_adjoint_against_truth_differences(name, cls):
    """truth_adjoint (closed form) against truth_derivatives (Richardson-extrapolated central differences of truth()), by k_error.
    Bound outside CANCELLING: 10 x the class's measured worst, and never looser than 1e-8 - two decades inside the 1e-6 the kernels
    are held to; `thinnest` and `degenerate` are printed and recorded.  K_SFC: the two share the closed form, so equal.  Padded
    layers and levels are exactly 0 and NaN beyond nlay[p] changes no bit."""
    b = rt.make_batch(name, cls)
    a = b.rounded(np.float64, 0.0)
    ref, got = rt.truth_derivatives(b, a), rt.truth_adjoint(*b.args(a))
    got_n = rt.truth_adjoint(*b.args(b.rounded(np.float64, np.nan)))
    bound = min(10 * ADJOINT_MEASURED[cls], 1e-8)
    fails = []
    for q in ("rad", "tb"):
        for k in ("k_o", "k_t", "k_tz", "k_sfc", "q"):
            assert got[q][k].dtype == np.longdouble and np.array_equal(got[q][k], got_n[q][k]), f"{q} {k}: padding beyond nlay[p] is read"
        for k in ("k_o", "k_t", "k_tz"):
            assert np.all(got[q][k][~(b.lev if k == "k_tz" else b.lay)] == 0), f"{q} {k}: padding is not zero"
            e = rt.k_error(got[q][k], ref[q][k], ref[q]["q"])
            print(f"truth_adjoint {name} {cls:14s} {q:3s} {k:4s} {e:.1e}")
            rt.record(f"truth_adjoint/{k}/{cls}/{q}", e)
            if cls not in rt.CANCELLING and not e <= bound:
                fails.append(f"{q} {k} {e:.2e} > {bound:.1e}")
        assert np.array_equal(got[q]["k_sfc"], ref[q]["k_sfc"]) and np.all(got[q]["k_sfc"][b.irt != 1] == 0)
        assert np.array_equal(got[q]["q"], ref[q]["q"])
    rt.dump_record()
    assert not fails, f"{name} {cls}: " + ", ".join(fails)
