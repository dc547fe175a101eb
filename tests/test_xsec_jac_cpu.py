"""Why xsec_jac_kernel exists, and that its definition is sound - on the CPU, with the oracle, on the three profiles of tests/xsec_cases.py
(call `all`, 2512 live cells).

The Jacobians difference optical depths at T +- 1e-2 K and P (1 +- 1e-4).  For the cross sections that cannot be xsec_kernel re-run at
those states: MONORTM_XSEC_SUB re-grids the spectrum when P or T moves (npts = int((v2x - v1x) / step)), and the stopping trip, the
bracket, the clamps and the branches move too.  What works is the base state's finite sum evaluated at the perturbed state
(tests/xsec_jac_truth.py).

1. the restatement at the base state IS the oracle's ODXSEC (<= 1e-12 of the layer's maximum), trip for trip;
2. its differences at the kernel's own steps are within the project's 1e-6 of the Richardson reference on every live cell;
3. the recorded finding: plain differences of the oracle at those steps disagree between h and 2 h by more than 1e-6 on at least a
   quarter of the live cells of every profile.

Measured (worst of the three profiles): 1. 4.5e-15 (the sums in long double on the reference's own grid points; the same restatement
in plain double: 2.1e-13), 974 / 375 / 615 walked cells with the oracle's trip count; 2. T 2.2e-9, ln P 9.5e-9, the Richardson
references' self-spread <= 1.2e-11; 3. T 36 - 54 %, ln P 46 - 58 % of the cells, the worst disagreement 5 x (T) and 540 x (ln P) the
layer's largest derivative.
"""
import os
import re

import numpy as np
import pytest

import xsec_cases as xc
import xsec_jac_truth as xt

TOL = 1e-6
PROFILES = range(len(xc.NLAYS))
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monortm_hip.h")


def test_header_code_equals_the_python_code():
    """MONORTM_JVAR_XS0 of the C header, api.JVAR_XS0 and "xs:<NAME>" name the same codes; they lie beyond every code of api.JAC_VARS."""
    from monortm_amd import api

    m = re.search(r"^#define\s+MONORTM_JVAR_XS0\s+\(?(\d+)\)?", open(HEADER).read(), re.M)
    assert m and int(m.group(1)) == api.JVAR_XS0 == 1101
    assert api.JVAR_XS0 > max(api.JAC_VARS.values())
    assert api.jac_codes(("xs:f12", 1, "p", api.JVAR_XS0 + 4), xc.NAMES).tolist() == [api.JVAR_XS0 + 2, 1, api.JAC_VARS["p"], api.JVAR_XS0 + 4]
    with pytest.raises(ValueError):
        api.jac_codes(("xs:SF6",), xc.NAMES)
    with pytest.raises(ValueError):
        api.jac_codes(("xs:F11",))


@pytest.mark.parametrize("i", PROFILES)
def test_frozen_evaluation_at_the_base_state_is_the_oracle(i):
    orc = xc.oracle(8)
    fz = xt.frozen(i)
    exp = orc.odx["all"][i]
    got = np.asarray(fz.odxsec(), np.float64)
    assert exp.any() and not got[exp == 0].any()
    e = np.abs(got - exp) / xt.layer_scale(exp)
    print(f"profile {i}: frozen evaluation at the base state against the oracle, max {e.max():.2e} of the layer's maximum")
    assert e.max() <= 1e-12
    tr, walked = orc.trace[i], 0
    for k in range(fz.pr.nlay):
        for iw in range(len(xc.WN)):
            for r, pl in enumerate(fz.plans[k][iw]):
                b = xc_branch(tr, r, k, iw)
                assert (pl is None) == (b in ("unprocessed", "outside")), (i, k, iw, r, b)
                if pl is None:
                    continue
                assert pl.walk == (b == "walk"), (i, k, iw, r, b)
                if pl.walk and tr.crit_margin[r, k, iw] >= xc.MIN_CRIT:
                    assert pl.trips == tr.trips[r, k, iw], (i, k, iw, r, pl.trips, int(tr.trips[r, k, iw]))
                    walked += 1
    print(f"profile {i}: {walked} walked cells stop at the oracle's trip")
    assert walked > 100


def xc_branch(tr, r, k, iw) -> str:
    from oracle import pyoracle

    return pyoracle.XS_BRANCHES[int(tr.branch[r, k, iw])]


@pytest.mark.parametrize("i", PROFILES)
def test_frozen_differences_at_the_kernels_steps_match_richardson(i):
    fz = xt.frozen(i)
    live = xc.oracle(8).odx["all"][i] != 0
    for var, h, mul in (("t", xt.KERNEL_DT, False), ("p", xt.KERNEL_DLNW, True)):
        ref, half = fz.richardson(var)
        d = np.asarray(fz.central(var, h, mul=mul), np.float64)
        sc = xt.layer_scale(ref)
        e, spread = (np.abs(d - ref) / sc)[live].max(), (np.abs(half - ref) / sc)[live].max()
        print(f"profile {i} d/d{'T' if var == 't' else ' ln P'}: frozen difference at h = {h:g} against Richardson {e:.2e} "
              f"(self-spread {spread:.1e}), {int(live.sum())} live cells, {np.mean(d[live] != 0):.0%} of them not zero")
        assert spread <= 1e-7, "the reference does not settle"
        assert e <= TOL
        assert np.mean(d[live] != 0) > 0.5


@pytest.mark.parametrize("i", PROFILES)
def test_plain_differences_of_the_oracle_do_not_converge(i):
    """The finding that rules out the obvious implementation; the assertion keeps it in the record."""
    from oracle import pyoracle

    orc = xc.oracle(8)
    pr = orc.profs["all"][i]
    live = orc.odx["all"][i] != 0

    def odx(p, t):
        return pyoracle.xsec_trace(xc.WN, p, t, orc.tabs, pr.xamnt, trace=False)[0]

    for var, h in (("T", xt.KERNEL_DT), ("ln P", xt.KERNEL_DLNW)):
        def central(s):
            if var == "T":
                return (odx(pr.p, pr.t + s * h) - odx(pr.p, pr.t - s * h)) / (2 * s * h)
            return (odx(pr.p * (1 + s * h), pr.t) - odx(pr.p * (1 - s * h), pr.t)) / (2 * s * h)

        d1, d2 = central(1.0), central(2.0)
        e = (np.abs(d1 - d2) / xt.layer_scale(d1))[live]
        print(f"profile {i} d/d{var}: central differences of the oracle at h and 2 h disagree by more than 1e-6 of the layer's largest "
              f"derivative in {np.mean(e > TOL):.0%} of {int(live.sum())} live cells, worst {e.max():.3g}")
        assert np.mean(e > TOL) >= 0.25
