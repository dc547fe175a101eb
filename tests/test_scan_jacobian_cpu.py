"""Jacobians of path scans (monortm_hip_rtm_scan_jac, monortm_hip_scan_jacobian), the part that needs no GPU:
the four entry points are declared, bound and exported; and the premise of the full entry on the CPU oracle - the central
differences of MODM that monortm_hip_jacobian forms do not depend on the path but for the factor: on amounts scaled by s they are s
times the differences on the vertical amounts."""
import copy
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from common import ROOT
from monortm_amd import _build, api, synth, tape3

SYMBOLS = {"monortm_hip_rtm_scan_jac": 24, "monortm_hip_rtm_scan_jac_dev": 25, "monortm_hip_scan_jacobian": 39,
           "monortm_hip_scan_jacobian_dev": 41}   # name: arguments


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "monortm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_build.build_hip())
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/monortm_hip.h"
        assert name in api.SYMBOLS, f"{name} is not bound in api.SYMBOLS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert len(m.group(1).split(",")) == nargs == len(api.SYMBOLS[name][1]), name
    assert api.SCAN_JAC_RTM_FIELDS == ("rad", "tb", "k_o", "k_path", "k_t", "k_tz", "k_sfc")
    assert api.SCAN_JAC_FIELDS == ("o", "rad", "tb", "k_t", "k_tz", "k_w", "k_clw", "k_o", "k_path", "k_sfc")


@pytest.fixture(scope="module")
def oracle_case(workdir):
    """The case of tests/test_scan_cpu.py: the line list and channels of tests/test_jacobian.py::case."""
    from oracle.pyoracle import Oracle

    t3 = f"{workdir}/TAPE3_scan_jac_cpu"
    tape3.write_tape3(t3, synth.synthetic_lines(300, seed=777, lc_frac=0.5, sdep_frac=0.2))
    wn = np.unique(np.concatenate([synth.c2_channels(12, seed=11), synth.sounder_channels()]))
    orc = Oracle(t3, wn[0], wn[-1])
    yield wn, orc
    orc.close()


def scaled(pr, s):
    """The profile with every amount of layer l multiplied by s[l]; P, T, TZ as they were."""
    q = copy.deepcopy(pr)
    s = np.asarray(s, np.float64)
    q.wkl, q.wbrodl, q.clw = pr.wkl * s[:, None], pr.wbrodl * s, pr.clw * s
    return q


def modm_differences(orc, pr, mols):
    """The difference quotients monortm_hip_jacobian forms from its perturbed states, on the oracle's MODM: d O / d T at T +- JAC_DT
    and d O / d ln WKL_m at WKL_m (1 +- JAC_DLNW), [1 + len(mols)][nlay][nwn]."""
    def o(**kw):
        p = copy.deepcopy(pr)
        for k, v in kw.items():
            setattr(p, k, v)
        return orc.run(p).o

    out = [(o(t=pr.t + api.JAC_DT) - o(t=pr.t - api.JAC_DT)) * (0.5 / api.JAC_DT)]
    for m in mols:
        wp, wm = pr.wkl.copy(), pr.wkl.copy()
        wp[:, m - 1] *= 1.0 + api.JAC_DLNW
        wm[:, m - 1] *= 1.0 - api.JAC_DLNW
        out.append((o(wkl=wp) - o(wkl=wm)) * (0.5 / api.JAC_DLNW))
    return np.array(out)


# measured on the oracle (worst over the three profiles and the three differences, per_layer factors in [1, 6]); the bound is 100 x
# that, the margin for other libm builds
MEASURED = 1.2e-6
BOUND = 100 * MEASURED


@pytest.mark.parametrize("kind", ["uniform", "per_layer"])
def test_premise_modm_differences_scale_with_the_path(oracle_case, kind):
    """What the full entry rests on (and tests/test_scan_jacobian.py's comparison with MonoRTM.jacobian on scaled amounts): the
    central differences of MODM on amounts scaled per layer by s equal s x the differences on the vertical amounts.  What differs is
    the rounding of the TOTAL O (8.9e-16 relative, tests/test_scan_cpu.py) divided by the step.  Worst relative difference on the
    per-channel layer-max scale, measured with per_layer factors: d/dT 1.2e-11, d/dlnW of H2O 4.7e-12, d/dlnW of O3 1.2e-6 (O3 holds
    ~1e-6 of O in these channels, so 1e-16 O / (2 x 1e-4) is 1e-6 of ITS difference: the case the w_floor of the K_W comparisons is
    for); with uniform s = 2, an exact scaling, 0.  MEASURED = 1.2e-6, the worst of them; asserted: 100 x that = 1.2e-4."""
    wn, orc = oracle_case
    rng = np.random.default_rng(4)
    worst = np.zeros(3)   # d / dT, d / d ln WKL of molecules 1 and 3
    for i, irt in zip((500, 501, 502), (1, 3, 2)):
        pr = synth.perturbed_profile(i, wn, nlay=20, cloud=True, irt=irt)
        s = np.full(20, 2.0) if kind == "uniform" else rng.uniform(1.0, 6.0, 20)
        want = modm_differences(orc, pr, (1, 3)) * s[None, :, None]
        got = modm_differences(orc, scaled(pr, s), (1, 3))
        scale = np.abs(want).max(axis=1, keepdims=True)
        assert np.all(scale > 0)
        worst = np.maximum(worst, np.max(np.abs(got - want) / scale, axis=(1, 2)))
    print(f"premise of the full entry ({kind}): worst relative difference d/dT {worst[0]:.2e}, d/dlnW(1) {worst[1]:.2e}, d/dlnW(3) {worst[2]:.2e}")
    assert worst.max() <= BOUND


# ---- the reference of tests/test_scan_jacobian.py::test_adjoint_matches_oracle_differences, downwelling case -----------------------
RADCN1, RADCN2 = 1.191042722E-12, 1.4387752   # src/PhysConstants.f90


def _bb(v, t):
    return RADCN1 * v ** 3 / (np.exp(v * RADCN2 / t) - 1.0)


def _rad_down(pr, tau):
    """RAD for irt = 3 (RDN + TRTOT x COSMOS, src/RTMmono.f90:207-218, :147) in numpy; tau [nlay, nwn] may be complex."""
    v, odt, rdn = pr.wn, tau.sum(0), 0.0
    odtot = odt.copy()
    for l in range(pr.nlay - 1, -1, -1):
        od = tau[l]
        odt = odt - od
        pade = 0.193 * od + 0.013 * od ** 2
        rdn = rdn + np.exp(-odt) * (1.0 - np.exp(-od)) * (_bb(v, pr.t[l]) + pade * _bb(v, pr.tz[l])) / (1.0 + pade)
    return rdn + np.exp(-odtot) * _bb(v, 2.75)


def _orc_rad(pr, o):
    from oracle.pyoracle import lib

    nwn = pr.nwn
    rup, rdn, trtot, rad, tb = (np.zeros(nwn) for _ in range(5))
    ts = ctypes.c_double(pr.tmpsfc)
    lib().orc_rtm(1, pr.irt, nwn, pr.wn, pr.nlay, np.ascontiguousarray(pr.t), np.ascontiguousarray(pr.tz), np.ascontiguousarray(o),
                  ctypes.byref(ts), rup, trtot, rdn, np.ascontiguousarray(pr.reflc), np.ascontiguousarray(pr.emiss), rad, tb)
    return rad


def test_difference_quotient_of_the_downwelling_case_resolves_k_o(oracle_case):
    """The GPU test compares the adjoint at 1e-6 with Richardson-extrapolated central differences of the oracle's RTM.  In opaque
    channels downwelling radiance saturates: the largest |dRAD/dO_k| of a column is ~1e-4 of RAD, and a quotient with step 1e-4
    resolves it to ~10 ulp(RAD) / 1e-4 ~ 1e-7 .. 1e-6 of it.  Here: the quotient's own error for the profile that test uses (306)
    against the exact derivative by the complex step, by the same rel_err, with O changed in its last bits (the GPU's O differs from
    the oracle's there).  Measured: 1.3e-7 worst of 6 draws (profile 303 with the same factors: up to 1.1e-6); asserted: 5e-7, half
    the GPU test's bound."""
    wn, orc = oracle_case
    pr = synth.perturbed_profile(306, wn, nlay=20, cloud=True, irt=3)
    fac = np.random.default_rng(63).uniform(1.0, 6.0, 20)
    o0 = orc.run(pr).o
    np.testing.assert_allclose(_rad_down(pr, fac[:, None] * o0), _orc_rad(pr, fac[:, None] * o0), rtol=1e-13)
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(3):
        o = o0 * (1.0 + 2e-16 * rng.integers(-3, 4, o0.shape))
        truth, fd = np.zeros_like(o), np.zeros_like(o)
        for k in range(20):
            t = (fac[:, None] * o).astype(complex)
            t[k] += 1j * 1e-30 * fac[k]
            truth[k] = _rad_down(pr, t).imag / 1e-30
            h, d = 1e-4 * max(float(o[k].max()), 1.0), []
            for hh in (h, 2 * h):
                q = []
                for sgn in (1, -1):
                    oo = o.copy()
                    oo[k] += sgn * hh
                    q.append(_orc_rad(pr, fac[:, None] * oo))
                d.append((q[0] - q[1]) / (2 * hh))
            fd[k] = (4 * d[0] - d[1]) / 3
        worst = max(worst, float(np.max(np.abs(fd - truth) / np.abs(truth).max(axis=0, keepdims=True))))
    print(f"difference quotient of the downwelling case: own error {worst:.2e}")
    assert worst <= 5e-7


def test_scan_jacobian_bench_builds_its_workload():
    """tools/scan_jacobian_bench.py imports, and its workload is the headline batch of bench.py (configs[3]): everything the tool does
    before it needs the GPU."""
    spec = importlib.util.spec_from_file_location("scan_jacobian_bench", os.path.join(ROOT, "tools", "scan_jacobian_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec, profs, desc = mod.workload()
    assert len(profs) == 1024 and profs[0].nlay == 64 and profs[0].nwn == 50 and rec.n_physical == 500
    assert "configs[3]" in desc
    assert mod.stats([1.0, 2.0, 3.0, 4.0, 10.0]) == dict(median=3.0, min=1.0, max=10.0, iqr=2.0, n=5)
