"""The forward measurement operator (monortm_hip_rtm_obs, monortm_hip_obs), the part that needs no GPU: the
band brightness temperature helpers, what the Python wrappers refuse before any library call, and the premise of the GPU test's
end-to-end comparison on the CPU oracle."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import obs_cases as oc
from common import ROOT
from monortm_amd import api, synth, tape3
from test_scan_cpu import scaled

U = 2.0 ** -53


def _orc_rtm(pr, o):
    """(RAD, TB) of the oracle's RTM on optical depths o [nlay, nwn]."""
    from oracle.pyoracle import lib

    nwn = pr.nwn
    rup, rdn, trtot, rad, tb = (np.zeros(nwn) for _ in range(5))
    ts = ctypes.c_double(pr.tmpsfc)
    lib().orc_rtm(1, pr.irt, nwn, pr.wn, pr.nlay, np.ascontiguousarray(pr.t), np.ascontiguousarray(pr.tz), np.ascontiguousarray(o),
                  ctypes.byref(ts), rup, trtot, rdn, np.ascontiguousarray(pr.reflc), np.ascontiguousarray(pr.emiss), rad, tb)
    return rad, tb


@pytest.fixture(scope="module")
def oracle_case(workdir):
    """The case of tests/test_scan_cpu.py: the line list and channels of tests/test_jacobian.py::case."""
    from oracle.pyoracle import Oracle

    t3 = f"{workdir}/TAPE3_obs_fwd_cpu"
    tape3.write_tape3(t3, synth.synthetic_lines(300, seed=777, lc_frac=0.5, sdep_frac=0.2))
    wn = np.unique(np.concatenate([synth.c2_channels(12, seed=11), synth.sounder_channels()]))
    orc = Oracle(t3, wn[0], wn[-1])
    yield wn, orc
    orc.close()


def formula_bound(vcen, rad):
    """Relative rounding error of ONE evaluation pair of TB = RADCN2 v / log(x + 1), x = RADCN1 v^3 / rad, in IEEE double with
    u = 2^-53: the rounding of x + 1 moves log(x + 1) by u relative to 1, that is by u / log(1 + x) <= u (1 + 1/x) relative to the
    logarithm (log(1 + x) >= x / (1 + x)); the rounding of x itself moves it by less than that; the logarithm's own rounding and the
    division add u each: <= 2 u (1 + 1/x) per evaluation, 4 u (1 + 1/x) between two of them."""
    x = api.RADCN1 * np.asarray(vcen) ** 3 / np.asarray(rad)
    return 4 * U * (1.0 + 1.0 / x)


def test_band_tb_of_one_sample_is_the_monochromatic_tb(oracle_case):
    """Identity operator, vcen = wn: the band TB of a one-sample channel IS the monochromatic TB.  api.band_tb on the oracle's RAD
    against the oracle's own TB, relative, at 4 x 2^-53 (1 + 1/x) (formula_bound)."""
    wn, orc = oracle_case
    worst = 0.0
    for i, irt in zip((500, 501, 502), (1, 3, 2)):
        pr = synth.perturbed_profile(i, wn, nlay=20, cloud=True, irt=irt)
        o = orc.run(pr).o
        for s in (1.0, 3.7):
            rad, tb = _orc_rtm(pr, s * o)
            got = api.band_tb(wn, rad[None, :])[0]
            ratio = np.abs(got - tb) / tb / formula_bound(wn, rad)
            worst = max(worst, float(ratio.max()))
            assert np.all(ratio <= 1.0), float(ratio.max())
    print(f"band_tb against the oracle's TB: worst error / bound = {worst:.2f}")


def test_band_tb_slope_is_the_derivative(oracle_case):
    """band_tb_slope against a central difference of band_tb in t = ln(rad), rad e^(+-eta) with eta = 1e-5.  With L = log(1 + x),
    s = x / (1 + x) (s <= L) and g = d TB / dt = rad x slope = RADCN2 v s / L^2:  g' = g p, p = -(1 - s) + 2 s / L in [-1, 2], and
    g'' = g (p^2 + p') with |p'| <= 1/4 + 2 + 2, so |g''| <= 8.25 g and the truncation eta^2 g'' / 6 is below 1.4 eta^2 g.  Rounding:
    each of the two values carries formula_bound / 2 of TB and the rounding of its argument (u g), divided by 2 eta, relative to
    g = TB s / L:  (formula_bound L / s / 2 + u) / eta.  8 u for the slope's own operations."""
    wn, orc = oracle_case
    pr = synth.perturbed_profile(500, wn, nlay=20, cloud=True, irt=1)
    rad, _ = _orc_rtm(pr, orc.run(pr).o)
    rad = np.stack([rad, 0.01 * rad, 30.0 * rad])          # towards the Wien side and beyond any radiance of the atmosphere
    eta = 1e-5
    diff = (api.band_tb(wn, rad * np.exp(eta)) - api.band_tb(wn, rad * np.exp(-eta))) / (2 * eta)
    got = api.band_tb_slope(wn, rad) * rad
    x = api.RADCN1 * wn ** 3 / rad
    L, s = np.log1p(x), x / (1.0 + x)
    bound = 1.4 * eta ** 2 + (0.5 * formula_bound(wn, rad) * L / s + U) / eta + 8 * U
    ratio = np.abs(got - diff) / np.abs(got) / bound
    print(f"band_tb_slope against the central difference: worst error / bound = {float(ratio.max()):.2f} (bound up to {float(bound.max()):.1e})")
    assert np.all(got > 0) and np.all(ratio <= 1.0)
    # the recipe of INTEGRATION 5f keeps the leading axes
    assert api.band_tb_slope(wn, rad[None])[..., None, :].shape == (1, 3, 1, len(wn))


def test_band_tb_zero_and_nan_rules():
    v = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    rad = np.array([[1e-13, 0.0, -1e-13, np.nan, np.inf]])
    for fn in (api.band_tb, api.band_tb_slope):
        got = fn(v, rad)
        assert got.shape == (1, 5) and got[0, 0] > 0 and got[0, 1] == 0.0 and np.all(np.isnan(got[0, 2:]))
    for bad in ([1.0, 0.0, 1.0, 1.0, 1.0], [1.0, -2.0, 1.0, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0, 1.0], [1.0, 2.0]):
        with pytest.raises(ValueError):
            api.band_tb(bad, rad)
        with pytest.raises(ValueError):
            api.band_tb_slope(bad, rad)


# ---- the wrappers, without a context ---------------------------------------------------------------------------------------------------
class NoLibrary:
    def __getattr__(self, name):
        def entry(*args):
            raise AssertionError(f"the wrapper reached the library ({name})")
        return entry


@pytest.fixture()
def dry():
    """A MonoRTM that has no context and fails the test at any library call, one operator registered, and a batch for it."""
    r = object.__new__(api.MonoRTM)
    r.lib, r.ctx, r.real_kind, r.dtype = NoLibrary(), None, 8, np.float64
    wn = np.linspace(1.0, 5.0, 52)
    op = oc.operator("A", "nested", 52)
    r._obs = {17: op}
    prs = [synth.perturbed_profile(3, wn, nlay=4)]
    return r, prs, np.ones((9, 4)), op


def test_quantity_names():
    assert api._quantity("band_tb", band=True) == 2 and api._quantity("TB", band=True) == 1 and api._quantity("rad", band=True) == 0
    assert api._quantity("tb") == 1 and api._quantity("rad") == 0 and api._quantity(2) == 2
    for q in ("band_tb", "bt"):
        with pytest.raises(ValueError):
            api._quantity(q)
        with pytest.raises(KeyError):      # what an unknown name has always raised
            api._quantity(q)
    with pytest.raises(ValueError):
        api._quantity("bt", band=True)


def test_band_tb_is_for_the_forward_entries_only(dry):
    r, prs, path, op = dry
    O = np.ones((1, 4, 52))
    for call in (lambda: r.rtm_jacobian(prs, O, quantity="band_tb"), lambda: r.jacobian(prs, quantity="band_tb"),
                 lambda: r.rtm_scan_jacobian(prs, O, path, quantity="band_tb"), lambda: r.scan_jacobian(prs, path, quantity="band_tb"),
                 lambda: r.rtm_obs_jacobian(prs, O, path, 17, quantity="band_tb"), lambda: r.obs_jacobian(prs, path, 17, quantity="band_tb")):
        with pytest.raises(ValueError):
            call()
    # the forward wrappers accept the name: with a good vcen they get as far as the library
    v = np.linspace(1.0, 2.0, op.nchan)
    for call in (lambda: r.rtm_obs(prs, O, path, 17, quantity="band_tb", vcen=v), lambda: r.obs(prs, path, 17, quantity="band_tb", vcen=v)):
        with pytest.raises(AssertionError, match="reached the library"):
            call()


@pytest.mark.parametrize("bad", ["missing", "short", "zero", "negative", "nan", "inf", "matrix"])
def test_vcen_is_validated_before_any_library_call(dry, bad):
    r, prs, path, op = dry
    v = np.linspace(1.0, 2.0, op.nchan)
    v = dict(missing=None, short=v[:-1], zero=np.where(np.arange(op.nchan) == 2, 0.0, v), negative=-v, nan=np.where(np.arange(op.nchan) == 6, np.nan, v),
             inf=np.where(np.arange(op.nchan) == 0, np.inf, v), matrix=v[None])[bad]
    with pytest.raises(ValueError, match="vcen"):
        r.rtm_obs(prs, np.ones((1, 4, 52)), path, 17, quantity="band_tb", vcen=v)
    with pytest.raises(ValueError, match="vcen"):
        r.obs(prs, path, 17, quantity=2, vcen=v)
    # ignored for the other quantities: the call gets as far as the library
    with pytest.raises(AssertionError, match="reached the library"):
        r.obs(prs, path, 17, quantity="tb", vcen=v)


def test_symbols_and_fields():
    lib = ctypes.CDLL(api._build.build_hip())
    assert all(hasattr(lib, n) and n in api.SYMBOLS for n in ("monortm_hip_rtm_obs", "monortm_hip_rtm_obs_dev", "monortm_hip_obs", "monortm_hip_obs_dev"))
    assert [len(api.SYMBOLS[n][1]) for n in ("monortm_hip_rtm_obs", "monortm_hip_rtm_obs_dev", "monortm_hip_obs", "monortm_hip_obs_dev")] == [20, 21, 31, 33]
    assert api.OBS_FIELDS == ("o", "y")


# ---- the premise of the end-to-end comparison ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("views,chmap", [("A", "nested"), ("B", "comb")])
def test_premise_contracted_scan_equals_contracted_runs(oracle_case, views, chmap):
    """What tests/test_obs_forward.py's comparison with Oracle.run on scaled amounts means: Y contracted from the oracle's RTM on
    s x O (what the forward operator computes) against Y contracted from whole oracle runs on amounts scaled by s.  The two differ
    by MODM's linearity in the amounts, which tests/test_scan_cpu.py holds to 1e-13 relative in every tau.  A relative change eps of
    every tau moves a layer's term of the radiance (transmittance above x emission) by at most (1.2 + x) eps of the term, x the
    optical depth between the layer and the observer, and the term carries exp(-x): summed over the column that stays below ~4 eps
    of the radiance (twice for the reflected path), and d ln TB / d ln RAD <= 1.  Asserted: 1e-12 S per element, TB and RAD."""
    wn, orc = oracle_case
    op = oc.operator(views, chmap, len(wn))
    fac = oc.factors(op.npath)
    worst = 0.0
    for i, irt in zip((500, 501), (1, 3)):
        pr = synth.perturbed_profile(i, wn, nlay=20, cloud=True, irt=irt)
        s = fac[:, None] * (1.0 + 0.01 * np.arange(20) / 19.0)[None, :]
        o = orc.run(pr).o
        for k in (1, 0):
            a = np.array([_orc_rtm(pr, s[j][:, None] * o)[k] for j in range(op.npath)])[None]
            runs = [orc.run(scaled(pr, s[j])) for j in range(op.npath)]
            b = np.array([(r.tb if k else r.rad) for r in runs])[None]
            ya, S = oc.reference(op, a)
            yb, _ = oc.reference(op, b)
            e = np.abs(ya - yb)
            worst = max(worst, float(np.max(e / np.where(S > 0, S, 1.0))))
            assert np.all(e <= 1e-12 * S)
    print(f"premise {views}/{chmap}: worst |dY| / S = {worst:.2e}")


MIXED_CASE = ("B30", "A", "nested")   # batch, views, channel map of the mixed-sign band-TB case of tests/test_obs_forward.py


def test_mixed_sign_case_of_the_gpu_test_is_decided():
    """tests/test_obs_forward.py excludes from its NaN-position check the elements whose contracted radiance is below 1e-12 S (their
    sign is not determined) and caps their share at 5 % of the non-empty elements.  Here, with the oracle's radiances on that test's
    batch, factors and operator (the seeds of test_obs_jacobian.shared_mono): the share that would be excluded, and that the case
    holds elements of both signs."""
    import rtm_truth
    import test_scan_jacobian as sj

    name, views, chmap = MIXED_CASE
    b = sj.Batch(sj.BATCHES[name], 11 + list(sj.BATCHES).index(name))
    op = oc.operator(views, chmap, sj.NWN)
    path = b.path(oc.factors(op.npath))
    O = b.pad(b.O, 0.0)
    rad = np.stack([rtm_truth.oracle(b.wn, b.nlay, b.irt, b.T, b.TZ, O * path[:, j, :, None], b.ts, b.em, b.rf)[0]["rad"]
                    for j in range(op.npath)], axis=1)
    y, S = oc.reference(op, rad)
    live = S > 0
    undecided = live & (np.abs(y) < 1e-12 * S)
    print(f"mixed-sign operator: {int(undecided.sum())} of {int(live.sum())} elements undecided, {int((y[live] <= 0).sum())} not positive")
    assert undecided.sum() <= 0.05 * live.sum() and np.any(y[live] <= 0) and np.any(y[live] > 0)


def test_obs_bench_builds_its_workload():
    """tools/obs_bench.py imports without a GPU and describes the workload of tools/obs_jacobian_bench.py."""
    spec = importlib.util.spec_from_file_location("obs_bench", os.path.join(ROOT, "tools", "obs_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.stats([1.0, 2.0, 3.0, 4.0, 10.0]) == dict(median=3.0, min=1.0, max=10.0, iqr=2.0, n=5)
    op = mod.operator(16, 50)
    assert (op.nview, op.nchan, op.npath, op.nwn) == (4, 10, 16, 50)
