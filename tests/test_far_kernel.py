"""far_kernel's variants - 1, 2, 4 and 8 waves per workgroup, double and single precision - on the cases of tests/far_cases.py.

The launcher chooses the variant of every level by itself from the density of the line list; which one served a launch is read from
monortm_hip_counter (selectors 16 .. 19) and must be exactly what the case declares: a case that silently takes another variant fails.
MONORTM_FAR_WAVES overrides the choice and would void every expectation: the module refuses to run with it.

Per case and precision, from ONE set of runs (cached: nothing runs twice):
  oracle     O_BY_MOL on the stretches of far_cases.stretches() - per (layer, molecule) row |got - ref| / max over the stretch of |ref| -
             within 1e-10 in double, the far-field bound of test_hip_parity.py::test_far_kernel_dense_grid; single precision through
             compare(..., SGL_VS_DBL, rad_floor=1e-30); compare() on top for the radiances of the stretch.  The oracle's own additivity in
             this measure is ~2e-14 (tests/test_far_cpu.py).
  in-kernel  the whole grid against the same context with far_levels = 0 and tile_waves = auto (lines_kernel forms the far field
             itself): 1e-11 in the same measure (single precision: SGL_VS_DBL), every wavenumber; rows of a molecule without a column are
             exactly zero.
  repeat     the same call twice is bit-identical (the waves' sums are added in wave order).
  slices     one case with nslice = 3.
Observed maxima per case: LABNOTES, "far_kernel's multi-wave variants".
"""
import dataclasses
import os
import types

import numpy as np
import pytest

import far_cases as fc
from common import RTOL, compare
from monortm_amd import api, tape3

pytestmark = pytest.mark.gpu

SGL_VS_DBL = 5e-5          # compare() of a real_kind = 4 context against double-precision values (tests/test_hip_parity.py)
_RESULTS = {}


@pytest.fixture(scope="module")
def dev(workdir):
    import torch

    if os.environ.get("MONORTM_FAR_WAVES"):
        pytest.fail("MONORTM_FAR_WAVES is set: it overrides the waves per workgroup these tests expect far_kernel to choose - unset it")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return types.SimpleNamespace(workdir=workdir)


def far_counts(rt) -> np.ndarray:
    return np.array([rt.counter(api.FAR_COUNTER0 + k) for k in range(len(api.FAR_WAVES))])


def multiset(counts) -> tuple:
    return tuple(sorted(n for n, k in zip(api.FAR_WAVES, counts) for _ in range(int(k))))


def cut(d, sl):
    """The Dump of a whole grid on one stretch."""
    return dataclasses.replace(d, **{k: getattr(d, k)[..., sl] for k in ("o", "o_by_mol", "oc", "o_clw", "rup", "rdn", "trtot", "rad", "tb", "tmr")})


def run_once(dev, name, kind):
    key = (name, kind)
    if key in _RESULTS:
        if isinstance(_RESULTS[key], BaseException):     # (a run that failed is not started again by the next test of the case)
            raise _RESULTS[key]
        return _RESULTS[key]
    try:
        _RESULTS[key] = _run(dev, name, kind)
    except BaseException as e:
        _RESULTS[key] = e
        raise
    return _RESULTS[key]


def _run(dev, name, kind):
    from oracle.pyoracle import Oracle

    case = fc.CASES[name]
    pl, wn, profs = fc.plan(case, kind), case.wn, fc.profiles(case)
    t3 = f"{dev.workdir}/TAPE3_far_{name}"
    tape3.write_tape3(t3, fc.records(case))
    rt = api.MonoRTM(t3, wn[0], wn[-1], real_kind=kind)
    assert rt.line_count(0) == pl.nlines, "the context holds other blocks of the file than the mirror expects"
    levels = "auto" if case.far_levels is None else case.far_levels
    res = types.SimpleNamespace(case=case, profs=profs, moved={})

    def call(label, tile_waves, far_levels, nslice=0):
        rt.set_option("tile_waves", tile_waves)
        rt.set_option("far_levels", far_levels)
        rt.set_option("nslice", nslice or "auto")
        before = far_counts(rt)
        out = rt.run(profs)
        res.moved[label] = multiset(far_counts(rt) - before)
        return out

    assert not far_counts(rt).any() and rt.counter(api.FAR_COUNTER0 + 4) == -1 and rt.counter(15) == -1
    res.got = call("first", case.tile_waves, levels)
    res.again = call("again", case.tile_waves, levels)
    res.inkernel = call("inkernel", "auto", 0)
    res.sliced = call("sliced", case.tile_waves, levels, case.nslice) if case.nslice else None
    rt.close()
    orc = Oracle(t3, wn[0], wn[-1])
    res.exp = {what: [orc.run(p) for p in fc.profiles(case, sl)] for what, sl in fc.stretches(case)}
    orc.close()
    return res


@pytest.mark.parametrize("name,kind", fc.RUNS)
def test_variants_taken_and_oracle(name, kind, dev):
    res = run_once(dev, name, kind)
    case = res.case
    for label in ("first", "again") + (("sliced",) if case.nslice else ()):
        assert res.moved[label] == case.expect, f"{name} real_kind={kind} ({label}): far_kernel launches by waves per workgroup {res.moved[label]}, the case declares {case.expect}"
    assert res.moved["inkernel"] == (), res.moved
    worst = {}
    for what, sl in fc.stretches(case):
        for ip, exp in enumerate(res.exp[what]):
            got = cut(res.got[ip], sl)
            e = fc.row_error(got.o_by_mol, exp.o_by_mol)
            worst[what] = max(worst.get(what, 0.0), float(e.max()))
            tag = f"{name} real_kind={kind} {what} profile {ip}"
            if kind == 8:
                assert e.max() <= fc.TOL_ORACLE, f"{tag}: E = {e.max():.2e} at (layer, molecule) {np.unravel_index(np.argmax(e), e.shape)}\n{e}"
                compare(got, exp, rtol=RTOL, what=tag)
            else:
                compare(got, exp, rtol=SGL_VS_DBL, what=tag, rad_floor=1e-30)
    print(f"E oracle {name} real_kind={kind} variants {res.moved['first']}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("name,kind", fc.RUNS)
def test_equals_in_kernel_far_field(name, kind, dev):
    res = run_once(dev, name, kind)
    worst = 0.0
    runs = [("far_kernel", res.got)] + ([(f"nslice={res.case.nslice}", res.sliced)] if res.sliced else [])
    for label, dumps in runs:
        for ip, (g, r) in enumerate(zip(dumps, res.inkernel)):
            e = fc.row_error(g.o_by_mol, r.o_by_mol)
            worst = max(worst, float(e.max()))
            assert e.max() <= (fc.TOL_INKERNEL if kind == 8 else SGL_VS_DBL), f"{name} real_kind={kind} {label} profile {ip}: E = {e.max():.2e}\n{e}"
            nocol = res.profs[ip].wkl == 0.0
            assert not g.o_by_mol[nocol].any() and np.isfinite(g.o_by_mol).all()
            if kind == 8:
                np.testing.assert_allclose(g.tb, r.tb, rtol=1e-10)
    assert not res.case.zero or any((p.wkl == 0.0).any() for p in res.profs)
    print(f"E in-kernel {name} real_kind={kind}: {worst:.2e}")


@pytest.mark.parametrize("name,kind", fc.RUNS)
def test_bit_reproducible(name, kind, dev):
    res = run_once(dev, name, kind)
    for ip, (a, b) in enumerate(zip(res.got, res.again)):
        for k in ("o", "o_by_mol", "rad", "tb"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), f"{name} real_kind={kind} profile {ip}: {k} differs between two calls"


def test_every_variant_served_a_launch(dev):
    """Last: over the module far_kernel ran with 1, 2, 4 and 8 waves per workgroup in double precision and with 2, 4 and 8 in single."""
    seen = {8: set(), 4: set()}
    for name, kind in fc.RUNS:
        seen[kind] |= set(run_once(dev, name, kind).moved["first"])
    assert seen[8] == {1, 2, 4, 8} and {2, 4, 8} <= seen[4], seen
    assert any(r.sliced is not None for r in _RESULTS.values() if not isinstance(r, BaseException))
