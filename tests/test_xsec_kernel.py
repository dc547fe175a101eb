"""The cross-section kernel (xsec_kernel.hip) against the oracle's MONORTM_XSEC_SUB, cell by cell, on the cases of tests/xsec_cases.py.

The kernel takes 64 trips of the reference's outward walk at once and has to stop at the trip the sequential walk stops at: the tail that
is cut is about 1e-3 of a cell.  One trip early or late moves a cell by thr = 1e-6 x step / hwb >= 1.4e-7 here - under the 1e-6 / 2e-4 of
the parity tests, far over the bound of this file.  tests/test_xsec_cpu.py shows on the oracle's trace that no cell of the cases sits
near a threshold, an index or a switch where the two builds' roundings could part ways, and that the stops fall on every lane, in
the first block of 64 trips and after hundreds of blocks, by the criterion and by leaving both ends of the spectrum.

The line file holds no lines, the tables go in through set_xsec (the same bits the oracle gets), and a call has 127 x 10 x 3 waves at most.

Bounds:
  double   every ODXSEC cell within 1e-9 (relative) of the oracle; a cell the oracle has as zero exactly zero.
  single   P, T and XAMNT arrive as float32 and the oracle is given those values; the arithmetic is double, only the store rounds:
           |got - float32(e)| <= 2^-23 |e|.
  batch    the ragged batch (10, 4, 7 layers) equals the single-profile calls bit for bit; rows at lay >= nlay[prof] are exactly zero.
  sum      O with IXSECT = 1 minus O with IXSECT = 0 equals ODXSEC within 1e-12 of O (the finish kernel's addition, modm.f90:268).
  twice    a second call gives the same bits.

Observed on an MI355X (double: worst relative error of a call over its three profiles, and the walk of that cell in the oracle's trace):
  CCL4 alone  3.3e-13  t3, 1068 trips      F11 alone   2.6e-12  d2, 2700 trips      F12 alone   8.3e-12  ov2, 3289 trips
  HNO3 alone  4.8e-12  wide, 3489 trips    N2O5 alone  5.4e-12  neg, 1935 trips     all five    8.3e-12  (the F12 cell)
The worst cells are low-pressure layers (18.5 - 110 mb): step = 0.25 hwb, thousands of trips whose rounding the scan orders differently.
Single: every cell of every call equals float32 of the oracle's value bit for bit.  O(IXSECT = 1) - O(IXSECT = 0) - ODXSEC: 2.2e-16 of O at
the most, with ODXSEC up to 56 times the rest of O.  The whole file: 7 tests in 2.6 s.
Seeded errors, once each on a scratch build (never committed): `before = answer + incl` (the scan's shift dropped) and the stop lane taken
as first + 1 both fail the double and the single test in every call, by 2.5e-07 = thr in the calls of CCL4, F11, F12 and HNO3.
"""
import types

import numpy as np
import pytest

import continuum_cases as cc
import xsec_cases as xc
from monortm_amd import api

pytestmark = pytest.mark.gpu

_GOT = {}


@pytest.fixture(scope="module")
def dev(workdir):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return types.SimpleNamespace(t3=cc.header_only_tape3(f"{workdir}/TAPE3_xsec_kernel"))


def gpu(dev, kind: int):
    """Every call of xsec_cases.calls() through a context of `kind`, once per session: .single[label][i] = ODXSEC [nlay, nwn] of profile i
    called alone, .batch[label] = ODXSEC [3, 10, nwn] of the ragged batch; for the call `all` also O with and without IXSECT = 1 and a
    second run of the batch."""
    if kind in _GOT:
        return _GOT[kind]
    orc = xc.oracle(kind)
    rt = api.MonoRTM(dev.t3, xc.WN[0], xc.WN[-1], real_kind=kind)
    assert rt.line_count(0) == 0
    rt.set_xsec(orc.tabs)
    res = types.SimpleNamespace(single={}, batch={}, o1=None, o0=None, again=None)
    for label, profs in orc.profs.items():
        assert all(p.xs_names and not p.xs_dir for p in profs)
        res.single[label] = [rt.modm([p], ixsect=1)[4][0] for p in profs]
        out = rt.modm(profs, ixsect=1)
        res.batch[label] = out[4]
        if label == "all":
            res.o1 = out[0]
            res.o0 = rt.modm(profs, ixsect=0)[0]
            res.again = rt.modm(profs, ixsect=1)[4]
    rt.close()
    _GOT[kind] = res
    return res


def where(orc, label: str, i: int, lay: int, w: int) -> str:
    """What the oracle's trace says about a cell: per region in range, branch, trips, lane and block of the stop."""
    tr = orc.trace[i]
    out = [f"{label} profile {i} layer {lay} (P = {orc.profs[label][i].p[lay]:g} mb, T = {orc.profs[label][i].t[lay]:g} K) wn = {xc.WN[w]!r}"]
    for r, name in enumerate(xc.REGION_NAMES):
        b = tr.branch[r, lay, w]
        if b == 2:
            j = int(tr.trips[r, lay, w])
            out.append(f"{name}: walk, {j} trips, lane {(j - 1) % 64}, block {(j - 1) // 64}, "
                       f"{'criterion' if tr.stopkind[r, lay, w] == 1 else 'both ends'}, thr {tr.thr[r, lay, w]:.3g}")
        elif b == 3:
            out.append(f"{name}: linear")
    return "; ".join(out)


def worst_by_call(dev, kind: int, err) -> dict:
    """label -> (worst err(got, exp) over the profiles, description of the cell)"""
    orc, got = xc.oracle(kind), gpu(dev, kind)
    out = {}
    for label in orc.odx:
        worst = (-1.0, "")
        for i, exp in enumerate(orc.odx[label]):
            g = got.single[label][i]
            assert g.shape == exp.shape and g.dtype == (np.float32 if kind == 4 else np.float64)
            assert np.isfinite(g).all(), label
            assert not g[exp == 0].any(), f"{label} profile {i}: a cell the oracle has as zero is not zero"
            e = err(g.astype(np.float64), exp)
            lay, w = np.unravel_index(int(np.argmax(e)), e.shape)
            if e[lay, w] > worst[0]:
                worst = (float(e[lay, w]), where(orc, label, i, lay, w))
        out[label] = worst
    return out


def test_double_precision_every_cell_against_the_oracle(dev):
    def err(g, exp):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(exp != 0, np.abs(g - exp) / np.abs(exp), 0.0)

    worst = worst_by_call(dev, 8, err)
    for label, (e, cell) in worst.items():
        print(f"xsec kernel, real_kind = 8, {label}: max relative error {e:.3e} at {cell}")
    bad = {k: v for k, v in worst.items() if not v[0] <= xc.TOL_DBL}
    assert not bad, bad


def test_single_precision_is_one_rounding_from_the_oracle(dev):
    def err(g, exp):   # in units of the bound, 2^-23 |e|
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(exp != 0, np.abs(g - exp.astype(np.float32).astype(np.float64)) / (xc.TOL_SGL * np.abs(exp)), 0.0)

    worst = worst_by_call(dev, 4, err)
    for label, (e, cell) in worst.items():
        print(f"xsec kernel, real_kind = 4, {label}: max |got - float32(e)| / (2^-23 |e|) = {e:.4f} at {cell}")
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("kind", [8, 4])
def test_ragged_batch_equals_single_profiles_bit_for_bit(kind, dev):
    got = gpu(dev, kind)
    assert len(set(xc.NLAYS)) > 1
    for label, batch in got.batch.items():
        assert batch.shape == (len(xc.NLAYS), max(xc.NLAYS), len(xc.WN))
        for i, nl in enumerate(xc.NLAYS):
            assert np.array_equal(batch[i, :nl], got.single[label][i]), (label, i)
            assert not batch[i, nl:].any() and np.isfinite(batch[i]).all(), (label, i)


def test_cross_sections_are_summed_into_O(dev):
    got = gpu(dev, 8)
    odx = got.batch["all"]
    assert odx.any() and got.o0.shape == got.o1.shape == odx.shape
    live = np.zeros(odx.shape, bool)
    for i, nl in enumerate(xc.NLAYS):
        live[i, :nl] = True
    assert (got.o1[live] != 0).all()
    dev_ = np.abs((got.o1 - got.o0) - odx)[live] / np.abs(got.o1[live])
    print(f"xsec kernel: O(IXSECT = 1) - O(IXSECT = 0) - ODXSEC, max {dev_.max():.3e} of O; ODXSEC / O up to {np.max(odx[live] / got.o1[live]):.3g}")
    assert dev_.max() <= xc.TOL_SUM


@pytest.mark.parametrize("kind", [8, 4])
def test_second_call_gives_the_same_bits(kind, dev):
    got = gpu(dev, kind)
    assert np.array_equal(got.again, got.batch["all"])
