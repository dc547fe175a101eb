"""Every launch variant of the continuum / cloud / total kernel (continuum_kernel.hip: finish_mw_kernel, finish_kernel<HIGH>, <PAR>, <Q4>,
plain with 64 / 256 threads) against the CPU oracle, slot by slot, on the cases of tests/continuum_cases.py.

The line file holds no lines, so O, OC and O_CLW are the finish kernel's work alone.  Which variant served a call is read from
monortm_hip_counter (selectors 2 .. 7): a case aimed at one variant that silently takes another fails.  tests/test_continuum_cpu.py
holds the oracle's continuum to the reference's, which is what makes it the reference here.

Tolerances (E of continuum_cases.py: per (layer, slot) row, relative with a floor of 1e-4 of the row's peak; zero rows exactly zero):
  double   1e-10 for OC, and for O in the one-factor calls.  Coarse values differ from the oracle's by <= ~20 ulp (pow as exp(y log x)
           with |y ln x| <= 4, rcp2 1 ulp, exp_cw 2 ulp), pass two 4-point interpolations with sum |w| <= 1.25 each and the 1e-4 floor:
           20 x 2.2e-16 x 1.56 x 1e4 = 7e-11.  It is the tolerance the far-field tests hold kernels to against the oracle.
  single   2^-23: the inputs are rounded to float32 first and the oracle is given those values, so only the stores round.
  O_CLW    1e-12, the tolerance tests/test_function_kat.py gives ODCLW_TKC (single: 2^-23, the store).
compare() of tests/common.py stays on top, for the radiances.
Observed E per case: LABNOTES, "Finish kernels slot by slot".
"""
import types

import numpy as np
import pytest

import continuum_cases as cc
from common import RTOL, compare
from monortm_amd import api

pytestmark = pytest.mark.gpu

SGL_VS_DBL = 5e-5          # compare() of a real_kind = 4 context against double-precision values (tests/test_hip_parity.py)
ONE_FACTOR_PROFILES = 5    # profiles of a one-factor call held to the oracle: the first five and the last (the GPU runs the whole batch)
_RESULTS = {}


@pytest.fixture(scope="module")
def dev(workdir):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return types.SimpleNamespace(cus=int(torch.cuda.get_device_properties(0).multi_processor_count),
                                 t3=cc.header_only_tape3(f"{workdir}/TAPE3_finish_kernels"))


def finish_counts(rt) -> np.ndarray:
    return np.array([rt.counter(api.FINISH_COUNTER0 + k) for k in range(len(cc.VARIANTS))])


def expect_counts(run, ncalls: int) -> np.ndarray:
    want = np.zeros(len(cc.VARIANTS), np.int64)
    want[cc.VARIANTS.index(run.expect)] = ncalls
    return want


def cut(O, OC, OCLW, i, nlay):
    return types.SimpleNamespace(o=O[i, :nlay], oc=OC[i, :nlay], o_clw=OCLW[i, :nlay])


def run_once(dev, case, run, kind=8, nprof=None, first=0):
    """One run of a case on the GPU and through the oracle, computed once per session: got / exp [call label][profile index]."""
    key = (case.name, run.label, kind, nprof, first)
    if key in _RESULTS:
        return _RESULTS[key]
    from oracle.pyoracle import Oracle

    n = case.nprofiles(dev.cus) if nprof is None else nprof
    profs = cc.profiles(case, run, n, first)
    if kind == 4:
        profs = [cc.to_f32(p) for p in profs]
    rt = api.MonoRTM(dev.t3, run.wn[0], run.wn[-1], real_kind=kind)
    assert rt.line_count(0) == 0
    if run.generic:
        rt.set_option("finish", "generic")
    orc = Oracle(dev.t3, run.wn[0], run.wn[-1])
    res = types.SimpleNamespace(profs=profs, got={}, exp={}, moved=None, want=None)
    before, ncalls = finish_counts(rt), 0
    for label, ps in cc.calls(profs):
        if label == "main":
            idx = range(n)
            res.got[label] = dict(enumerate(rt.run(ps)))
        else:
            idx = sorted(set(range(min(n, ONE_FACTOR_PROFILES))) | {n - 1})
            O, OBM, OC, OCLW = rt.modm(ps)
            assert not OBM.any()
            res.got[label] = {i: cut(O, OC, OCLW, i, ps[i].nlay) for i in idx}
        res.exp[label] = {i: orc.run(ps[i]) for i in idx}
        ncalls += 1
    res.moved, res.want = finish_counts(rt) - before, expect_counts(run, ncalls)
    rt.close()
    orc.close()
    _RESULTS[key] = res
    return res


def errors(res) -> dict:
    """The worst E of a run by field: OC and O_CLW over every call, O over the one-factor calls (there it is ONE term)."""
    e = {"oc": 0.0, "o_clw": 0.0, "o_one_factor": 0.0}
    e.update({f"o_only{k}": 0.0 for k in range(cc.NFAC)})
    for label, got in res.got.items():
        for i, g in got.items():
            x = res.exp[label][i]
            e["oc"] = max(e["oc"], cc.E(g.oc, x.oc))
            e["o_clw"] = max(e["o_clw"], cc.E(g.o_clw, x.o_clw))
            if label != "main":
                e["o_" + label] = max(e["o_" + label], cc.E(g.o, x.o))
                e["o_one_factor"] = max(e["o_one_factor"], e["o_" + label])
    return e


def check_run(dev, case, run, kind=8):
    res = run_once(dev, case, run, kind)
    what = f"{case.name} {run.label} real_kind={kind}"
    assert np.array_equal(res.moved, res.want), f"{what}: finish launches by variant {dict(zip(cc.VARIANTS, res.moved))}, wanted {run.expect} alone"
    e = errors(res)
    print(f"E {what}: " + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    tol = cc.TOL_DBL if kind == 8 else cc.TOL_SGL
    assert e["oc"] <= tol and e["o_one_factor"] <= tol, f"{what}: {e}"
    assert e["o_clw"] <= (cc.TOL_CLW if kind == 8 else cc.TOL_SGL), f"{what}: {e}"
    for i, g in res.got["main"].items():
        if kind == 8:
            compare(g, res.exp["main"][i], rtol=RTOL, what=f"{what} [{i}]")
        else:
            compare(g, res.exp["main"][i], rtol=SGL_VS_DBL, what=f"{what} [{i}]", rad_floor=1e-30)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_finish_variant_against_oracle(name, dev):
    case = cc.CASES[name]
    for run in case.runs:
        check_run(dev, case, run)


@pytest.mark.parametrize("name,label", cc.SGL_CASES)
def test_finish_variant_single_precision(name, label, dev):
    case = cc.CASES[name]
    check_run(dev, case, next(r for r in case.runs if r.label == label), kind=4)


def pair_error(a, b, fields=("oc", "o_clw", "o"), one_factor_o=range(cc.NFAC), chan=slice(None)) -> tuple:
    """(worst E between two results of the same states over the profiles both hold, whether every array is bit-identical)."""
    worst, same = 0.0, True
    for label in a.got:
        for i in set(a.got[label]) & set(b.got[label]):
            ga, gb = a.got[label][i], b.got[label][i]
            for f in fields:
                if f == "o" and label not in [f"only{k}" for k in one_factor_o]:
                    continue
                x, y = getattr(ga, f)[..., chan], getattr(gb, f)[..., chan]
                worst, same = max(worst, cc.E(x, y), cc.E(y, x)), same and np.array_equal(x, y)
    return worst, same


def test_variants_agree_with_each_other(dev):
    """The same states through two variants: the first three profiles of the big batches alone (<PAR>) against their rows in the batch
    (<Q4>, plain), finish = generic (<PAR>) against finish_mw_kernel, and the two runs of edge820 (finish_mw_kernel, <PAR>) on the
    channels they share.  Held at 1e-10; the observed maxima are in LABNOTES."""
    out = {}
    for name in ("q4_ragged", "plain64", "plain256_wide"):
        case = cc.CASES[name]
        run = case.runs[0]
        alone = run_once(dev, case, run, nprof=3)
        assert np.array_equal(alone.moved, expect_counts(types.SimpleNamespace(expect="par"), 8)), alone.moved
        out[f"{name}: par / {run.expect}"] = pair_error(alone, run_once(dev, case, run))
    gen, mw = cc.CASES["mw_generic"], cc.CASES["mw_chunks"]
    for rg in gen.runs:
        rm = next(r for r in mw.runs if r.label == rg.label)
        assert np.array_equal(rg.wn, rm.wn)
        out[f"mw_chunks {rg.label}: par / mw"] = pair_error(run_once(dev, gen, rg), run_once(dev, mw, rm))
    e = cc.CASES["edge820"]
    # (all but the last channel; O of the Rayleigh-only call is 0 below 820 and the Rayleigh term at 820: not compared)
    out["edge820: mw / par"] = pair_error(run_once(dev, e, e.runs[0]), run_once(dev, e, e.runs[1]), one_factor_o=range(6), chan=slice(0, -1))
    for k, (worst, same) in out.items():
        print(f"variants {k}: E = {worst:.2e}, bit-identical = {same}")
    bad = {k: v for k, v in out.items() if not v[0] <= cc.TOL_DBL}
    assert not bad, bad


def _device_batch(dev, case, run, kind=8):
    import torch

    profs = cc.profiles(case, run, case.nprofiles(dev.cus))
    rt = api.MonoRTM(dev.t3, run.wn[0], run.wn[-1], real_kind=kind)
    db = api.DeviceBatch(rt, profs)
    return torch, profs, rt, db


@pytest.mark.parametrize("name,label", [("q4_ragged", ""), ("mw_chunks", "65"), ("mw_chunks", "257")])
def test_padded_layers_are_zero(name, label, dev):
    """Layers >= nlay[p] of a ragged batch are exactly zero in O, OC, O_CLW and O_BY_MOL, whatever the output arrays held (NaN) - the
    zero fill of a 16-lane team (<Q4>) and of every wavenumber chunk (finish_mw_kernel).  The layers below are the host path's."""
    case = cc.CASES[name]
    run = next(r for r in case.runs if r.label == label)
    torch, profs, rt, db = _device_batch(dev, case, run)
    for t in (db.O, db.OC, db.OCLW, db.OBM):
        t.fill_(float("nan"))
    before = finish_counts(rt)
    db.step()
    torch.cuda.synchronize()
    db.check()
    assert np.array_equal(finish_counts(rt) - before, expect_counts(run, 1))
    O, OC, OCLW, OBM = (t.cpu().numpy() for t in (db.O, db.OC, db.OCLW, db.OBM))
    assert len({p.nlay for p in profs}) > 1
    host = run_once(dev, case, run).got["main"]
    for i, p in enumerate(profs):
        for a in (O, OC, OCLW, OBM):
            assert not a[i, p.nlay:].any() and np.isfinite(a[i]).all(), (i, p.nlay)
        assert np.array_equal(O[i, : p.nlay], host[i].o) and np.array_equal(OC[i, : p.nlay], host[i].oc)
        assert np.array_equal(OCLW[i, : p.nlay], host[i].o_clw)
    rt.close()


def test_graph_replay_q4_equals_stream_launches(dev):
    """q4_ragged recorded into a HIP graph: the replay equals the stream launches array for array."""
    case = cc.CASES["q4_ragged"]
    run = case.runs[0]
    torch, profs, rt, db = _device_batch(dev, case, run)
    db.step()
    torch.cuda.synchronize()
    ref = db.dumps(profs)
    db.capture()
    for t in (db.O, db.OBM, db.OC, db.OCLW, db.RAD, db.TB, db.TMR):
        t.fill_(float("nan"))
    before = finish_counts(rt)
    db.replay()
    torch.cuda.synchronize()
    db.check()
    assert not (finish_counts(rt) - before).any()       # a replay launches from the graph: the host side is not entered
    for i, d in enumerate(db.dumps(profs)):
        for k in ("o", "o_by_mol", "oc", "o_clw", "rup", "rdn", "trtot", "rad", "tb", "tmr"):
            assert np.array_equal(getattr(d, k), getattr(ref[i], k)), (i, k)
    assert not torch.isnan(db.O).any() and not torch.isnan(db.OC).any()
    rt.close()


def test_finish_option_and_counters(dev):
    """set_option("finish", ...) parses strictly and switches per call; unknown counters are -1."""
    case = cc.CASES["mw_chunks"]
    run = case.runs[0]
    profs = cc.profiles(case, run, 2)
    rt = api.MonoRTM(dev.t3, run.wn[0], run.wn[-1])
    assert rt.counter(8) == -1 and not finish_counts(rt).any()
    seq = []
    for value in ("generic", "auto", "generic", ""):
        rt.set_option("finish", value)
        before = finish_counts(rt)
        rt.modm(profs)
        seq.append(cc.VARIANTS[int(np.argmax(finish_counts(rt) - before))])
        assert (finish_counts(rt) - before).sum() == 1
    assert seq == ["par", "mw", "par", "mw"]
    for bad in ("mw", "1", "Generic"):
        with pytest.raises(api.MonoRTMError) as e:
            rt.set_option("finish", bad)
        assert e.value.code == 6
    rt.close()


def test_every_variant_was_reached(dev):
    """Last: over the cases of this file every one of the six variants served calls (the runs are cached: nothing runs twice)."""
    total = np.zeros(len(cc.VARIANTS), np.int64)
    for case in cc.CASES.values():
        for run in case.runs:
            total += run_once(dev, case, run).moved
    assert (total > 0).all(), dict(zip(cc.VARIANTS, total))
