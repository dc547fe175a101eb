"""The launch-wide chunk plan of lines_ms_kernel (ms_plan_wave in monortm_amd/csrc/lines_ms_kernel.hip: the candidate windows of a state
with RHORAT <= 1, their prefix sums and per chunk the plain / MXBRD bits and the slot words, written once per launch by blocks of
ms_reach_kernel's grid) against every wave planning for itself, and against the oracle.  Option `ms_plan` = "on" (the default: a wave
whose states all match the plan copies its windows, and its plain chunks take their words from it) / "off" (the searches and ballots of
every wave) puts both paths through the same inputs in one build; `lines_kernel = ms` forces the kernel onto these small batches.

The shapes are the smallest at which the plan can go wrong (the builders of tests/test_ms_prepare_fused.py where the shape is theirs):
  match         7 profiles x 3 layers x 50 channels x the 500-line list: one full group of six and a group of one, one profile with
                fewer layers, one state without a column of one molecule (the wave still matches); 15 chunks of 32 + a tail of 20
  dense_mixed   the same with the bottom layer of two profiles at RHORAT 1.2 (asserted here): the waves of layer 0 fall back, the
                others match; dense_mixed2: RHORAT > 2, the dense word
  absent        a molecule's column zero in ALL six states of a group's bottom layer: that wave falls back (its union is empty where
                the plan's window is not), the others match
  ns2_g8, real  G = 8, CL = 16, two passes on 40 channels; the real-like list with CL = 21: molecules beyond MXBRD, coupled O2 whose
                window is the whole range, non-plain chunks between plain ones
  handback      c2lc cut down: Voigt candidates make the trip hand chunks back inside matching waves
  tail          the 333-line list: a last chunk of 13 lines
  nan, nan_column   a NaN temperature (both paths stop) / a NaN column (the wave falls back and carries the NaNs)
  shift_edge    a sorted list with lines within 1e-9 of both window bounds wn[0] - 25 - pad and wn[-1] + 25 + pad, on either side, in two
                molecules: the plan's windows must be the per-wave ones to the line (bottom layers at RHORAT 1.014 fall back, with
                their own pad)
(a) the two paths give identical bits in every output and stop alike; (b) the `on` run agrees with the oracle, profile by profile,
at the tolerance tests/test_ms_kernel.py uses.  One test needs no GPU: the match rule and the plan's windows restated in Python
(the reach rule of tests/ms_reach_cases.py for the chunk words) - per-wave windows equal the plan's exactly where the rule says so."""
import numpy as np
import pytest

import ms_reach_cases as mr
import test_ms_prepare_fused as fused
from common import FIELDS, RTOL, compare, compare_nan_aware
from monortm_amd import api, synth, tape3

ETEMP = 4   # MONORTM_ETEMP: the reference's STOP in TIPS_2003


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


def _dense_mixed(p0, t0):
    rec, kw, profs = fused._ragged()
    for i in (1, 4):
        profs[i].p[0], profs[i].t[0] = p0, t0
    return rec, kw, profs


def _absent():
    rec, kw, profs = fused._ragged()
    for i in range(6):
        profs[i].wkl[0, 2] = 0.0   # no O3 in the bottom layer of the whole first group
    return rec, kw, profs


EDGE_WN = np.linspace(100.0, 140.0, 50)


def _shift_edge():
    pshift = 0.05
    pad = 2.0 * float(np.float32(pshift)) + 1e-6   # max_abs_shift x 1 + 1e-6 (line_table.cpp: 2 |delt| for a list without broadening records)
    vlo, vhi = EDGE_WN[0] - 25.0 - pad, EDGE_WN[-1] + 25.0 + pad
    lines = []
    for mol in (mr.H2O, mr.CO2):
        at = [vlo - 1e-9, vlo, vlo + 1e-9] + list(np.linspace(90.0, 150.0, 37)) + [vhi - 1e-9, vhi, vhi + 1e-9, vhi + 1.0]
        lines += [mr.Line(mol, float(v), pshift) for v in at]
    ll = mr.LineList("shift_edge", 50, lines, "plain")
    assert ll.mas() == 2.0 * float(np.float32(pshift))
    return mr.records(ll), {}, [mr.profile(EDGE_WN, "ORD", fc=1.0 + 0.07 * i) for i in range(7)]


CASES = {"match": fused._ragged, "dense_mixed": lambda: _dense_mixed(1050.0, 250.0), "dense_mixed2": lambda: _dense_mixed(1100.0, 150.0),
         "absent": _absent, "ns2_g8": fused._ns2_g8, "real": fused._ns2_real, "handback": fused._special, "tail": fused._tail,
         "nan": lambda: fused._ragged(nan="t"), "nan_column": lambda: fused._ragged(nan="column"), "shift_edge": _shift_edge}
_RUNS = {}


def _runs(name, workdir):
    """The case's file and profiles and its two runs (computed once, shared by the two tests of the case)."""
    if name not in _RUNS:
        rec, kw, profs = CASES[name]()
        t3 = f"{workdir}/TAPE3_msplan_{name}"
        tape3.write_tape3(t3, rec, **kw)
        out = {}
        for mode in ("on", "off"):
            rt = api.MonoRTM(t3, profs[0].wn[0], profs[0].wn[-1])
            rt.set_option("lines_kernel", "ms")
            rt.set_option("ms_plan", mode)
            try:
                out[mode] = rt.run(profs)
            except api.MonoRTMError as e:   # (kept: the two paths must stop alike)
                out[mode] = e.code
            rt.close()
        _RUNS[name] = (t3, profs, out["on"], out["off"])
    return _RUNS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_plan_is_bitwise_every_wave_for_itself(name, workdir, gpu):
    _, profs, on, off = _runs(name, workdir)
    if name == "nan":
        assert on == ETEMP and off == ETEMP, f"NaN temperature: ms_plan on -> {on!r}, off -> {off!r}, not the temperature stop"
        return
    assert not isinstance(on, int) and not isinstance(off, int), f"{name}: error code {on!r} / {off!r}"
    for i in range(len(profs)):
        for f in FIELDS:
            x, y = np.asarray(getattr(on[i], f)), np.asarray(getattr(off[i], f))
            assert np.array_equal(x, y, equal_nan=True), f"{name} profile {i}: {f} differs between ms_plan = on and off " \
                                                         f"(max |difference| {np.nanmax(np.abs(x - y)):.3e})"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_plan_matches_oracle(name, workdir, gpu):
    from oracle.pyoracle import Oracle, OracleError

    t3, profs, on, _ = _runs(name, workdir)
    orc = Oracle(t3, profs[0].wn[0], profs[0].wn[-1])
    if name == "nan":
        with pytest.raises(OracleError, match="TIPS"):
            orc.run(profs[3])
        orc.close()
        assert on == ETEMP
        return
    assert not isinstance(on, int), f"{name}: error code {on!r}"
    for i, pr in enumerate(profs):
        exp = orc.run(pr)
        if np.isnan(pr.wkl).any():   # (the reference's NaN stays in the profile that holds it: positions must coincide)
            compare_nan_aware(on[i], exp, rtol=RTOL, what=f"ms_plan on vs oracle {name}[{i}]")
        else:
            compare(on[i], exp, rtol=RTOL, what=f"ms_plan on vs oracle {name}[{i}]")
    orc.close()


@pytest.mark.gpu
def test_ms_plan_option_values(workdir, gpu):
    """`ms_plan` knows auto / on / off and refuses anything else (a mistyped switch must not run silently)."""
    rec = synth.synthetic_lines(20, seed=3)
    t3 = f"{workdir}/TAPE3_msplan_opt"
    tape3.write_tape3(t3, rec)
    wn = synth.c2_channels(10)
    rt = api.MonoRTM(t3, wn[0], wn[-1])
    for v in ("auto", "on", "off"):
        rt.set_option("ms_plan", v)
    with pytest.raises(api.MonoRTMError):
        rt.set_option("ms_plan", "yes")
    rt.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the mirror (no GPU): ms_prologue's windows, ms_plan_wave's, the match rule
# ---------------------------------------------------------------------------------------------------------------------------------
def _table(rec, nmol):
    """Per molecule the line centres in file order (the table's order: a file's lines ascend), and max_abs_shift."""
    keep = np.asarray(rec.iflg) >= 0
    mol = np.asarray(rec.mol)[keep] % 100
    vnu = np.asarray(rec.vnu, float)[keep]
    return [vnu[mol == m + 1] for m in range(nmol)], mr.max_abs_shift(np.asarray(rec.pshift)[keep])


def _window(v, wn, mas, rhorat):
    """lines_ms_kernel.hip, ms_prologue: [lo, hi) of a sorted molecule for one state - or None where it is empty."""
    pad = mas * max(rhorat, 1.0) + 1e-6
    vlo, vhi = wn[0] - 25.0 - pad, wn[-1] + 25.0 + pad
    lo = int(np.searchsorted(v, vlo, side="left"))        # first centre >= vlo
    hi = max(lo, int(np.searchsorted(v, vhi, side="right")))   # first centre > vhi, searched from lo on
    return (lo, hi) if hi > lo else None


def _wave_windows(tab, mas, wn, states):
    """The union a wave forms: states = [(RHORAT, WTOT, T, columns)] of its live states."""
    out = []
    for m, v in enumerate(tab):
        ws = [_window(v, wn, mas, r) for r, _, _, wk in states if wk[m] != 0.0]
        ws = [w for w in ws if w]
        out.append((min(w[0] for w in ws), max(w[1] for w in ws)) if ws else None)
    return out


def _matches(plan, states):
    ok = all(r <= 1.0 and wtot == wtot and t == t for r, wtot, t, _ in states)
    return ok and all(w is None or any(wk[m] != 0.0 for *_, wk in states) for m, w in enumerate(plan))


def _waves(profs):
    g = mr.group_size(profs[0].nwn, len(profs))
    for p0 in range(0, len(profs), g):
        for lay in range(max(p.nlay for p in profs)):
            st = [(float(mr.rhorat_of(p)[lay]), float(p.wkl[lay].sum() + p.wbrodl[lay]), float(p.t[lay]), p.wkl[lay])
                  for p in profs[p0:p0 + g] if lay < p.nlay]
            if st:
                yield (p0, lay), st


@pytest.mark.parametrize("name", ["match", "absent", "dense_mixed", "shift_edge"])
def test_match_rule_and_plan_windows_cpu(name):
    rec, _, profs = CASES[name]()
    wn, nmol = np.asarray(profs[0].wn, float), profs[0].wkl.shape[1]
    tab, mas = _table(rec, nmol)
    plan = [_window(v, wn, mas, 1.0) for v in tab]
    assert any(plan), "no molecule has a candidate: the case tests nothing"
    seen = {True: 0, False: 0}
    for key, states in _waves(profs):
        rule = _matches(plan, states)
        same = _wave_windows(tab, mas, wn, states) == plan
        if name in ("match", "absent"):
            assert same == rule, f"{name} wave {key}: the rule says {'match' if rule else 'fall back'}, windows {'equal' if same else 'differ'}"
        else:   # (a denser state widens the pad by less than the gap to the next line in most lists: equal windows without a match are allowed)
            assert same or not rule, f"{name} wave {key}: the rule says match and the windows differ"
        seen[rule] += 1
    assert seen[True] > 0, f"{name}: no wave matches the plan"
    if name != "match":
        assert seen[False] > 0, f"{name}: no wave falls back"
    if name == "dense_mixed":
        assert all(float(mr.rhorat_of(profs[i])[0]) > 1.0 for i in (1, 4))
        _, _, p2 = CASES["dense_mixed2"]()
        assert all(float(mr.rhorat_of(p2[i])[0]) > mr.REACH_RHO for i in (1, 4))
    if name == "shift_edge":
        # the lines at vlo - 1e-9 and vhi + 1e-9 are outside, those at the bounds and 1e-9 inside are in: 3 + 37 + 2 + ... per molecule
        v = tab[0]
        lo, hi = plan[0]
        pad = mas + 1e-6
        assert v[lo] == wn[0] - 25.0 - pad and v[lo - 1] < v[lo] and v[hi - 1] == wn[-1] + 25.0 + pad and v[hi] > v[hi - 1]
        # ... and the chunk words of the plan are the reach words of exactly those lines (tests/ms_reach_cases.py's rule)
        cand = [x for m, w in enumerate(plan) if w for x in tab[m][w[0]:w[1]]]
        lps, cl = mr.lps_of(len(wn)), 32
        words = [mr.reach_word(wn, lps, float(x), mas, False) for x in cand]
        for c0 in range(0, len(cand), cl):
            rk = [sum(((w >> k) & 1) << j for j, w in enumerate(words[c0:c0 + cl])) for k in range(mr.WPS)]
            assert all(r < (1 << min(cl, len(cand) - c0)) for r in rk) and any(rk)
