"""The constructed line lists of tests/line_class_cases.py, without a GPU: the classes the cases claim against the mirror of the class
rule, a census of the class steps, pair positions, group offsets and cutter positions that the GPU module (tests/test_line_classes.py)
reaches - asserted complete - and the additivity of the reference, which is the noise floor of the GPU module's measure."""
import numpy as np
import pytest

import line_class_cases as lc
from monortm_amd import tape3

GENERIC, KO2, KCO2 = 0, 1, 2
CLASSES = [(t, m) for t in (False, True) for m in (False, True)]
POSITIONS = ("first", "second", "tail", "single")
_CENSUS = {}


def _census(cfg_name):
    """Everything `cfg_name` walks, over all its cases and channel counts: a list of (case, nwn, tile index, slice, steps)."""
    if cfg_name not in _CENSUS:
        cfg = lc.CONFIGS[cfg_name]
        _CENSUS[cfg_name] = [(c.name, nwn, ti, w["slice"], w["steps"]) for c in lc.cases_of(cfg) for nwn in cfg.nwn
                             for ti, w in enumerate(lc.mirror(c, cfg, nwn))]
    return _CENSUS[cfg_name]


def _runs(steps):
    """The steps split into walks: maximal stretches of one molecule without a cutter that start at a 'first' or 'single' ... i.e. as
    walk() formed them: a new walk begins after a tail / single, at a cutter, at a new molecule, or at bit 0 of a group."""
    out, cur = [], []
    for l, s in steps:
        if s["pos"] == "cutter" or (cur and (cur[-1][0]["mol"] != l["mol"] or l["bit"] == 0 or cur[-1][1]["pos"] in ("tail", "single")
                                              or cur[-1][0]["index"] + 1 != l["index"])):
            if cur:
                out.append(cur)
            cur = []
        if s["pos"] != "cutter":
            cur.append((l, s))
    if cur:
        out.append(cur)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the class table
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", list(lc.CONFIGS) + ["sgl4_sounder"])
def test_claimed_classes_equal_the_mirror(cfg_name):
    """The class a case claims for a line - from its zone's nominal position alone - is what the mirror finds from the shifted centre in
    every state, for every tile of every channel count the configuration runs; the mirror asserts the 0.25 cm-1 margin to every class
    boundary and window end, the 0.5 cm-1 between channels and centres and the 0.01 cm-1 bound on the shifts on its way."""
    cfg = lc.CONFIGS.get(cfg_name, lc.SGL4)
    n = 0
    for case in lc.cases_of(cfg):
        for nwn in cfg.nwn:
            wn = lc.channels(case, cfg, nwn)
            profs = lc.big_batch(wn, 3) if cfg is lc.SGL4 else lc.profiles(case, cfg, wn)
            tl = [(float(wn[0]), float(wn[-1]))] if cfg.family == "ms" else lc.tiles(wn, 64 * cfg.nw * cfg.wpl)
            for lo, hi in tl:
                for l in lc.classify(case, lo, hi, lc.states_of(profs), full_boundary=cfg.family == "sgl2"):
                    want = lc.claimed(l["zone"], l["mol"], lo, hi, l["y"])
                    assert (l["test"], l["m2"]) == want, f"{case.name} nwn={nwn} tile [{lo}, {hi}] {l}: claimed {want}"
                    n += 1
            lc.mirror(case, cfg, nwn, profs)
    assert n > 0


def test_zone_table_of_the_docstring():
    """The zones' classes against 0.5 - 40 cm-1 and against the sounder range, as the module docstring of line_class_cases states them."""
    want = {"TM": (True, True), "UM": (False, True), "U1": (False, False), "T1": (True, False)}
    for z, cls in want.items():
        assert lc.claimed(z, lc.O3, 0.5, 40.0) == cls and lc.claimed(z, lc.O2, 0.5, 40.0) == cls
        assert lc.claimed(z, lc.CO2, 0.5, 40.0) == (cls[0], False)
    for z, cls in {"F1": (False, True), "F2": (False, True), "UM": (False, True), "TS": (True, False)}.items():
        assert lc.claimed(z, lc.O3, 0.3, 6.5) == cls
    assert all(lc.ZONE[z] + 6.5 <= 25.0 - lc.MARGIN - 0.3 for z in ("F1", "F2")) and lc.ZONE["UM"] + 6.5 >= 25.0 + lc.MARGIN


def test_table_offsets_of_the_group_cases():
    """The padding puts the O3 run where the case says: the molecules in front hold that many candidate lines (the GPU module checks the
    same numbers against monortm_hip_line_count)."""
    cfg = lc.CONFIGS["wn"]
    for off in (0, 1, 62, 63):
        w = lc.mirror(lc.CASES[f"group_bit{off}"], cfg, 37)[0]
        first = next(l for l, _ in w["steps"] if l["mol"] == lc.O3)
        assert first["bit"] == off and first["index"] == 0
    for name, mol, b0, b1 in (("group_two", lc.O3, 50, 99), ("group_three", lc.O3, 3, 132), ("group_three_o2", lc.O2, 60, 129)):
        c = lc.CASES[name]
        before = sum(c.nlines(m) for m in c.mols if m < mol)
        assert (before, before + c.nlines(mol) - 1) == (b0, b1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------------
def _steps_reached(cfg_name):
    got = set()
    for _c, _n, _t, _s, steps in _census(cfg_name):
        for _l, s in steps:
            if s["pos"] != "cutter":
                got.add((s["kind"], s["test"], s["m2"], s["pos"]))
    return got


@pytest.mark.parametrize("cfg_name", ["wn", "dbl2", "sgl1", "sgl2"])
def test_census_every_step_at_every_position(cfg_name):
    """lines_kernel: every (molecule kind, TEST, M2) step evaluates a first line of a pair, a second one, an odd tail and a single line -
    where the loops pair lines (lc.walk): generic molecules and O2, not the float one-wavenumber loops.  CO2 and those loops take one
    line at a time: every step is reached, by runs of one line and of more."""
    got = _steps_reached(cfg_name)
    paired = () if cfg_name == "sgl1" else (GENERIC, KO2)
    want = {(k, t, m, p) for k in paired for t, m in CLASSES for p in POSITIONS}
    assert not want - got, f"{cfg_name}: never reached: {sorted(want - got)}"
    loose = {(k, t, m) for k in (GENERIC, KO2) for t, m in CLASSES} | {(KCO2, t, False) for t in (False, True)}
    for many in (False, True):
        reached = {g[:3] for g in got if (g[3] != "single") == many}
        assert not loose - reached, f"{cfg_name}: never reached by a run of {'several lines' if many else 'one line'}: {sorted(loose - reached)}"
    assert not {g for g in got if g[0] == KCO2 and g[2]}, "CO2 has no negative resonance"


def test_census_every_step_at_every_position_ms():
    """lines_ms_kernel: the generic classes ONE and TWO, tested or not; O2 and CO2 always in their tested forms."""
    got = _steps_reached("ms")
    want = ({(GENERIC, t, m, p) for t, m in CLASSES for p in POSITIONS} | {(KO2, True, m, p) for m in (False, True) for p in POSITIONS} |
            {(KCO2, True, False, p) for p in ("first", "single")})
    assert not want - got, f"never reached: {sorted(want - got)}"
    assert not {g for g in got if g[0] != GENERIC and not g[1]}


@pytest.mark.parametrize("cfg_name,kinds", [("wn", (GENERIC, KO2)), ("dbl2", (GENERIC, KO2)), ("ms", (GENERIC,)), ("sgl1", (GENERIC, KO2))])
def test_census_every_ordered_class_pair_at_both_alignments(cfg_name, kinds):
    """Every ordered pair (class of line i, class of line i + 1) of one molecule's neighbouring lines, with i even and with i odd in
    its walk.  One wavenumber per lane in double precision: a walk pairs the lines whatever their classes, so 'even' is a pair inside
    one step and 'odd' a pair across two steps.  The other tiles cut the walk where the class changes: the alignment is that of line i
    in the molecule's run."""
    got = set()
    for _c, _n, _t, _s, steps in _census(cfg_name):
        by_mol = {}
        for l, s in steps:
            by_mol.setdefault(l["mol"], []).append((l, s))
        for mol, ls in by_mol.items():
            start = 0
            for k in range(len(ls) - 1):
                (a, sa), (b, sb) = ls[k], ls[k + 1]
                if sa["pos"] == "cutter" or b["bit"] == 0:
                    start = k + 1
                if "cutter" in (sa["pos"], sb["pos"]) or b["bit"] == 0 or b["index"] != a["index"] + 1:
                    continue
                got.add((lc.KIND[mol], (a["etest"], a["em2"]), (b["etest"], b["em2"]), (k - start) % 2))
                if cfg_name == "wn":   # the mirror's walk says the same
                    assert ((k - start) % 2 == 0) == (sa["pos"] == "first" and sb["pos"] == "second"), (a, sa, sb)
    want = {(k, c0, c1, al) for k in kinds for c0 in CLASSES for c1 in CLASSES for al in (0, 1)}
    assert not want - got, f"{cfg_name}: never reached: {sorted(want - got)}"


def test_census_seventeen_line_sequence():
    """The 17-line list holds each of the 16 ordered class pairs once; behind one more line every pair sits at the other alignment.
    Raw classes: what lines_ms_kernel and the two-wavenumber tiles walk (the one-wavenumber tiles smooth these short runs away and
    take their class changes from the block lists)."""
    for nm, mol in (("gen", lc.O3), ("o2", lc.O2)):
        seen = {}
        for name in (f"pairs_{nm}", f"pairs_{nm}_shift"):
            z = lc.CASES[name].zones(mol)
            lines = lc.classify(lc.CASES[name], 0.5, 40.0, lc.states_of([lc.base_profile(lc.wide_channels(37))]))
            cls = [(l["test"], l["m2"]) for l in lines]
            assert cls == [lc.claimed(x, mol, 0.5, 40.0) for x in z]
            seen[name] = {(a, b, i % 2) for i, (a, b) in enumerate(zip(cls[:-1], cls[1:]))}
        a, b = seen[f"pairs_{nm}"], seen[f"pairs_{nm}_shift"]
        want = {(c0, c1) for c0 in CLASSES for c1 in CLASSES}
        assert {x[:2] for x in a} == want and len(a) == 16
        assert {(c0, c1, 1 - al) for c0, c1, al in a} <= b


def test_census_case_list():
    """The kinds of list and how many of each there are: an edit that drops a case shows here."""
    from collections import Counter

    assert Counter(t for c in lc.CASES.values() for t in c.tags) == {"run": 28, "blocks": 14, "island": 12, "group": 7, "cut": 6, "pairs": 5, "co2": 3,
                                                                     "full": 3, "span3": 2, "zero": 2, "lump": 2, "span2": 1, "slice": 1, "voigt": 1}
    assert len(lc.CASES) == 80


def test_census_lumped_pedestal_of_the_two_wavenumber_tile():
    """eval_fast2 lumps the pedestals of an untested one-resonance generic sub-run of 16 lines or more (one wave_sum of pa): sub-runs of
    exactly 15 and 16 lines and a longer one are walked, in the one-wave tile and in the tiles of two and four waves."""
    for cfg_name in ("dbl2", "dbl2_tw1", "dbl2_tw2", "dbl2_tw4"):
        lens = set()
        for _c, _n, _t, _s, steps in _census(cfg_name):
            for run in _runs(steps):
                if {(s["kind"], s["test"], s["m2"]) for _l, s in run} == {(GENERIC, False, False)}:
                    lens.add(len(run))
        assert {15, 16} <= lens and max(lens) > 16, (cfg_name, sorted(lens))


def test_census_mixed_pairs_take_the_more_general_step():
    """In the one-wavenumber walk a pair of two classes is evaluated by the step of the more general line: every (class of the first,
    class of the second) reaches the step that is the OR of both, for generic molecules and O2."""
    got = set()
    for _c, _n, _t, _s, steps in _census("wn"):
        for (a, sa), (b, sb) in zip(steps[:-1], steps[1:]):
            if sa["pos"] == "first" and sb["pos"] == "second":
                assert (sa["test"], sa["m2"]) == (a["etest"] or b["etest"], a["em2"] or b["em2"]) == (sb["test"], sb["m2"])
                got.add((sa["kind"], (a["etest"], a["em2"]), (b["etest"], b["em2"])))
    want = {(k, c0, c1) for k in (GENERIC, KO2) for c0 in CLASSES for c1 in CLASSES}
    assert not want - got, f"never reached: {sorted(want - got)}"


def test_census_group_offsets_and_spans():
    """A molecule's run starts at bit 0, 1, 62 and 63 of a 64-line group and runs over two and three groups - unsliced, and cut by the
    slice boundaries of nslice = 3 (which also move the groups: a slice counts its 64 from its own first line)."""
    first_bits, spans, cut_by_slice = set(), set(), 0
    for cname, _n, _t, _s, steps in _census("wn"):
        runs = {}
        for l, s in steps:
            runs.setdefault(l["mol"], []).append(l)
        for mol, ls in runs.items():
            if "group" in lc.CASES[cname].tags and mol == lc.CASES[cname].test_mol:
                first_bits.add(ls[0]["bit"])
                spans.add(1 + sum(1 for l in ls[1:] if l["bit"] == 0))
    assert {0, 1, 62, 63} <= first_bits and {2, 3} <= spans, (first_bits, spans)
    per_slice = {}
    for cname, _n, _t, s, steps in _census("slice3"):
        for l, _ in steps:
            if l["mol"] == lc.CASES[cname].test_mol:
                per_slice.setdefault(cname, set()).add(s)
    cut_by_slice = sum(1 for v in per_slice.values() if len(v) >= 2)
    assert len(per_slice["group_three"]) == 3 and cut_by_slice >= 3, per_slice


def test_census_cutter_positions():
    """The coupled O2 line sits at positions 0, 1, 2, middle, last - 1 and last of its run of nine: the walks around it are 0, 1, 2 and
    more lines long, in lines_kernel and in lines_ms_kernel."""
    for cfg_name in ("wn", "ms", "dbl2"):
        pos, lens = set(), set()
        for cname, nwn, _t, _s, steps in _census(cfg_name):
            if "cut" not in lc.CASES[cname].tags:
                continue
            o2 = [(l, s) for l, s in steps if l["mol"] == lc.O2]
            k = [i for i, (_l, s) in enumerate(o2) if s["pos"] == "cutter"]
            assert len(k) == 1 and len(o2) == 9
            pos.add(k[0])
            if cfg_name == "wn":
                lens |= {k[0], 8 - k[0]}
        assert pos == set(lc.CUT_AT.values()), (cfg_name, pos)
        if cfg_name == "wn":
            assert {0, 1, 2} <= lens and max(lens) >= 3


def test_census_full_class():
    """Single precision, two and four wavenumbers per lane: FULL steps at every position for generic molecules and O2, two-resonance
    steps that are not FULL beside them, and a FULL line that the smoothing returned to the two-resonance loop."""
    for cfg, profs in ((lc.CONFIGS["sgl2_sounder"], None), (lc.SGL4, 3)):
        got, lost, notfull = set(), 0, 0
        for case in lc.cases_of(cfg):
            for nwn in cfg.nwn:
                p = lc.big_batch(lc.sounder_channels(nwn), profs) if profs else None
                for w in lc.mirror(case, cfg, nwn, p):
                    for l, s in w["steps"]:
                        if s["full"]:
                            assert not s["test"] and s["m2"] and l["full"]
                            got.add((s["kind"], s["pos"]))
                        lost += l["full"] and not l["efull"]
                        notfull += s["m2"] and not s["test"] and not l["full"]
        assert {(k, p) for k in (GENERIC, KO2) for p in ("first", "second", "tail")} <= got, got
        assert lost > 0 and notfull > 0
    assert not any(s["full"] for cfg in ("wn", "dbl2", "sgl1", "ms") for *_x, steps in _census(cfg) for _l, s in steps)


def test_census_run_lengths_and_zero_rows():
    """Walks of 1, 2, 3, 4, 5, 8 and 9 lines of every class in the one-wavenumber tile, and both kinds of zero rows: lines the window
    drops and lines that are walked but out of reach of every channel."""
    got = set()
    for _c, _n, _t, _s, steps in _census("wn"):
        for run in _runs(steps):
            cls = {(s["kind"], l["etest"], l["em2"]) for l, s in run}
            if len(cls) == 1:
                got.add(cls.pop() + (len(run),))
    want = {(k, t, m, n) for k in (GENERIC, KO2) for t, m in CLASSES for n in lc.RUN_LENGTHS} | {(KCO2, t, False, n) for t in (False, True) for n in lc.RUN_LENGTHS}
    assert not want - got, f"never reached: {sorted(want - got)}"
    cfg = lc.CONFIGS["wn"]
    assert not lc.mirror(lc.CASES["out_of_reach"], cfg, 37)[0]["steps"]
    walked = lc.mirror(lc.CASES["out_of_reach_walked"], cfg, 37)[0]["steps"]
    assert len(walked) == 9 and all(s["test"] for _l, s in walked)


def test_every_case_runs_somewhere_and_files_stay_one_block():
    used = {c.name for cfg in list(lc.CONFIGS.values()) + [lc.SGL4] for c in lc.cases_of(cfg)}
    assert used == set(lc.CASES)
    for c in lc.CASES.values():
        rec = lc.records(c)
        assert len(rec) <= tape3.NLINEREC and rec.n_physical == len(c.lines)
        s = rec.sp[rec.iflg >= 0].astype(float) * rec.vnu[rec.iflg >= 0] * (1.0 - np.exp(-1.4387752 * rec.vnu[rec.iflg >= 0] / 296.0))
        for mol in c.mols:
            sm = s[(rec.mol[rec.iflg >= 0] % 100) == mol]
            if not len(sm):
                continue
            assert sm.min() > 0 and sm.max() / sm.min() <= 100.0, "strengths of a molecule within two decades"
        ph = rec.iflg >= 0
        assert np.all((rec.alfa[ph] >= 0.03) & (rec.alfa[ph] <= 0.1) & (rec.hwhm[ph] >= 0.03) & (rec.hwhm[ph] <= 0.1) & (rec.pshift[ph] != 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# additivity of the reference
# ---------------------------------------------------------------------------------------------------------------------------------
ADDITIVITY_TOL = 1e-13
ADDITIVE_CASES = [n for n, c in lc.CASES.items() if not c.sounder and len(c.lines) <= 40 and not c.voigt] + ["group_three", "full_mixed"]


def test_reference_rows_are_sums_of_single_line_rows(workdir):
    """For each list the oracle's row of a molecule equals the sum of its rows over the single-line lists, to 1e-13 of the row's peak,
    in the three dense layers: no cancellation hides in the lists, and the GPU module's 1e-11 sits two decades above what the reference's
    own summation order can move.  (Lists of up to 40 lines, the 130-line list and a FULL list; the worst E is printed.)"""
    from oracle.pyoracle import Oracle

    worst = (0.0, "")
    for name in ADDITIVE_CASES:
        case = lc.CASES[name]
        wn = lc.sounder_channels(40) if case.sounder else lc.wide_channels(37)
        pr = lc.base_profile(wn, nlay=3)
        t3 = f"{workdir}/TAPE3_lcadd_{name}"
        tape3.write_tape3(t3, lc.records(case))
        orc = Oracle(t3, wn[0], wn[-1])
        whole = orc.run(pr).o_by_mol
        orc.close()
        parts = np.zeros_like(whole)
        for k, rec in enumerate(lc.single_line_cases(case)):
            tape3.write_tape3(t3 + "_1", rec)
            orc = Oracle(t3 + "_1", wn[0], wn[-1])
            parts += orc.run(pr).o_by_mol
            orc.close()
        e = lc.row_errors(whole, parts)
        assert np.isfinite(e).all(), f"{name}: a row of zeros is not the sum of zeros"
        if e.max() > worst[0]:
            worst = (float(e.max()), name)
        assert e.max() <= ADDITIVITY_TOL, f"{name}: E = {e.max():.2e}"
    print(f"additivity of the reference: worst E = {worst[0]:.2e} ({worst[1]})")
