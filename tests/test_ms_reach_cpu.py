"""The slot masks of lines_ms_kernel without a GPU: the rule (monortm_amd/csrc/ms_reach.hpp), its Python mirror and the cases of
tests/ms_reach_cases.py.

  * the mirror equals the header: tests/native/ms_reach_check.cpp, built with the host compiler, prints the word of every case's
    lines and of 100000 seeded random inputs (NaN centres, `every` lines, fewer than five channels, empty slots);
  * the margin is sound: for random channels, lines and states with RHORAT <= 2 the slots a line truly reaches are a subset of its
    word, under the plain and the species-broadening shift rules; the species-shift lists are tight against that margin;
  * census: every slot that holds a channel has, on both sides and for the negative-resonance bits, a line that only the dense word
    lets through, a line that the margin keeps, and twins outside in every state - or a written reason; the pattern lists put a
    lone reaching line at every group position of every step that tests a mask (the MS_IFK / MS_IFQ sites of lines_ms_asm.hpp);
  * discrimination: the oracle with and without each claimed line differs by at least 1e-4 of a named cell of O_BY_MOL - a hundred
    times the 1e-6 the GPU module asserts there.  A condition on the inputs, measured here; no kernel is involved;
  * margins: every shifted centre keeps 0.02 cm-1 from its exact 25 cm-1 boundary in every state.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ms_reach_cases as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c) or os.path.exists(c)), None)
DISCRIMINATION = 1e-4

# slots without an edge of a kind, with the reason (the census accepts no other gap)
NO_LINE_BELOW = 1.5      # cm-1: a centre below it cannot be placed 0.25 cm-1 outside with a positive wavenumber to spare


def _why_absent(side, wlo, whi):
    if side == "lo" and wlo - mr.CUT < NO_LINE_BELOW:
        return f"the slot's low edge {wlo - mr.CUT:.2f} cm-1 is not a positive wavenumber a line can have"
    if side == "neg" and mr.CUT - wlo < NO_LINE_BELOW:
        return f"WN + X <= 25 needs X <= {mr.CUT - wlo:.2f} cm-1 for the slot's lowest channel: no such line"
    return None


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    if CXX is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++ or $CXX)")
    exe = tmp_path_factory.mktemp("ms_reach") / "ms_reach_check"
    src = os.path.join(ROOT, "tests", "native", "ms_reach_check.cpp")
    subprocess.run([CXX, "-O1", "-std=c++17", src, "-o", str(exe)], check=True, timeout=300)

    def run(rows):
        """rows: (wn, LPS, every, x, max_abs_shift) -> the words"""
        text = "".join(f"{len(wn)} {lps} {int(every)} {_num(x)} {_num(mas)} " + " ".join(_num(w) for w in wn) + "\n" for wn, lps, every, x, mas in rows)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True, timeout=300).stdout.split()
        assert len(out) == len(rows)
        return [int(v) for v in out]

    return run


def _num(v):
    v = float(v)
    return "nan" if v != v else ("inf" if v == np.inf else ("-inf" if v == -np.inf else v.hex()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the mirror equals ms_reach.hpp
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mirror_equals_header_on_the_cases(native):
    rows = []
    for ll in mr.lists().values():
        wn, mas = ll.wn, ll.mas()
        for l in ll.lines:
            for every in (False, True):
                rows.append((wn, mr.lps_of(len(wn)), every, l.vnu, mas))
    got = native(rows)
    for r, g in zip(rows, got):
        assert g == mr.reach_word(r[0], r[1], r[3], r[4], r[2]), r
    assert len(rows) > 500


def test_mirror_equals_header_on_random_inputs(native):
    rng = np.random.default_rng(20261020)
    rows = []
    for i in range(100000):
        nwn = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 9, 11, 33, 50, 64])) if i % 4 else int(rng.integers(1, 65))
        lps = mr.lps_of(nwn) if i % 7 else int(rng.integers(1, 14))       # (also an LPS the plan would not choose: empty or overfull slots)
        wn = np.sort(rng.uniform(0.1, float(rng.choice([6.0, 40.0, 300.0])), nwn))
        mas = float(rng.choice([0.0, 0.006, 0.1, 2.0]))
        x = float(rng.uniform(0.0, wn[-1] + 60.0))
        if i % 5 == 0:    # on an edge of a slot's hull, to the last bit and one margin either way
            k = int(rng.integers(0, min(mr.WPS, -(-nwn // lps))))
            wlo, whi = wn[lps * k], wn[min(lps * k + lps, nwn) - 1]
            x = float(rng.choice([whi + 25.0, wlo - 25.0, 25.0 - wlo])) + float(rng.choice([-1.0, 0.0, 1.0])) * (mas * 2.0 + 1e-6) * float(rng.choice([1.0, 1.0 + 1e-9, 1.0 - 1e-9]))
        if i % 97 == 0:
            x = float("nan")
        if i % 1009 == 0:
            mas = float("nan")
        rows.append((wn, lps, i % 13 == 0, x, mas))
    got = native(rows)
    bad = [(r, g) for r, g in zip(rows, got) if g != mr.reach_word(r[0], r[1], r[3], r[4], r[2])]
    assert not bad, f"{len(bad)} of {len(rows)} words differ; first: {bad[0]}"
    assert len(set(got)) > 30       # (the inputs spread over the words: an interval of R bits with a prefix of Q bits)


def test_nan_and_every_reach_every_slot_that_holds_a_channel(native):
    for nwn in mr.NWN_SETS:
        wn = mr.channels(nwn)
        full = sum((1 | 256) << k for k, _, _ in mr.slots(wn))
        rows = [(wn, mr.lps_of(nwn), False, float("nan"), 0.1), (wn, mr.lps_of(nwn), True, 500.0, 0.1), (wn, mr.lps_of(nwn), False, 500.0, 0.1)]
        assert native(rows) == [full, full, 0]
        assert [mr.reach_word(*r[:2], r[3], r[4], r[2]) for r in rows] == [full, full, 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# soundness of the margin
# ---------------------------------------------------------------------------------------------------------------------------------
def _random_case(rng):
    nwn = int(rng.integers(1, 65))
    wn = np.sort(rng.uniform(0.1, float(rng.choice([8.0, 40.0, 120.0])), nwn))
    return wn, mr.lps_of(nwn)


def test_margin_is_sound_on_plain_lists():
    """X = vnu + pshift RHORAT and max_abs_shift >= 2 |pshift|: sound for every RHORAT <= 2 (and up to 4, which is why a test of the
    dense word on a plain list needs RHORAT > 4)."""
    rng = np.random.default_rng(1)
    tight = 0
    for _ in range(4000):
        wn, lps = _random_case(rng)
        psh = rng.uniform(-0.06, 0.06, 6).astype(np.float32)
        mas = mr.max_abs_shift(psh)
        rho = np.concatenate([rng.uniform(0.0, 2.0, 5), [2.0]])
        for p in psh:
            k = int(rng.integers(0, len(mr.slots(wn))))
            _, wlo, whi = mr.slots(wn)[k]
            e = float(rng.choice([whi + 25.0, wlo - 25.0, 25.0 - wlo]))
            vnu = e + float(rng.uniform(-0.3, 0.3))
            if vnu <= 0.0:
                continue
            word = mr.reach_word(wn, lps, vnu, mas, False)
            true = mr.true_reach(wn, lps, [vnu + mr.shift_plain(p, r) for r in rho])
            assert true & ~word == 0, (wn, vnu, float(p), mas, bin(true), bin(word))
            tight += int(mr.true_reach(wn, lps, [vnu + mr.shift_plain(p, 4.0 * 1.2)]) & ~word != 0)
    assert tight > 20      # (the draws do come close enough to the edges that a shift of 4.8 x pshift leaves the word)


def test_margin_is_sound_with_species_shifts():
    """X = vnu + delt RHORAT + sum_j rho_j flg_j (shift_j - delt) with sum_j rho_j <= RHORAT and max_abs_shift = 2 |delt| + max_j
    |shift_j|: sound for RHORAT <= 2, and tight there - with delt = 0 and one broadener making up the gas the shift reaches
    max_abs_shift x RHORAT, so half the margin (RHORAT 1 instead of 2) is not enough."""
    rng = np.random.default_rng(2)
    half_fails = 0
    for it in range(4000):
        wn, lps = _random_case(rng)
        n = 5
        delt = (rng.uniform(-0.03, 0.03, n) * (it % 2)).astype(np.float32)
        shifts = rng.uniform(-0.06, 0.06, (n, 7)).astype(np.float32)
        flg = rng.integers(0, 2, (n, 7))
        mas = mr.max_abs_shift(delt, shifts)
        states = []
        for _ in range(5):
            frac = rng.dirichlet(np.full(8, 0.3))[:7] if rng.uniform() < 0.7 else np.eye(7)[int(rng.integers(0, 7))] * rng.uniform(0.9, 1.0)
            states.append((float(rng.choice([rng.uniform(0.0, 2.0), 2.0])), frac))
        for i in range(n):
            k = int(rng.integers(0, len(mr.slots(wn))))
            _, wlo, whi = mr.slots(wn)[k]
            e = float(rng.choice([whi + 25.0, wlo - 25.0, 25.0 - wlo]))
            vnu = e + float(rng.uniform(-0.25, 0.25))
            if vnu <= 0.0:
                continue
            xs = [vnu + mr.shift_ibrd(delt[i], flg[i], shifts[i], frac, r) for r, frac in states]
            word = mr.reach_word(wn, lps, vnu, mas, False)
            true = mr.true_reach(wn, lps, xs)
            assert true & ~word == 0, (wn, vnu, mas, bin(true), bin(word))
            half_fails += int(true & ~mr.reach_word(wn, lps, vnu, 0.5 * mas, False) != 0)
    assert half_fails > 0, "no draw needs more than half the margin: the property would not notice MS_REACH_RHO = 1"


# ---------------------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------------------
def _wave_states(ll, kind):
    profs = mr.batch(kind, ll.wn)
    return profs, mr.waves(profs)


def test_batches_mix_what_the_dense_word_depends_on():
    for nwn in mr.NWN_SETS:
        wn = mr.channels(nwn)
        profs = mr.batch("dense", wn)
        w = mr.waves(profs)
        g = mr.group_size(nwn, len(profs))
        assert 2 <= len(profs) <= 12
        mixed = [st for st in w.values() if is_mixed(st)]
        assert mixed, f"nwn {nwn}: no wave holds a dense state beside an ordinary one"
        assert any(not mr.is_dense(st) for st in w.values())
        if g < len(profs):      # a short last group, and at the bottom layer a wave without a dense state beside one with
            assert len(profs) % g != 0
            assert mr.is_dense(w[(0, 0)]) and not mr.is_dense(w[(g, 0)])
        # the fifth layer of profile 4 is dense and no other profile has it
        (only,) = [st for (p0, lay), st in w.items() if lay == 4]
        assert [i for i, _ in only] == [4] and mr.is_dense(only) and all(p.nlay == 4 for i, p in enumerate(profs) if i != 4)
        assert all(not mr.is_dense(st) for st in mr.waves(mr.batch("mask", wn)).values())
        assert all(float(np.min(p.t)) > 70.0 for p in profs)
    nanb = mr.batch("nan", mr.channels(50))
    assert [i for i, p in enumerate(nanb) if np.isnan(p.p).any()] == [3] and mr.group_size(50, len(nanb)) == 6     # wave-mates: 0 .. 5


def is_mixed(states):
    return any(r > 4.0 for _, r in states) and any(r <= mr.REACH_RHO for _, r in states)


def test_census_of_the_edges():
    """Per channel set, slot, side and type: the claimed line, its twin, what each is claimed to need - and that the group in which
    the kernel meets the claimed line tests a mask and holds no other line with the slot's bit (a neighbour's bit would let it through)."""
    missing, steps_seen = [], set()
    for nwn in mr.NWN_SETS:
        wn = mr.channels(nwn)
        lps = mr.lps_of(nwn)
        allr = [float(r) for kind in ("dense", "mask") for p in mr.batch(kind, wn) for r in mr.rhorat_of(p)]
        for k, wlo, whi in mr.slots(wn):
            for side in ("hi", "lo", "neg"):
                for typ in ("dense", "mask"):
                    ll = mr.lists().get((f"{side}_{typ}_s{k}", nwn))
                    if ll is None:
                        if _why_absent(side, wlo, whi) is None:
                            missing.append((nwn, k, side, typ))
                        continue
                    assert _why_absent(side, wlo, whi) is None
                    (c,) = ll.claimed()
                    (t,) = [i for i, l in enumerate(ll.lines) if l.role == "twin"]
                    assert ll.lines[c].role == typ and ll.lines[c].slot == k and ll.lines[t].mol != ll.lines[c].mol
                    bit = mr.slot_bit(ll.lines[c])
                    mas = ll.mas()
                    words = [mr.reach_word(wn, lps, l.vnu, mas, False) for l in ll.lines]
                    profs, w = _wave_states(ll, ll.batch)
                    needs = [key for key, st in w.items() if mr.true_reach(wn, lps, [mr.shifted(ll, c, r) for _, r in st]) & bit]
                    assert needs, (ll.name, nwn, "the claimed line reaches its slot in no wave")
                    if typ == "dense":
                        # the word lacks the bit, and every wave that needs it holds a state with RHORAT > 4 and is dense
                        assert words[c] & bit == 0
                        assert all(any(r > 4.0 for _, r in w[key]) and mr.is_dense(w[key]) for key in needs)
                    else:
                        # the word has the bit through the margin alone (the table centre lies outside), in a wave that uses its masks
                        assert words[c] & bit and mr.reach_word(wn, lps, ll.lines[c].vnu, 0.0, False) & bit == 0
                        needs = [key for key in needs if not mr.is_dense(w[key])]
                        assert needs
                    for key in needs:
                        (grp,) = [(step, idx) for step, idx in mr.walk_list(ll, profs, 192, states=w[key]) if c in idx]
                        assert grp[0] is not None, (ll.name, nwn, "the claimed line is evaluated without a mask")
                        assert all(words[i] & bit == 0 for i in grp[1] if i != c), (ll.name, nwn, "a neighbour carries the slot's bit")
                        if side == "neg":
                            assert grp[0] in mr.IFQ_STEPS
                        steps_seen.add(grp[0])
                    # the twin reaches the slot in no state of any batch
                    assert mr.true_reach(wn, lps, [mr.shifted(ll, t, r) for r in allr]) & bit == 0
    assert not missing, f"no line for {missing}"
    # all three kinds of ms_eval_run meet an edge line (the single two-resonance line belongs to the pattern lists)
    assert steps_seen >= {"MS_SINGLE1", "MS_PAIR1", "MS_PAIR2", "MS_PAIR1_K1", "MS_PAIR2_K1", "MS_PAIR1_K2"}, steps_seen


def test_census_of_the_species_shifts():
    """With species shifts the margin is tight: the mask line needs more than half of it in a wave that uses its masks (a margin of
    max_abs_shift x 1 would drop it), the dense line needs the dense word at RHORAT 3 - within what a plain list's margin covers."""
    wn = mr.channels(50)
    lps = mr.lps_of(50)
    for typ in ("mask", "dense"):
        ll = mr.lists()[(f"ibrd_{typ}", 50)]
        (c,) = ll.claimed()
        bit = mr.slot_bit(ll.lines[c])
        assert ll.mas() == pytest.approx(mr.IBRD_SHIFT, rel=1e-6)
        words = [mr.reach_word(wn, lps, l.vnu, ll.mas(), False) for l in ll.lines]
        profs, w = _wave_states(ll, ll.batch)
        assert all(p.ibrd == 1 for p in profs)
        needs = [key for key, st in w.items() if mr.true_reach(wn, lps, [mr.shifted(ll, c, r) for _, r in st]) & bit]
        assert needs
        if typ == "mask":
            assert words[c] & bit and mr.reach_word(wn, lps, ll.lines[c].vnu, 0.5 * ll.mas(), False) & bit == 0
            assert all(not mr.is_dense(w[key]) for key in needs)
        else:
            assert words[c] & bit == 0 and all(mr.is_dense(w[key]) and max(r for _, r in w[key]) < 4.0 for key in needs)
        for key in needs:
            (grp,) = [(step, idx) for step, idx in mr.walk_list(ll, profs, 192, states=w[key]) if c in idx]
            assert grp[0] == "MS_PAIR1" and all(words[i] & bit == 0 for i in grp[1] if i != c)


def test_tile_ends_are_on_sorted_molecules():
    """The candidate window of a sorted molecule pads with max_abs_shift x max(RHORAT, 1): the dense lines at the tile's own two ends
    (slot 0's low edge where it exists, the last slot's high edge) lie beyond the window that RHORAT = 1 would give."""
    n = 0
    for (name, nwn), ll in mr.lists().items():
        if not name.startswith(("hi_dense", "lo_dense")):
            continue
        wn = ll.wn
        for mol in {l.mol for l in ll.lines}:
            v = [l.vnu for l in ll.lines if l.mol == mol]
            assert v == sorted(v)
        last = mr.slots(wn)[-1][0]
        for l in ll.lines:
            if l.role == "dense" and ((l.side == "hi" and l.slot == last) or (l.side == "lo" and l.slot == 0)):
                pad1 = ll.mas() * 1.0 + 1e-6
                assert not (wn[0] - 25.0 - pad1 <= l.vnu <= wn[-1] + 25.0 + pad1)
                pad58 = ll.mas() * 5.8 + 1e-6
                assert wn[0] - 25.0 - pad58 <= l.vnu <= wn[-1] + 25.0 + pad58
                n += 1
    assert n >= len(mr.NWN_SETS) + 1      # every set's top end, and the low end of the 5-channel set


EXPECTED_SITES = {("MS_QUAD1", 4), ("MS_PAIR1", 2), ("MS_PAIR2", 2), ("MS_SINGLE1", 1), ("MS_SINGLE2", 1), ("MS_PAIR1_K1", 2), ("MS_PAIR2_K1", 2), ("MS_PAIR1_K2", 2)}
# (step, mask, position) that cannot occur, with the reason: none - every site of the header is reached at every position
CANNOT = {}


def test_census_of_the_patterns():
    """A lone reaching line at every position of every group that tests a mask, for both chunk sizes the GPU module runs.  The steps
    come from the MS_IFK / MS_IFQ sites of lines_ms_asm.hpp; a site the header gains fails here until a pattern reaches it."""
    with open(os.path.join(ROOT, "monortm_amd", "csrc", "lines_ms_asm.hpp")) as f:
        sites = mr.mask_sites(f.read())
    assert sites == EXPECTED_SITES, sites ^ EXPECTED_SITES
    want = {(step, mask, pos) for step, n in sites for pos in range(n) for mask in (("Q", "R0") if step in mr.IFQ_STEPS else ("R",))}
    for ms_items in (64, 192):
        seen = set()
        for name, nwn in (("patterns_r", 5), ("patterns_q", 50)):
            ll = mr.lists()[(name, nwn)]
            wn, lps = ll.wn, mr.lps_of(nwn)
            profs = mr.batch(ll.batch, wn)
            # the words are what every state sees: no line of a pattern list comes near a boundary, margin or not
            allr = [float(r) for p in profs for r in mr.rhorat_of(p)]
            for i, l in enumerate(ll.lines):
                word = mr.reach_word(wn, lps, l.vnu, ll.mas(), False)
                assert mr.true_reach(wn, lps, [mr.shifted(ll, i, r) for r in allr]) == word == mr.reach_word(wn, lps, l.vnu, 0.0, False)
                assert word & 31, "every line of a pattern list reaches some slot: a wrong skip shows"
            steps = mr.walk_list(ll, profs, ms_items)
            assert all(step is None or (step, len(idx)) in sites for step, idx in steps)
            assert sorted(i for _, idx in steps for i in idx) == list(range(len(ll.lines)))     # every line is walked once
            seen |= mr.lone_positions(ll, profs, ms_items)
        gap = {w for w in want - seen if w not in CANNOT}
        assert not gap, f"ms_items {ms_items}: no lone reaching line at {sorted(gap)}"
        assert not set(CANNOT) & seen


# ---------------------------------------------------------------------------------------------------------------------------------
# discrimination and margins
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_claimed_line_shows_in_a_named_cell(workdir):
    worst = (np.inf, None)
    n = 0
    for key, (ll, kind) in mr.runs().items():
        if kind == "nan" or not ll.claimed():
            continue
        cells = mr.named_cells(ll, kind, workdir)
        for c, cell in cells.items():
            assert cell is not None, f"{key}: line {c} is inside its boundary in no state of the batch"
            prof, lay, m, ch, rel, val = cell
            l = ll.lines[c]
            assert rel >= DISCRIMINATION, (f"{key}: without the {l.role} line of slot {l.slot} ({l.side}, molecule {l.mol}, {l.vnu:.3f} cm-1) the cell (profile {prof}, "
                                           f"layer {lay}, molecule {m + 1}, channel {ch}) moves by {rel:.2e} of itself")
            assert mr.lps_of(ll.nwn) * l.slot <= ch < mr.lps_of(ll.nwn) * (l.slot + 1)
            worst = min(worst, (rel, key))
            n += 1
    print(f"{n} claimed lines; the least change of a named cell: {worst[0]:.2e} ({worst[1]})")
    assert n >= 100


def test_margins_from_the_exact_boundaries():
    """Claimed lines and twins keep 0.02 cm-1 from their 25 cm-1 boundary in every state of every batch they run on; a dense line is
    0.02 - 0.06 cm-1 inside at RHORAT 5.84 and outside wherever RHORAT <= 4, a mask line 0.02 - 0.06 inside at RHORAT 1.9."""
    for key, (ll, kind) in mr.runs().items():
        rhos = sorted({float(r) for p in mr.batch(kind, ll.wn) for r in mr.rhorat_of(p) if r == r})
        for i, l in enumerate(ll.lines):
            if l.role not in ("dense", "mask", "twin"):
                continue
            ins = [mr.inside(ll, i, mr.shifted(ll, i, r)) for r in rhos]
            assert min(abs(v) for v in ins) >= mr.MARGIN, (key, i, ins)
            if l.role == "twin":
                assert max(ins) <= -0.05 + 1e-12
            elif l.role == "dense" and kind == "ibrd_dense":
                r3 = max(rhos)
                assert 2.9 < r3 < 3.1 and 0.02 <= mr.inside(ll, i, mr.shifted(ll, i, r3)) <= 0.06 and all(v < 0 for v, r in zip(ins, rhos) if r <= 2.0)
            elif l.role == "dense" and kind == "dense":
                assert 0.02 <= mr.inside(ll, i, mr.shifted(ll, i, max(rhos))) <= 0.06 and max(rhos) > 5.8
                assert all(v < 0 for v, r in zip(ins, rhos) if r <= 4.0)
            elif l.role == "mask":
                r19 = max(r for r in rhos if r <= 2.0)
                assert 1.85 < r19 < 1.95 and 0.02 <= mr.inside(ll, i, mr.shifted(ll, i, r19)) <= 0.06


def test_voigt_by_shift(workdir):
    """The channel beside the 20.3 cm-1 line is more than 100 Doppler widths from the table centre and less from the shifted one in
    the 1 hPa layer, zeta <= 0.99, and the oracle does evaluate a Voigt shape there - for that line alone in the file."""
    from monortm_amd import tape3
    from oracle.pyoracle import Oracle

    ll = mr.lists()[("voigt_shift", 50)]
    wn = ll.wn
    (v,) = [i for i, l in enumerate(ll.lines) if l.role == "voigt"]
    profs = mr.batch("voigt", wn)
    rho, t = float(mr.rhorat_of(profs[0])[3]), float(profs[0].t[3])
    hwd = mr.lc.DOP * np.sqrt(t / mr.lc.MASS[mr.O3]) * mr.VOIGT_CENTRE
    d0 = float(np.min(np.abs(wn - ll.lines[v].vnu)))
    d1 = float(np.min(np.abs(wn - mr.shifted(ll, v, rho))))
    assert d0 > 100.0 * hwd * 1.2 and d1 < 100.0 * hwd * 0.9, (d0, d1, 100.0 * hwd)
    hw_hi = 0.08 * rho * (296.0 / t) ** 0.75
    assert hw_hi / (hw_hi + hwd) <= 0.99
    rec = mr.records(ll)
    one = tape3.LineRecords(**{k: np.asarray(getattr(rec, k))[[v]] for k in ("vnu", "sp", "alfa", "epp", "mol", "hwhm", "tmpalf", "pshift", "iflg", "sdep")})
    path = f"{workdir}/TAPE3_msr_voigt_one"
    tape3.write_tape3(path, one)
    orc = Oracle(path, wn[0], wn[-1])
    orc.census(reset=True)
    orc.run(profs[0])
    assert orc.census()["voigt"] > 0
    orc.close()
