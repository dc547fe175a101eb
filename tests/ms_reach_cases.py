"""Constructed cases for the slot masks of lines_ms_kernel (monortm_amd/csrc/ms_reach.hpp, ms_reach_kernel and the dense word of
ms_prologue in lines_ms_kernel.hip; the masks are tested by MS_IFK / MS_IFQ in lines_ms_asm.hpp), and a Python mirror of the rule.

tests/test_ms_reach_cpu.py holds the mirror to the header bit for bit, proves the margin sound, counts what the cases reach and
measures - with the oracle, on the CPU - that every claimed line shows in a named cell; tests/test_ms_reach.py runs the cases on the GPU.

The rule.  Slot k of a wave = the k-th wavenumbers of its lanes = channels k LPS .. k LPS + LPS - 1 of every state, LPS = ceil(nwn / 5).
Bit k of a line's word: it can come within 25 cm-1 of a channel of slot k (hull [wlo - 25, whi + 25]); bit 8 + k: its negative
resonance can (WN + Xnu <= 25: Xnu <= 25 - wlo).  Both from the table centre with a margin pad = max_abs_shift x 2 + 1e-6, where
max_abs_shift = max over the list of 2 |delt| + max_j |species shift_j| (line_table.cpp).  The actual centre is
    X = vnu + pshift_as_stored_REAL4 x RHORAT                                                     (plain)
    X = vnu + delt RHORAT + sum_j rho_j flg_j (shift_j - delt),  rho_j = RHORAT wk_j / WTOT       (IBRD, lines_device.hpp)
so on a plain list the margin holds up to RHORAT = 4, with species shifts only up to 2.  A wave that holds a state with
RHORAT > 2 (or a NaN one) uses no mask (the dense word).

Lists (one TAPE3 block each, built for a channel set; H2O 1, CO2 2, O3 3, O2 7).  The loops test a mask for a GROUP of lines (four,
two, one), so an edge list holds ONE claimed line: its molecule holds besides it only a partner 3.25 cm-1 outside (no bit of the slot), its
twin lives in another molecule (_edge_list):
    hi_dense_sK / lo_dense_sK   the upper / lower edge of slot K's hull: the table centre lies pad + 0.05 = 0.25 cm-1 OUTSIDE and the shifted centre
                           0.04 cm-1 inside at RHORAT 5.84 (|pshift| = 0.05 cm-1/atm): only the dense word lets the line through.  At RHORAT <= 3
                           it stays 0.1 cm-1 outside.  The twin: 0.05 cm-1 outside, its shift points outward (outside in every state).
    hi_mask_sK / lo_mask_sK     the same with the table centre 0.072 cm-1 outside: 0.023 cm-1 inside at RHORAT 1.9, 0.021 outside at 1.014 - the
                           masks are in force and it is the margin that keeps the line
    neg_dense_sK / neg_mask_sK  the same for bits 8 .. 12: centres around 25 - wlo (generic molecules: CO2 has no negative resonance, O2 no Q mask)
    ibrd_mask / ibrd_dense species shifts (delt = 0, a CO2 shift of 0.1 cm-1/atm in a CO2 atmosphere): the shift reaches 0.955 x max_abs_shift x
                           RHORAT, so the margin is tight at RHORAT 1.9 and the dense word is needed at RHORAT 3
    patterns_r             nwn = 5 (channels 60 cm-1 apart, a line reaches at most one slot): per kind an unsorted molecule whose lines reach
                           slot 1 only ("a") or slot 2 only ("b"); runs put a lone "a" at every position of every group
    patterns_q             nwn = 50: two-resonance lines; "a" at 15.5 (Q bits 0, 1) among "b" at 20 (Q bit 0) for the Q masks, "a" at 20 (every
                           R bit) among "c" at 5 (R bit 4 clear) for the R masks behind a clear Q bit
    voigt_shift            |pshift| = 1 cm-1/atm and a 1 hPa top layer: a channel more than 100 Doppler widths from the table centre and
                           less from the shifted one (the near_lb shortcut of ms_prepare)
A line 0.04 cm-1 inside 25 cm-1 adds 2 x 0.04 / 25^3 of its amplitude, a line 8 cm-1 from the channel 1 / 64: at a hull edge the claimed
line is alone in its cell; at the negative-resonance limit its own positive resonance is the rest of the cell (neg_fraction).

States.  Four layers; the bottom one is ORD 1000 hPa / 288 K (RHORAT 1.014), R19 1887 / 290 (1.90), R3 3000 / 292 (3.00) or R58
3000 / 150 (5.84); above it 200 hPa / 220 K, 50 / 215, 1 / 250.  cntnm = 0: the line sum is the total.
"""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass

import numpy as np

import line_class_cases as lc
from monortm_amd import synth, tape3

H2O, CO2, O3, O2 = lc.H2O, lc.CO2, lc.O3, lc.O2
WPS = 5
REACH_RHO = 2.0
CUT = 25.0
NWN_SETS = (5, 50, 64, 33, 7, 6, 1)
NPROF = {5: 7, 50: 8, 64: 6, 33: 11, 7: 7, 6: 7, 1: 7}      # (twelve states a wave do not fit the LDS: modm_plan.hpp keeps lines_kernel then)
PSHIFT = 0.05
OUT_DENSE, OUT_MASK, OUT_TWIN = 0.25, 0.072, 0.05
MARGIN = 0.02
BOTTOM = {"ORD": (1000.0, 288.0), "R19": (1887.0, 290.0), "R3": (3000.0, 292.0), "R58": (3000.0, 150.0)}
UPPER_P = np.array([200.0, 50.0, 1.0])
UPPER_T = np.array([220.0, 215.0, 250.0])
LEVEL_T = np.array([289.0, 250.0, 217.0, 230.0, 255.0])
LAYER_DP = np.array([100.0, 60.0, 30.0, 0.5])


def lps_of(nwn: int) -> int:
    return (nwn + WPS - 1) // WPS


# ---------------------------------------------------------------------------------------------------------------------------------
# the mirror
# ---------------------------------------------------------------------------------------------------------------------------------
def reach_word(wn, LPS: int, vnu: float, mas: float, every: bool) -> int:
    """ms_reach.hpp restated: the 16-bit word of a table line at vnu for the ascending channels wn."""
    wn = [float(w) for w in wn]
    nwn = len(wn)
    pad = mas * REACH_RHO + 1e-6
    r = 0
    for k in range(WPS):
        c0 = LPS * k
        if c0 >= nwn:
            break
        wlo, whi = wn[c0], wn[min(c0 + LPS, nwn) - 1]
        if every or (not (vnu - pad - 25.0 > whi) and not (wlo - 25.0 > vnu + pad)):
            r |= 1 << k
        if every or not (wlo + (vnu - pad) > 25.0):
            r |= 256 << k
    return r


def true_reach(wn, LPS: int, xs) -> int:
    """The slots a line does reach: bit k, some (state, channel of slot k) has |WN - X| <= 25; bit 8 + k, some has WN + X <= 25.
    xs: the shifted centre per state."""
    wn = np.asarray(wn, float)
    r = 0
    for k in range(WPS):
        w = wn[LPS * k: LPS * k + LPS]
        if not len(w):
            break
        for x in xs:
            if np.any(np.abs(w - x) <= CUT):
                r |= 1 << k
            if np.any(w + x <= CUT):
                r |= 256 << k
    return r


def shift_plain(pshift: float, rhorat: float) -> float:
    return float(np.float32(pshift)) * rhorat


def shift_ibrd(delt: float, flg, shifts, frac, rhorat: float) -> float:
    """lines_device.hpp:1413-1425: delt RHORAT + sum_j rho_j flg_j (shift_j - delt) with rho_j = RHORAT frac_j, frac_j = wk_j / WTOT
    (the fractions of the seven broadeners: their sum is at most 1)."""
    delt = float(np.float32(delt))
    s = delt * rhorat
    for j in range(7):
        s += rhorat * float(frac[j]) * int(flg[j]) * (float(np.float32(shifts[j])) - delt)
    return s


def max_abs_shift(pshift, shifts=None) -> float:
    """line_table.cpp:219-226 for a list without the O2 self-shift correction: max over the lines of 2 |delt| + max_j |shift_j|."""
    p = np.abs(np.asarray(pshift, np.float32).astype(np.float64))
    mx = np.zeros_like(p) if shifts is None else np.abs(np.asarray(shifts, np.float32).astype(np.float64)).reshape(len(p), -1).max(axis=1)
    return float(np.max(2.0 * p + mx)) if len(p) else 0.0


def slots(wn):
    """[(k, wlo, whi)] of the slots that hold a channel."""
    wn = np.asarray(wn, float)
    L = lps_of(len(wn))
    return [(k, float(wn[L * k]), float(wn[min(L * k + L, len(wn)) - 1])) for k in range(WPS) if L * k < len(wn)]


# ---------------------------------------------------------------------------------------------------------------------------------
# channels, states, batches
# ---------------------------------------------------------------------------------------------------------------------------------
def channels(nwn: int) -> np.ndarray:
    if nwn == 5:
        return np.array([30.0, 90.0, 150.0, 210.0, 270.0])
    if nwn == 7:
        return np.array([2.0, 4.0, 8.0, 9.5, 16.0, 18.0, 32.0])
    if nwn == 6:
        return np.array([2.0, 4.0, 8.0, 9.5, 16.0, 18.0])
    if nwn == 1:
        return np.array([3.0])
    return np.linspace(0.5, 40.0, nwn)


CO2_MIX = np.array([1.0e-2, 0.95, 1e-7, 3e-7, 1e-7, 1.6e-6, 5e-3])     # a CO2 atmosphere: wk_j / air, with 0.03 of other broadeners
CO2_FRACTION = float(CO2_MIX[1] / (CO2_MIX.sum() + 0.03))              # wk_CO2 / WTOT = 0.9548


def profile(wn, bottom="ORD", fc=1.0, dense_top=False, nan_layer=None, co2=False) -> synth.Profile:
    pb, tb = BOTTOM[bottom]
    p = np.concatenate([[pb], UPPER_P])
    t = np.concatenate([[tb], UPPER_T])
    tz = LEVEL_T.copy()
    dp = LAYER_DP.copy()
    vmr = lc.VMR.copy()
    if dense_top:      # a fifth layer, denser than the masks allow, that no other profile of the batch has
        p, t, tz, dp = np.append(p, BOTTOM["R58"][0]), np.append(t, BOTTOM["R58"][1]), np.append(tz, 160.0), np.append(dp, 100.0)
        vmr = np.vstack([vmr, vmr[0]])
    if nan_layer is not None:
        p[nan_layer] = np.nan
    air = 2.1e25 * dp / 1013.0 * fc
    if co2:
        return synth.Profile(wn=np.asarray(wn, float), p=p, t=t, tz=tz, wkl=CO2_MIX[None, :] * air[:, None], wbrodl=0.03 * air, clw=np.zeros(len(p)), irt=3,
                             cntnm=np.zeros(7), ibrd=1)
    return synth.Profile(wn=np.asarray(wn, float), p=p, t=t, tz=tz, wkl=vmr * air[:, None], wbrodl=0.781 * air, clw=np.zeros(len(p)), irt=3,
                         cntnm=np.zeros(7))


_ORDER = {"dense": ("ORD", "R19", "R58", "R3", "ORD", "R19", "ORD", "R19", "ORD", "ORD", "R19", "ORD"),
          "mask": ("ORD", "R19", "ORD", "ORD", "R19", "ORD", "R19", "ORD", "ORD", "R19", "ORD", "ORD")}


def batch(kind: str, wn) -> list:
    """dense: every bottom state; profile 2 (R58) and profile 3 (R3) make the bottom wave of the first group dense, profile 4 has a
    fifth layer of RHORAT 5.84 that no other profile has; the last group (where the group is smaller than the batch) holds no dense
    state.  mask: ORD and R19 only - every wave uses its masks.  nan: mask with a NaN pressure in layer 1 of profile 3.  voigt: ORD."""
    n = NPROF[len(wn)]
    if kind == "voigt":
        return [profile(wn, "ORD", fc=1.0 + 0.05 * i) for i in range(min(n, 7))]
    if kind.startswith("ibrd"):   # species shifts: R19 is the densest state of the mask batch, R3 (dense word) of the dense one
        order = ("ORD", "R19", "R3" if kind == "ibrd_dense" else "ORD", "ORD", "R19", "ORD", "R19", "ORD")
        return [profile(wn, order[i], fc=1.0 + 0.07 * (i % 5), co2=True) for i in range(n)]
    order = _ORDER["mask" if kind == "nan" else kind]
    return [profile(wn, order[i], fc=1.0 + 0.07 * (i % 5), dense_top=(kind == "dense" and i == 4), nan_layer=(1 if kind == "nan" and i == 3 else None))
            for i in range(n)]


def rhorat_of(pr) -> np.ndarray:
    return lc.rhorat(pr.p, pr.t)


def group_size(nwn: int, nprof: int) -> int:
    return min(12, 64 // lps_of(nwn), nprof)


def waves(profs):
    """The states of every wave: (first profile, layer) -> [(profile, RHORAT)] over the profiles of the group that have the layer."""
    nwn, n = profs[0].nwn, len(profs)
    g = group_size(nwn, n)
    out = {}
    for p0 in range(0, n, g):
        for lay in range(max(p.nlay for p in profs)):
            st = [(i, float(rhorat_of(profs[i])[lay])) for i in range(p0, min(p0 + g, n)) if lay < profs[i].nlay]
            if st:
                out[(p0, lay)] = st
    return out


def is_dense(states) -> bool:
    return any(not (r <= REACH_RHO) for _, r in states)


# ---------------------------------------------------------------------------------------------------------------------------------
# line lists
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Line:
    mol: int
    vnu: float
    pshift: float
    mult: float = 1.0       # strength over the molecule's base strength
    role: str = ""          # dense, mask, twin, a, b, c, voigt, filler
    slot: int = -1
    side: str = ""          # hi, lo, neg
    brd_shift: float | None = None     # the line carries a CO2 broadening record with this shift (and delt = pshift)


@dataclass
class LineList:
    name: str
    nwn: int
    lines: list
    batch: str              # the batch kind it is run on

    @property
    def wn(self):
        return voigt_channels(self) if self.name == "voigt_shift" else channels(self.nwn)

    def claimed(self):
        return [i for i, l in enumerate(self.lines) if l.role in ("dense", "mask")]

    def mas(self):
        return max_abs_shift([l.pshift for l in self.lines], [[l.brd_shift or 0.0] for l in self.lines])


def records(ll: LineList, without=None) -> tape3.LineRecords:
    """TAPE3 records: widths, lower-state energies and exponents from a generator seeded per line index (so that a list without
    one line keeps the parameters of the others)."""
    cols = {k: [] for k in ("vnu", "sp", "alfa", "epp", "mol", "hwhm", "tmpalf", "pshift", "iflg", "sdep")}
    for i, l in enumerate(ll.lines):
        if i == without:
            continue
        rng = np.random.default_rng(1000 + i)
        s = 10.0 ** lc.S_LOG[l.mol] * l.mult
        alfa, hwhm = rng.uniform(0.05, 0.08), rng.uniform(0.05, 0.08)
        if l.mol == O2:
            alfa, hwhm = rng.uniform(0.04, 0.06), rng.uniform(0.03, 0.06)
        row = dict(vnu=l.vnu, sp=s / (l.vnu * (1.0 - np.exp(-synth.RADCN2 * l.vnu / 296.0))), alfa=alfa, epp=rng.uniform(50.0, 400.0), mol=l.mol + 100,
                   hwhm=hwhm, tmpalf=rng.uniform(0.6, 0.75), pshift=l.pshift, iflg=0, sdep=0.0)
        for k, v in row.items():
            cols[k].append(v)
    rec = tape3.LineRecords(**{k: np.asarray(v) for k, v in cols.items()})
    for j, l in enumerate(l for i, l in enumerate(ll.lines) if i != without):
        if l.brd_shift is not None:     # CO2 as the broadener (species 2): width, temperature exponent, shift
            rec.brd_flg[j, CO2 - 1] = 1
            rec.brd_dat[j, 3 * (CO2 - 1): 3 * CO2] = (0.07, 0.7, l.brd_shift)
    assert len(rec) <= min(200, tape3.NLINEREC)
    return rec


FAR = 3.0          # cm-1 beyond the twin's place: the partner that shares the claimed line's group and does not reach the slot


def _edge_list(nwn: int, side: str, typ: str, k: int):
    """One claimed line per list.  The loops test a mask for a GROUP of lines (four, two or one), so a neighbour that carries the
    slot's bit would let the claimed line through whatever its own bit says: the claimed line shares its molecule - hence its
    group - only with a partner 3.25 cm-1 outside the boundary (no bit of the slot), and its twin (which has the bit, through the margin)
    lives in another molecule.  Both orders ascend: the molecule is sorted and the candidate window applies.  The lines at the tile's
    own ends sit in a generic molecule: there the window drops the partner, and a single O2 / CO2 line is evaluated without a
    mask (ms_eval_run, n == 1).  Negative resonance: generic molecules only - the O2 loops decide it per lane, without the Q masks."""
    wn = channels(nwn)
    sl = slots(wn)
    _, wlo, whi = sl[k]
    e, out = {"hi": (whi + CUT, 1.0), "lo": (wlo - CUT, -1.0), "neg": (CUT - wlo, 1.0)}[side]
    if e - 0.5 < 1.0:
        return None                   # (no line at or below 0 cm-1: the slot has no such edge)
    tile_end = (side == "hi" and k == sl[-1][0]) or (side == "lo" and k == 0)
    if side == "neg" or tile_end:
        mol = (H2O, O3)[(k + (typ == "dense")) % 2]
    else:
        mol = (CO2, O2, O3, H2O)[(k + nwn + 2 * (typ == "dense") + (side == "lo")) % 4]
    other = O3 if mol == H2O else H2O
    lines = [Line(mol, e + out * (OUT_DENSE if typ == "dense" else OUT_MASK), -out * PSHIFT, 1.0, typ, k, side),
             Line(other, e + out * OUT_TWIN, out * PSHIFT, 1.0 / 30.0, "twin", k, side)]
    far = e + out * (OUT_DENSE + FAR)
    if far > 0.5:
        lines.append(Line(mol, far, out * 0.01, 1.0 / 30.0, "partner", k, side))
    if side == "lo":   # (the reader drops a block that ends below wn[0] - 25: a line far above keeps the block, and reaches nothing)
        lines.append(Line(other, float(wn[-1]) + 60.0, 0.01, 1.0 / 30.0, "anchor", k, side))
    lines.sort(key=lambda l: (l.mol, l.vnu))
    return LineList(f"{side}_{typ}_s{k}", nwn, lines, typ)


IBRD_SHIFT = 0.1


def _ibrd_list(typ: str) -> LineList:
    """Species shifts, nwn = 50, the high edge of slot 1, O3: delt = 0 and a CO2 shift of 0.1 cm-1/atm in a gas that is 95 % CO2 - the
    centre moves by 0.955 x 0.1 x RHORAT, close to max_abs_shift x RHORAT, so the margin of the words is tight at RHORAT 2: the
    mask line lies 0.15 cm-1 outside (0.03 inside at RHORAT 1.9; half the margin would drop it), the dense line 0.25 cm-1 outside
    (0.036 inside at RHORAT 3.0, where the dense word must serve).  Twin and partner as in the plain lists."""
    wn = channels(50)
    _, wlo, whi = slots(wn)[1]
    e = whi + CUT
    lines = [Line(O3, e + (0.25 if typ == "dense" else 0.15), 0.0, 1.0, typ, 1, "hi", brd_shift=-IBRD_SHIFT),
             Line(O3, e + OUT_DENSE + FAR, 0.0, 1.0 / 30.0, "partner", 1, "hi", brd_shift=IBRD_SHIFT),
             Line(H2O, e + OUT_TWIN, 0.0, 1.0 / 30.0, "twin", 1, "hi", brd_shift=IBRD_SHIFT)]
    lines.sort(key=lambda l: (l.mol, l.vnu))
    return LineList(f"ibrd_{typ}", 50, lines, f"ibrd_{typ}")


PATTERN_R = ((H2O, 21, 0, ()), (CO2, 21, 1, ()), (O3, 23, 0, ()), (O2, 21, 3, ()))     # molecule, lines, phase of the "a" lines, further "a" lines


def _pattern_r(spec=None) -> LineList:
    """nwn = 5, channels 30 / 90 / 150 / 210 / 270: "a" lines 8 - 12 cm-1 from 90 (slot 1 alone), "b" lines 8 - 12 cm-1 from 150 (slot 2 alone).
    Per molecule every fifth line, the last one and a few more are "a": with the molecules' line counts they fall on every position
    of the groups of four, the pairs and the odd last line, whether the chunks hold 9 or 21 lines (test_census_of_the_patterns)."""
    lines = []
    for mol, n, phase, more in (PATTERN_R if spec is None else spec):
        for i in range(n):
            a = (i + phase) % 5 == 0 or i == n - 1 or i in more
            base = 90.0 if a else 150.0
            lines.append(Line(mol, base + (8.0 + 0.15 * i) * (1.0 if i % 2 else -1.0), 0.002 * (1.0 if i % 3 else -1.0), 1.0, "a" if a else "b", 1 if a else 2, "r"))
    return LineList("patterns_r", 5, lines, "mask")


def _pattern_q() -> LineList:
    """nwn = 50, 0.5 .. 40 cm-1: two-resonance lines.  O3: "a" at 15.5 (Q bits 0 and 1) among "b" at 20 (Q bit 0): a lone line in
    Q_1.  H2O and O2: "a" at 20 (reaches every slot) among "c" at 5 (does not reach slot 4, 32.7 .. 40): a lone line in R_4 behind a clear
    Q bit.  Centres keep 0.1 cm-1 from every channel."""
    wn = channels(50)
    lines = []

    def put(mol, i, base, role, slot):
        x = base + 0.013 * i
        while np.min(np.abs(wn - x)) < 0.1:
            x += 0.05
        lines.append(Line(mol, x, 0.002 * (1.0 if i % 3 else -1.0), 1.0, role, slot, "q" if mol == O3 else "r"))

    for i in range(23):
        a = i % 5 == 0 or i == 22
        put(O3, i, 15.5 if a else 20.0, "a" if a else "b", 1)
    for mol, n, phase in ((H2O, 23, 1), (O2, 22, 2)):     # (O2's loops test no Q mask: its pairs of two-resonance lines test R alone)
        for i in range(n):
            a = (i + phase) % 5 == 0 or i == n - 1
            put(mol, i, 20.0 if a else 5.0, "a" if a else "c", 4)
    return LineList("patterns_q", 50, lines, "mask")


VOIGT_CENTRE, VOIGT_OFFSET, VOIGT_PSHIFT = 20.3, 0.0025, 1.0


def _voigt_shift() -> LineList:
    """O3: the line at 20.3 cm-1 with pshift = +1 cm-1/atm; a channel 0.0025 cm-1 above its table centre.  In the 1 hPa / 250 K layer
    (RHORAT 1.17e-3) the centre moves 1.17e-3 cm-1 towards the channel: 0.00133 cm-1 away, and 100 Doppler widths are 0.00166 cm-1
    (HWHM_D = 3.5812e-7 sqrt(250 / 48) x 20.3 = 1.66e-5); zeta = HW / (HW + HWD) ~ 0.85.  Other O3 lines 3 cm-1 and more away."""
    lines = [Line(O3, VOIGT_CENTRE, VOIGT_PSHIFT, 1.0, "voigt", -1, "")]
    for i, x in enumerate((6.2, 11.7, 17.1, 24.4, 29.9, 36.3)):
        lines.append(Line(O3, x, 0.5 * (1.0 if i % 2 else -1.0), 1.0, "filler"))
    for i, x in enumerate((9.3, 27.2)):
        lines.append(Line(O2, x, -0.5, 1.0, "filler"))
    lines.sort(key=lambda l: (l.mol, l.vnu))
    return LineList("voigt_shift", 50, lines, "voigt")


def voigt_channels(ll: LineList) -> np.ndarray:
    wn = channels(ll.nwn).copy()
    j = int(np.argmin(np.abs(wn - VOIGT_CENTRE)))
    wn[j] = VOIGT_CENTRE + VOIGT_OFFSET
    assert np.all(np.diff(wn) > 0)
    return wn


@functools.lru_cache(maxsize=None)
def lists() -> dict:
    out = {}
    for nwn in NWN_SETS:
        for side in ("hi", "lo", "neg"):
            for typ in ("dense", "mask"):
                for k, _, _ in slots(channels(nwn)):
                    ll = _edge_list(nwn, side, typ, k)
                    if ll is not None:
                        out[(ll.name, nwn)] = ll
    for ll in (_pattern_r(), _pattern_q(), _voigt_shift(), _ibrd_list("mask"), _ibrd_list("dense")):
        out[(ll.name, ll.nwn)] = ll
    return out


def runs():
    """Every (list, channel set, batch) the GPU module runs: key -> (LineList, batch kind).  The NaN batch on the two 50-channel mask lists."""
    out = {}
    for (name, nwn), ll in lists().items():
        out[f"{name}-{nwn}-{ll.batch}"] = (ll, ll.batch)
    for name in ("hi_mask_s0", "hi_mask_s2", "neg_mask_s1"):
        out[f"{name}-50-nan"] = (lists()[(name, 50)], "nan")
    return out


def shifted(ll: LineList, i: int, rhorat: float) -> float:
    l = ll.lines[i]
    if ll.batch.startswith("ibrd") and l.brd_shift is not None:
        flg, sh, frac = np.zeros(7, int), np.zeros(7), np.zeros(7)
        flg[CO2 - 1], sh[CO2 - 1], frac[CO2 - 1] = 1, l.brd_shift, CO2_FRACTION
        return l.vnu + shift_ibrd(l.pshift, flg, sh, frac, rhorat)
    return l.vnu + shift_plain(l.pshift, rhorat)


def edge_of(ll: LineList, i: int) -> float:
    """The exact boundary a claimed line or a twin was placed against."""
    l = ll.lines[i]
    k, wlo, whi = next(s for s in slots(ll.wn) if s[0] == l.slot)
    return {"hi": whi + CUT, "lo": wlo - CUT, "neg": CUT - wlo}[l.side]


def inside(ll: LineList, i: int, x: float) -> float:
    """How far inside its boundary (negative: outside) the centre x of line i lies."""
    e = edge_of(ll, i)
    return (x - e) if ll.lines[i].side == "lo" else (e - x)


def slot_bit(l: Line) -> int:
    return (256 << l.slot) if l.side in ("neg", "q") else (1 << l.slot)


# ---------------------------------------------------------------------------------------------------------------------------------
# discrimination: the cell in which a claimed line shows (oracle, CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def write(ll: LineList, workdir: str, without=None) -> str:
    path = f"{workdir}/TAPE3_msr_{ll.name}_{ll.nwn}" + ("" if without is None else f"_wo{without}")
    tape3.write_tape3(path, records(ll, without))
    return path


_NAMED = {}


def neg_fraction(mol: int, w: float, x: float) -> float:
    """The part of a line's term at channel w that its NEGATIVE resonance adds (a missing Q bit drops that part alone; the oracle can
    only drop the whole line): f- / (f+ + f-) with the Lorentz wings 1 / d^2, less the pedestal 1 / 625 for a generic molecule and
    without one for O2 (modm.f90:706-831).  The width is left out: HW^2 < 0.2 against d^2 > 60 here, under 1 % of either term."""
    ped = 0.0 if mol == O2 else 1.0 / CUT ** 2
    fm = 1.0 / (w + x) ** 2 - ped if w + x <= CUT else 0.0
    fp = 1.0 / (w - x) ** 2 - ped if abs(w - x) <= CUT else 0.0
    return fm / (fm + fp) if fm + fp > 0.0 else 0.0


def named_cells(ll: LineList, kind: str, workdir: str) -> dict:
    """claimed line -> (profile, layer, molecule index, channel, relative change, value with the line): the cell of the batch's
    O_BY_MOL that the line's removal changes most, relative to the cell.  The oracle with and without the line; computed once."""
    from oracle.pyoracle import Oracle

    key = (ll.name, ll.nwn, kind)
    if key in _NAMED:
        return _NAMED[key]
    profs = [p for p in batch(kind, ll.wn)]
    use = [i for i, p in enumerate(profs) if not np.isnan(p.p).any()]

    def obm(path):
        orc = Oracle(path, ll.wn[0], ll.wn[-1])
        out = {i: orc.run(profs[i]).o_by_mol for i in use}
        orc.close()
        return out

    full = obm(write(ll, workdir))
    cells = {}
    L = lps_of(ll.nwn)
    for c in ll.claimed():
        less = obm(write(ll, workdir, without=c))
        best = None
        line = ll.lines[c]
        m = line.mol - 1
        for i in use:
            for lay, rho in enumerate(rhorat_of(profs[i])):
                x = shifted(ll, c, float(rho))
                if not inside(ll, c, x) > 0.0:
                    continue           # (the slot's bit is not needed in this state)
                for ch in range(L * line.slot, min(L * line.slot + L, ll.nwn)):
                    a, b = full[i][lay, m, ch], less[i][lay, m, ch]
                    rel = abs(a - b) / abs(a) * (neg_fraction(line.mol, float(ll.wn[ch]), x) if line.side == "neg" else 1.0) if a != 0.0 else 0.0
                    if best is None or rel > best[4]:
                        best = (i, int(lay), m, int(ch), float(rel), float(a))
        cells[c] = best
    _NAMED[key] = cells
    return cells


# ---------------------------------------------------------------------------------------------------------------------------------
# the walk of a run through the assembly (MS_RUN_K0 / K1 / K2 of lines_ms_asm.hpp) and the mask sites
# ---------------------------------------------------------------------------------------------------------------------------------
def mask_sites(text: str) -> set:
    """(step, lines per group) of every MS_IFK / MS_IFQ site of lines_ms_asm.hpp: the *_ALL macros name the body of slot 0; MS_ALL5 is
    instantiated by MS_CLASS_PAIRS with the pair bodies of O2 and CO2."""
    text = re.sub(r"//[^\n]*", "", text)      # (the comments name the macros too)
    nb = {"15": 4, "3": 2, "1": 1}
    sites = set()
    for m in re.finditer(r'MS_IFK\("r0",\s*(\d+),\s*(MS_\w+)\(', text):
        sites.add((m.group(2), nb[m.group(1)]))
    for m in re.finditer(r'MS_IFQ\("q0",\s*"r0",\s*(\d+),\s*(MS_\w+)\(', text):
        sites.add((m.group(2), nb[m.group(1)]))
    all5 = re.search(r'#define MS_ALL5\(M, Z\) MS_IFK\("r0",\s*(\d+),\s*M\(', text)
    assert all5
    for m in re.finditer(r'MS_CLASS_PAIRS\("\d+",\s*"\d+",\s*(MS_\w+)\)', text):
        sites.add((m.group(1), nb[all5.group(1)]))
    return sites


def walk_run(kind: int, m2bits):
    """The steps of a run of ordinary lines of one molecule within a chunk: [(step, [line offsets])].  kind 0 generic: class ONE (no
    line of the pair has two resonances) in groups of four with an odd pair, class TWO in pairs, the odd last line by itself; kind 1 /
    2 (O2 / CO2): pairs only, the odd last line in C++ without a mask (step None)."""
    n, j, out = len(m2bits), 0, []
    m2 = [bool(b) and kind != 2 for b in m2bits]
    while n - j >= 2:
        two = m2[j] or m2[j + 1]
        k = 0
        while j + 2 * k + 1 < n and (m2[j + 2 * k] or m2[j + 2 * k + 1]) == two:
            k += 1
        if kind == 0 and not two:
            for q in range(k // 2):
                out.append(("MS_QUAD1", [j + 4 * q + i for i in range(4)]))
            if k % 2:
                out.append(("MS_PAIR1", [j + 2 * k - 2, j + 2 * k - 1]))
        else:
            step = {0: "MS_PAIR2", 1: "MS_PAIR2_K1" if two else "MS_PAIR1_K1", 2: "MS_PAIR1_K2"}[kind]
            for q in range(k):
                out.append((step, [j + 2 * q, j + 2 * q + 1]))
        j += 2 * k
    if n - j == 1:
        out.append((("MS_SINGLE2" if m2[j] else "MS_SINGLE1") if kind == 0 else None, [j]))
    return out


def walk_list(ll: LineList, profs, ms_items: int = 192, states=None):
    """Every step of the list in one wave: [(step, [line indices])].  states: the wave's (profile, RHORAT) (default: all states of
    the batch, which must then use their masks).  The candidates: a sorted molecule keeps the lines within max_abs_shift x
    max(RHORAT, 1) + 1e-6 of [wn[0] - 25, wn[-1] + 25], the union over the states; an unsorted one keeps every line.  Molecule by
    molecule in table order, cut into chunks of CL; M2 is the union over the states."""
    wn = ll.wn
    if states is None:
        assert all(not is_dense(st) for st in waves(profs).values())
        states = [(i, float(r)) for i, p in enumerate(profs) for r in rhorat_of(p)]
    rmax = max(r for _, r in states)
    pad = ll.mas() * max(rmax, 1.0) + 1e-6
    order = []
    for mol in sorted({l.mol for l in ll.lines}):
        idx = [i for i, l in enumerate(ll.lines) if l.mol == mol]
        v = [ll.lines[i].vnu for i in idx]
        if all(a <= b for a, b in zip(v[:-1], v[1:])):
            idx = [i for i in idx if wn[0] - CUT - pad <= ll.lines[i].vnu <= wn[-1] + CUT + pad]
        order += idx
    g = lc.ms_layout(len(wn), len(profs), len({l.mol for l in ll.lines}), ms_items)
    assert g is not None
    cl = g[1]
    steps = []
    for c0 in range(0, len(order), cl):
        chunk = order[c0:c0 + cl]
        j = 0
        while j < len(chunk):
            mol = ll.lines[chunk[j]].mol
            e = j
            while e < len(chunk) and ll.lines[chunk[e]].mol == mol:
                e += 1
            run = chunk[j:e]
            m2 = []
            for i in run:
                xs = [shifted(ll, i, r) for _, r in states]
                m2.append(any(wn[0] + x <= CUT for x in xs))
            for step, offs in walk_run(lc.KIND[mol], m2):
                steps.append((step, [run[o] for o in offs]))
            j = e
    return steps


IFQ_STEPS = ("MS_PAIR2", "MS_SINGLE2")      # these test Q first, and R behind a clear Q bit


def lone_positions(ll: LineList, profs, ms_items: int) -> set:
    """(step, mask, position) of every group of the walk in which exactly one line has the bit of some slot: mask R for the MS_IFK
    sites; for the MS_IFQ sites Q, and R0 = a lone R bit where no line of the group has the Q bit."""
    wn, lps = ll.wn, lps_of(ll.nwn)
    words = [reach_word(wn, lps, l.vnu, ll.mas(), False) for l in ll.lines]
    seen = set()
    for step, idx in walk_list(ll, profs, ms_items):
        if step is None:
            continue
        for k, _, _ in slots(wn):
            r = [(words[i] >> k) & 1 for i in idx]
            q = [(words[i] >> (8 + k)) & 1 for i in idx]
            if step in IFQ_STEPS:
                if sum(q) == 1:
                    seen.add((step, "Q", q.index(1)))
                if sum(q) == 0 and sum(r) == 1:
                    seen.add((step, "R0", r.index(1)))
            elif sum(r) == 1:
                seen.add((step, "R", r.index(1)))
    return seen
