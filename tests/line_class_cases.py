"""Constructed line lists for the class loops of the line sum, and a Python mirror of the rule that picks a line's class.

A line list here is written by hand: a line's place on the wavenumber axis decides its class against a channel set, so the class of
every line is known before any kernel runs.  tests/test_line_classes_cpu.py holds the mirror to the classes the cases claim and
counts what the cases reach; tests/test_line_classes.py runs them on the GPU.

The rule (monortm_amd/csrc/lines_device.hpp line_records; lines_kernel.hip / lines_ms_kernel.hip prepare stages), for a tile whose
channels run from lo to hi and a line with shifted centre X = vnu + pshift x RHORAT:
    window   a sorted molecule keeps the table lines with lo - 25 - pad <= vnu <= hi + 25 + pad, pad = max_abs_shift x max(RHORAT, 1)
             + 1e-6; an unsorted molecule and an O2 list with a coupled line keep every line; a zero column keeps none
    M2       lo + X <= 25   (never for CO2; always for a coupled O2 line)     negative resonance within reach of some channel
    TEST     |lo - X| > 25 or |hi - X| > 25  (never for a coupled O2 line)    the 25 cm-1 rule can fail for some channel
    FULL     single precision, two or four wavenumbers per lane: M2, not TEST, hi + X <= 25, no Voigt candidate, no Y factors
    Y        first-order coupled O2 (IFLG 1 / -1): the general loop, cuts the walk of the ordinary lines
    smoothing (one wavenumber per lane, and every single-precision tile), per 64 candidate lines counted from the slice's first:
             runs of untested lines shorter than 8 become tested, runs of one-resonance lines shorter than 8 become two-resonance,
             FULL runs (among the lines still untested) shorter than 8 lose FULL
    walk     lines_kernel<double>, one wavenumber per lane: the ordinary lines of a molecule between two cutters, within one 64-line
             group, in pairs from the first; a pair takes the step (TEST, M2) of the more general of its two lines; an odd last line
             and a run of one line take the single-line path
             every other tile: sub-runs of equal class within a group; double precision pairs them from the sub-run's first line
             lines_ms_kernel: no smoothing, the class is the union over the states of a wave, chunks of CL lines (test_ms_prepare_passes)
The thresholds themselves belong to the cut_boundaries fixtures: here every centre keeps MARGIN = 0.25 cm-1 from every boundary, in
every state and tile (the largest shift is below 0.01 cm-1), and every channel 0.5 cm-1 from every centre (the Voigt list apart).

Zones of line centres and their classes against channels from 0.5 to 40 cm-1 (one tile):
    TM 10.0 ..   tested, two resonances        UM 20.0 ..   untested, two resonances
    U1 24.9 ..   untested, one resonance       T1 32.0 ..   tested, one resonance        OUT 68.0 .., OUT2 67.0 ..  beyond 25 cm-1 of every channel
and against the sounder channels 0.3 - 6.5 cm-1: F1 10.0, F2 17.0 FULL; UM 20.0 two resonances, not FULL; TS 28.0 tested, one.
Lines of a zone sit 0.002 cm-1 apart.  A list is grouped by molecule in the file (H2O 1, CO2 2, O3 3, O2 7: the table's order); a
molecule whose zones do not ascend is an unsorted molecule to the table, which is how a class follows any other class.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from monortm_amd import synth, tape3

H2O, CO2, O3, O2 = 1, 2, 3, 7
KIND = {H2O: 0, O3: 0, O2: 1, CO2: 2}          # generic, O2, CO2 (eval_dispatch<KIND>)
KIND_NAME = ("generic", "O2", "CO2")
MARGIN = 0.25
NEAR = 0.5                                      # least distance channel - centre
STEP = 0.002
ZONE = {"TM": 10.0, "UM": 20.0, "U1": 24.9, "T1": 32.0, "OUT": 68.0, "OUT2": 67.0, "F1": 10.0, "F2": 17.0, "TS": 28.0}
ZONE_ORDER = ("TM", "F1", "F2", "UM", "U1", "TS", "T1", "OUT")
TOL_DBL = 1e-11
TOL_VOIGT = 1e-10
EPS_SGL = 2.0 ** -24
K_P0, K_T0 = 1013.25, 296.0
# log10 of the HITRAN strength: the upper part of synth.synthetic_lines' ranges (sized to standard_atmosphere's columns), 1.5 decades
S_LOG = {H2O: -25.8, CO2: -26.0, O3: -22.0, O2: -28.0}


# ---------------------------------------------------------------------------------------------------------------------------------
# line lists
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """mols: molecule -> zone names in table order ("UM*" = that line is first-order coupled: O2 only).  test_mol: the molecule whose
    column one profile of a batch sets to zero.  voigt: (molecule, index) of the line a channel is put beside."""
    name: str
    mols: dict
    test_mol: int
    about: str
    voigt: tuple | None = None
    sounder: bool = False          # zones are those of the sounder channel range
    tags: tuple = ()
    lines: list = field(default_factory=list, repr=False)   # (mol, zone, vnu, coupled) in file order

    def __post_init__(self):
        rng_off = {}
        self.lines = []
        for mol in sorted(self.mols):
            for z in self.mols[mol]:
                cpl = z.endswith("*")
                z = z.rstrip("*")
                k = rng_off.get((mol, z), 0)
                rng_off[(mol, z)] = k + 1
                assert k < 110, "a zone holds at most 110 lines of a molecule (U1 is 0.5 cm-1 wide less the margins)"
                self.lines.append((mol, z, ZONE[z] + STEP * k, cpl))

    def nlines(self, mol):
        return sum(1 for l in self.lines if l[0] == mol)

    def zones(self, mol):
        return [l[1] for l in self.lines if l[0] == mol]


def records(case: Case) -> tape3.LineRecords:
    """The TAPE3 records of a case: parameters from a generator seeded by the case's name, strengths within 1.5 decades, widths 0.03 -
    0.1, pressure shifts of 0.001 - 0.003 cm-1/atm of either sign."""
    rng = np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(case.name)))
    cols = {k: [] for k in ("vnu", "sp", "alfa", "epp", "mol", "hwhm", "tmpalf", "pshift", "iflg", "sdep")}
    for mol, _z, vnu, cpl in case.lines:
        s = 10.0 ** (S_LOG[mol] + 1.5 * rng.uniform())
        alfa, hwhm = rng.uniform(0.03, 0.1), rng.uniform(0.03, 0.1)
        if mol == O2:   # the air width must exceed 0.21 x self, so that the foreign width stays positive (lnfl_mod.f90:98-101)
            alfa, hwhm = rng.uniform(0.04, 0.06), rng.uniform(0.03, 0.06)
        shift = rng.uniform(0.001, 0.003) * (1.0 if rng.uniform() < 0.5 else -1.0)
        row = dict(vnu=vnu, sp=s / (vnu * (1.0 - np.exp(-synth.RADCN2 * vnu / 296.0))), alfa=alfa, epp=rng.uniform(0.0, 1500.0), mol=mol + 100,
                   hwhm=hwhm, tmpalf=rng.uniform(0.5, 0.8), pshift=shift, iflg=1 if cpl else 0, sdep=0.0)
        for k, v in row.items():
            cols[k].append(v)
        if cpl:      # the coupling record: Y, G at 200 / 250 / 296 / 340 K, as synth.synthetic_lines writes it
            assert mol == O2
            y = rng.uniform(0.1, 0.3) * np.array([1.3, 1.15, 1.0, 0.9])
            g = rng.uniform(0.005, 0.02) * np.array([1.5, 1.2, 1.0, 0.8])
            row = dict(vnu=y[0], sp=g[0], alfa=y[1], epp=g[1], mol=int(np.float32(y[2]).view(np.int32)), hwhm=g[2], tmpalf=y[3], pshift=g[3],
                       iflg=-1, sdep=0.0)
            for k, v in row.items():
                cols[k].append(v)
    rec = tape3.LineRecords(**{k: np.asarray(v) for k, v in cols.items()})
    assert len(rec) <= tape3.NLINEREC, "one block: the reader's block rules stay out of the way"
    return rec


def single_line_cases(case: Case):
    """One case per physical line of `case`: the same record alone in the file (the additivity of the reference)."""
    rec = records(case)
    phys = np.flatnonzero(rec.iflg >= 0)
    out = []
    for i in phys:
        sel = [i, i + 1] if rec.iflg[i] == 1 else [i]
        out.append(tape3.LineRecords(**{k: np.asarray(getattr(rec, k))[sel] for k in
                                        ("vnu", "sp", "alfa", "epp", "mol", "hwhm", "tmpalf", "pshift", "iflg", "sdep")}))
    return out


def _rep(z, n):
    return [z] * n


def _debruijn():
    """17 classes holding every ordered pair of the four once (an Eulerian circuit of the complete digraph with loops)."""
    seq = ["TM", "TM", "UM", "UM", "U1", "U1", "T1", "T1", "TM", "U1", "TM", "T1", "UM", "T1", "U1", "UM", "TM"]
    pairs = set(zip(seq[:-1], seq[1:]))
    assert len(seq) == 17 and len(pairs) == 16
    return seq


def _blocks(order):
    """A class sequence that survives the smoothing of the one-wavenumber tiles: every untested line inside eight untested ones in
    a row, every one-resonance line inside eight one-resonance ones."""
    out = []
    for z in order:
        out += _rep(z, 8 if z != "TM" else 1)
    return out


RUN_LENGTHS = (1, 2, 3, 4, 5, 8, 9)
CUT_AT = {"first": 0, "second": 1, "third": 2, "middle": 4, "last_but_one": 7, "last": 8}    # of an O2 run of nine


def _cases():
    c = []
    gen = ("TM", "UM", "U1", "T1")
    # ---- runs of one class: CO2, O3 and O2 each hold n lines of one zone (for CO2 the zone says tested / untested alone)
    for n in RUN_LENGTHS:
        for z in gen:
            c.append(Case(f"run_{z}_{n}", {CO2: _rep(z, n), O3: _rep(z, n), O2: _rep(z, n)}, O3, f"CO2, O3, O2: {n} x {z} each", tags=("run",)))
    # ... and behind twelve H2O lines of their own class: the short runs keep that class through the smoothing of the one-wavenumber tiles
    for n in (1, 2, 3, 5):
        for z in ("UM", "U1", "T1"):
            c.append(Case(f"island_{z}_{n}", {H2O: _rep(z, 12), CO2: _rep(z, n), O3: _rep(z, n), O2: _rep(z, n)}, O3,
                          f"12 H2O lines of {z}, then CO2, O3, O2: {n} x {z} each", tags=("island",)))
    # ---- every ordered pair of classes, once as is and once with a line in front (the other alignment to the pairs)
    db = _debruijn()
    for mol, nm in ((O3, "gen"), (O2, "o2")):
        c.append(Case(f"pairs_{nm}", {mol: db}, mol, "17 lines: all 16 ordered class pairs", tags=("pairs",)))
        c.append(Case(f"pairs_{nm}_shift", {mol: ["TM"] + db}, mol, "the same behind one more line", tags=("pairs",)))
    # the same transitions in blocks that the smoothing leaves alone (<= 64 lines each: one group)
    blk = {"a": ("TM", "U1", "TM", "T1", "TM", "UM", "TM"), "b": ("UM", "T1", "UM", "U1", "UM"), "c": ("T1", "U1", "T1", "UM", "U1")}
    for k, order in blk.items():
        for mol, nm in ((O3, "gen"), (O2, "o2")):
            c.append(Case(f"blocks_{nm}_{k}", {mol: _blocks(order)}, mol, "class changes between blocks of eight: " + " ".join(order), tags=("blocks",)))
            c.append(Case(f"blocks_{nm}_{k}_shift", {mol: ["TM"] + _blocks(order)}, mol, "the same behind one more line", tags=("blocks",)))
    c.append(Case("co2_mix", {CO2: ["TM", "UM", "TM", "TM", "UM", "UM", "UM", "TM", "UM"]}, CO2, "CO2 tested / untested in every order", tags=("pairs", "co2")))
    c.append(Case("co2_blocks", {CO2: ["TM"] + _rep("UM", 8) + ["TM", "TM"] + _rep("UM", 9) + ["TM"]}, CO2, "CO2 blocks that survive the smoothing", tags=("blocks", "co2")))
    c.append(Case("co2_blocks_shift", {CO2: ["TM", "TM"] + _rep("UM", 8) + ["TM", "TM"] + _rep("UM", 9) + ["TM"]}, CO2, "the same behind one more line", tags=("blocks", "co2")))
    # ---- 64-line groups: the O3 run starts at bit 0, 1, 62, 63 (H2O lines in front), and runs over two and three groups
    mix5 = ["TM", "UM", "UM", "U1", "T1"]
    for off in (0, 1, 62, 63):
        c.append(Case(f"group_bit{off}", {H2O: (_rep("UM", off)), O3: mix5, O2: mix5}, O3, f"{off} H2O lines, then five O3 lines from bit {off}", tags=("group",)))
    c.append(Case("group_two", {H2O: _rep("UM", 50), O3: _rep("TM", 10) + _rep("UM", 20) + _rep("U1", 12) + _rep("T1", 8)}, O3,
                  "O3 run of 50 lines over bits 50 .. 99: two groups", tags=("group", "span2")))
    long3 = _rep("TM", 20) + _rep("UM", 45) + _rep("U1", 30) + _rep("T1", 35)
    c.append(Case("group_three", {H2O: _rep("UM", 3), O3: long3}, O3, "O3 run of 130 lines over bits 3 .. 132: three groups", tags=("group", "span3", "slice")))
    c.append(Case("group_three_o2", {H2O: _rep("UM", 60), O2: _rep("TM", 10) + _rep("UM", 30) + _rep("U1", 20) + _rep("T1", 10)}, O2,
                  "O2 run of 70 lines over bits 60 .. 129: three groups", tags=("group", "span3")))
    # ---- cutters: one first-order coupled O2 line in an O2 run of nine
    for k, pos in CUT_AT.items():
        z = ["TM", "TM", "UM", "UM", "UM", "UM", "U1", "T1", "T1"]
        z[pos] = z[pos] + "*"
        c.append(Case(f"cut_{k}", {O2: z}, O2, f"coupled O2 line at position {pos} of nine", tags=("cut",)))
    # ---- a Voigt candidate among ordinary lines: the 0.05 hPa layer, a channel 0.0005 cm-1 from the one UM line
    c.append(Case("voigt", {O3: ["TM", "TM", "UM", "U1", "U1", "T1", "T1"]}, O3, "one generic list, a channel beside line 2 (alone in its zone)", voigt=(O3, 2), tags=("voigt",)))
    # ---- the lumped pedestal of the two-wavenumber double tile (eval_fast2: untested one-resonance generic sub-runs of >= 16 lines)
    c.append(Case("lump_15", {O3: _rep("U1", 15)}, O3, "15 untested one-resonance lines: one short of the lumped pedestal", tags=("lump",)))
    c.append(Case("lump_16", {O3: _rep("U1", 16)}, O3, "16 untested one-resonance lines: the lumped pedestal", tags=("lump",)))
    # ---- nothing within 25 cm-1: sorted (the window drops the lines), unsorted (they are walked and add exactly nothing)
    c.append(Case("out_of_reach", {CO2: _rep("OUT", 3), O3: _rep("OUT", 3), O2: _rep("OUT", 2)}, O3,
                  "every line beyond 25 cm-1 of every channel, sorted: the window drops them, rows of zeros", tags=("zero",)))
    c.append(Case("out_of_reach_walked", {CO2: ["OUT", "OUT2", "OUT"], O3: ["OUT", "OUT2", "OUT", "OUT"], O2: ["OUT", "OUT2"]}, O3,
                  "the same unsorted: the lines are walked as tested lines and add exactly nothing", tags=("zero",)))
    # ---- single precision, sounder channels: FULL lines (F1, F2), two-resonance lines that are not FULL (UM), tested lines (TS)
    full = _rep("F1", 5) + _rep("F2", 6) + _rep("UM", 9) + _rep("TS", 3)
    c.append(Case("full_sorted", {O3: full}, O3, "FULL, M2 not FULL, tested: in zone order", sounder=True, tags=("full",)))
    c.append(Case("full_o2", {O2: full}, O2, "the same for O2", sounder=True, tags=("full",)))
    c.append(Case("full_mixed", {O3: _rep("F1", 9) + ["UM"] + _rep("F2", 8) + _rep("UM", 8) + ["F1", "TS"] + _rep("F2", 3)}, O3,
                  "FULL runs of 9 and 8 around lines above 18.5 cm-1, short FULL runs that the smoothing returns to M2", sounder=True, tags=("full",)))
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return {x.name: x for x in c}


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------------------------
# channels and states
# ---------------------------------------------------------------------------------------------------------------------------------
# channels keep NEAR from every zone's lines and tile ends keep MARGIN from every class boundary of every zone
_KEEP_OUT = [(4.6, 5.4), (6.6, 7.4), (9.4, 10.8), (14.6, 15.4), (19.4, 20.8), (24.3, 25.7), (31.4, 32.8), (34.6, 35.4), (39.6, 39.95)]


def wide_channels(n: int) -> np.ndarray:
    """n channels from 0.5 to 40 cm-1, both ends included, none inside a keep-out interval."""
    if n == 1:
        return np.array([12.0])
    if n == 2:
        return np.array([0.5, 40.0])
    grid = np.linspace(0.5, 40.0, 40 * n + 1)
    ok = np.ones(len(grid), bool)
    for a, b in _KEEP_OUT:
        ok &= ~((grid > a) & (grid < b))
    grid = grid[ok]
    idx = np.unique(np.round(np.linspace(0, len(grid) - 1, n)).astype(int))
    assert len(idx) == n
    return grid[idx]


def sounder_channels(n: int) -> np.ndarray:
    """n channels from 0.3 to 6.5 cm-1 (no centre below 10 cm-1: nothing to keep out of)."""
    return np.linspace(0.3, 6.5, n)


def voigt_channels(case: Case, n: int) -> np.ndarray:
    mol, k = case.voigt
    vnu = [l[2] for l in case.lines if l[0] == mol][k]
    wn = wide_channels(n)
    j = int(np.argmin(np.abs(wn - vnu)))
    wn[j] = vnu + 0.0005
    assert np.all(np.diff(wn) > 0)
    return wn


LAYER_P = np.array([1000.0, 500.0, 150.0, 0.05])
LAYER_T = np.array([290.0, 255.0, 217.0, 250.0])
LAYER_TZ = np.array([295.0, 272.0, 236.0, 220.0, 262.0])
LAYER_DP = np.array([100.0, 100.0, 50.0, 0.02])
VMR = np.array([[1.0e-2, 4e-4, 5e-8, 3.2e-7, 1.5e-7, 1.7e-6, 0.209],
                [2.0e-3, 4e-4, 1e-7, 3.2e-7, 1.5e-7, 1.7e-6, 0.209],
                [6.0e-6, 4e-4, 8e-7, 3.0e-7, 1.0e-7, 1.6e-6, 0.209],
                [5.0e-6, 4e-4, 2e-6, 1.0e-8, 1.0e-7, 2.0e-7, 0.209]])


def base_profile(wn, fp=1.0, dt=0.0, fc=1.0, zero_mol=None, nlay=4) -> synth.Profile:
    air = 2.1e25 * LAYER_DP[:nlay] / 1013.0 * fc
    wkl = VMR[:nlay] * air[:, None]
    if zero_mol:
        wkl[:, zero_mol - 1] = 0.0
    return synth.Profile(wn=np.asarray(wn, float), p=LAYER_P[:nlay] * fp, t=LAYER_T[:nlay] + dt, tz=LAYER_TZ[:nlay + 1] + dt, wkl=wkl, wbrodl=0.781 * air,
                         clw=np.zeros(nlay), irt=3)


def batch7(wn, zero_mol) -> list:
    """Seven profiles with different T, P and columns; profile 3 has no column of `zero_mol`."""
    fc = (1.0, 0.6, 1.7, 1.0, 0.8, 1.3, 2.0)
    return [base_profile(wn, fp=1.0 + 0.012 * (i - 3), dt=2.5 * (i - 3), fc=fc[i], zero_mol=zero_mol if i == 3 else None) for i in range(7)]


def big_batch(wn, nprof=128, nlay=64) -> list:
    """The batch of the four-wavenumber float tile: copies of one 64-layer profile with small perturbations of p and t."""
    a = synth.standard_atmosphere(nlay, ztop_km=30)
    return [synth.Profile(wn=np.asarray(wn, float), p=a["p"] * (1.0 + 0.001 * (i % 17)), t=a["t"] + 0.01 * i, tz=a["tz"] + 0.01 * i, wkl=a["wkl"], wbrodl=a["wbrodl"],
                          clw=a["clw"], irt=3) for i in range(nprof)]


def rhorat(p, t):
    return (np.asarray(p) / np.asarray(t)) / (K_P0 / K_T0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the mirror
# ---------------------------------------------------------------------------------------------------------------------------------
def _open8(bits):
    """Runs of True shorter than 8 become False (open_runs8 on a list of at most 64 booleans)."""
    out, i, n = [False] * len(bits), 0, len(bits)
    while i < n:
        if bits[i]:
            j = i
            while j < n and bits[j]:
                j += 1
            if j - i >= 8:
                out[i:j] = [True] * (j - i)
            i = j
        else:
            i += 1
    return out


def _open8_word(x: int) -> int:
    """open_runs8 as the device writes it, on a 64-bit word."""
    m = (1 << 64) - 1
    e = x & (x >> 1)
    e &= e >> 2
    e &= e >> 4
    e |= (e << 1) & m
    e |= (e << 2) & m
    e |= (e << 4) & m
    return e


@dataclass
class TableLine:
    mol: int
    zone: str
    vnu: float
    pshift: float
    coupled: bool
    index: int       # position among the molecule's lines in the table


def table(case: Case):
    """The device's line table of a case: per molecule (ascending number) its lines in file order, with the pressure shift as
    stored (REAL*4), whether the molecule is sorted, and max_abs_shift (line_table.cpp)."""
    rec = records(case)
    phys = np.flatnonzero(rec.iflg >= 0)
    assert len(phys) == len(case.lines)
    by_mol, k = {}, {}
    for i, (mol, z, vnu, cpl) in zip(phys, case.lines):
        assert int(rec.mol[i]) % 100 == mol and rec.vnu[i] == vnu
        by_mol.setdefault(mol, []).append(TableLine(mol, z, vnu, float(rec.pshift[i]), cpl, k.get(mol, 0)))
        k[mol] = k.get(mol, 0) + 1
    is_sorted = {m: all(a.vnu <= b.vnu for a, b in zip(ls[:-1], ls[1:])) for m, ls in by_mol.items()}
    mas = max(2.0 * abs(float(p)) for p in rec.pshift[phys])
    return by_mol, is_sorted, mas


def _dist(x, bounds):
    return min(abs(x - b) for b in bounds)


def classify(case: Case, lo: float, hi: float, states, full_boundary: bool = False):
    """The candidate lines of a tile [lo, hi] and their raw classes, the same in every state (p, t, columns present) of `states` - a list of
    (p, t, set of molecules with a column).  Returns a list of dicts in walk order (molecule, then table order) with keys mol, zone,
    index, test, m2, y, full.  Asserts the margins."""
    by_mol, is_sorted, mas = table(case)
    rmax = max(float(rhorat(p, t)) for p, t, _ in states)
    assert mas * rmax < 0.01, f"{case.name}: a shift of {mas * rmax:.4f} cm-1"
    out = []
    for mol in sorted(by_mol):
        ls = by_mol[mol]
        if not any(mol in have for _, _, have in states):
            continue
        windowed = is_sorted[mol] and not (mol == O2 and any(l.coupled for l in ls))
        for l in ls:
            if windowed:
                ends = (lo - 25.0, hi + 25.0)
                assert _dist(l.vnu, ends) >= MARGIN, f"{case.name}: line {l.vnu} within {MARGIN} of the window {ends}"
                if not (ends[0] <= l.vnu <= ends[1]):
                    continue
            cls = set()
            for p, t, _have in states:
                x = l.vnu + l.pshift * float(rhorat(p, t))
                cut = np.inf if (mol == O2 and l.coupled) else 25.0
                m2 = mol != CO2 and lo + x <= cut
                al = not (abs(lo - x) > cut) and not (abs(hi - x) > cut)
                full = m2 and al and not l.coupled and hi + x <= 25.0
                if cut == 25.0:
                    bounds = [lo - 25.0, lo + 25.0, hi - 25.0, hi + 25.0] + ([25.0 - lo] if mol != CO2 else []) + ([25.0 - hi] if full_boundary and mol != CO2 else [])
                    assert _dist(x, bounds) >= MARGIN - 0.01, f"{case.name}: centre {x} within {MARGIN} of a class boundary of the tile [{lo}, {hi}]"
                cls.add((not al, m2, full))
            assert len(cls) == 1, f"{case.name}: line {l.vnu} changes class between the states"
            test, m2, full = cls.pop()
            out.append(dict(mol=mol, zone=l.zone, index=l.index, vnu=l.vnu, test=test, m2=m2, y=bool(l.coupled), full=full))
    return out


def claimed(zone: str, mol: int, lo: float, hi: float, coupled: bool = False):
    """(TEST, M2) of a zone's lines by the table of the module docstring, from the zone's nominal position alone."""
    if coupled:
        return (False, True)
    x = ZONE[zone]
    return (not (hi - 25.0 <= x <= lo + 25.0), mol != CO2 and x <= 25.0 - lo)


DOP = 3.5812e-7      # HWHM_D / Xnu = DOP sqrt(T / M): sqrt(2 ln 2 k / (amu c^2))
MASS = {H2O: 18.0, CO2: 44.0, O3: 48.0, O2: 32.0}


def check_channels(case: Case, wn):
    """Every channel keeps NEAR from every centre, which is far beyond 100 Doppler widths of any line here in any layer: no Voigt
    candidate (modm.f90:427), the 0.05 hPa layer included.  The Voigt list: its chosen line, and that line alone, has a channel within 50
    Doppler widths in the 0.05 hPa layer, where its zeta = HW / (HW + HWD) is below 0.9; in the three dense layers zeta > 0.99."""
    cen = np.array([l[2] for l in case.lines])
    d = np.abs(np.asarray(wn)[:, None] - cen[None, :])
    hwd_max = DOP * np.sqrt(300.0 / 18.0) * 70.0
    assert 100.0 * hwd_max < 0.02 < NEAR
    if case.voigt:
        mol, k = case.voigt
        j = [i for i, l in enumerate(case.lines) if l[0] == mol][k]
        for p, t in zip(LAYER_P, LAYER_T):
            hwd = DOP * np.sqrt((t + 8.0) / MASS[mol]) * cen[j]
            hw_lo, hw_hi = 0.03 * float(rhorat(p * 0.96, t + 8.0)) * (K_T0 / (t + 8.0)) ** 0.5, 0.1 * float(rhorat(p * 1.04, t - 8.0)) * (K_T0 / (t - 8.0)) ** 0.8
            if p < 1.0:
                assert hw_hi / (hw_hi + hwd * 0.95) < 0.9 and d[:, j].min() < 50.0 * hwd * 0.95
            else:
                assert hw_lo / (hw_lo + hwd) > 0.99
        d = np.delete(d, j, axis=1)
    assert d.size == 0 or d.min() >= NEAR - 0.01, f"{case.name}: a channel {d.min():.3f} cm-1 from a centre"


def no_far_field(lines, lo, hi, nw, wpl):
    """lines_kernel moves lines into a tile's far-field sums only in tiles of two waves or more, when 2 x far + half-far lines among 64
    reach 32.  A far line is untested, has no or a FULL negative resonance, and lies at least kappa tile half-widths from the tile's
    centre (2.25; 1.2 for the four-wave tile, which alone has half-far lines: untested, FULL): fewer than 16 candidates rule it out.
    (far_kernel serves dense grids of >= 4 tiles with ~1000 lines each: never these lists.)"""
    w0, rr = 0.5 * (lo + hi), 0.5 * (hi - lo)
    if nw < 2 or wpl < 2 or rr == 0.0:
        return True
    kappa = 1.2 if nw * wpl >= 8 else 2.25
    far = sum(1 for l in lines if not l["test"] and not l["y"] and (not l["m2"] or l["full"]) and abs(l["vnu"] - w0) >= kappa * rr - 0.01)
    half = sum(1 for l in lines if nw * wpl >= 8 and not l["test"] and l["full"])
    return far + half < 16


def effective(lines, family: str, vbeg: int = 0, vend: int | None = None, group: int = 64):
    """The classes after the smoothing of the prepare stage, for the candidates [vbeg, vend) of one slice.  family: 'asm' (double, one
    wavenumber per lane), 'sgl1' / 'sgl2' (single precision, one / two or four wavenumbers per lane), 'dbl2' (double, two
    wavenumbers per lane: no smoothing), 'ms' (lines_ms_kernel: no smoothing; group = CL).  Returns the slice's lines with keys
    etest, em2, efull added, and `bit` = the line's place in its group."""
    vend = len(lines) if vend is None else vend
    out = []
    smooth = family in ("asm", "sgl1", "sgl2")
    for g0 in range(vbeg, vend, group):
        grp = [dict(l) for l in lines[g0:min(g0 + group, vend)]]
        al = [not l["test"] for l in grp]
        m2 = [l["m2"] for l in grp]
        if smooth:
            ca = _open8(al)
            cm = [not b for b in _open8([not b for b in m2] + [True] * (64 - len(grp)))[:len(grp)]]
            # (lanes past the last line hold no two-resonance bit: a gap at the end of the list runs on into them)
            word = sum(1 << i for i, b in enumerate(al) if b)
            assert [bool((_open8_word(word) >> i) & 1) for i in range(len(grp))] == ca
        else:
            ca, cm = al, m2
        fu = [False] * len(grp)
        if family == "sgl2":
            fu = _open8([l["full"] and a and l["mol"] != CO2 for l, a in zip(grp, ca)])
        for i, l in enumerate(grp):
            l["etest"], l["em2"], l["efull"], l["bit"] = not ca[i], bool(cm[i]) and l["mol"] != CO2, fu[i], i
            if smooth:   # a line only ever takes a more general loop
                assert (l["etest"] or not l["test"]) and (l["em2"] or not l["m2"])
        out += grp
    return out


def walk(eff, family: str):
    """The steps that evaluate the lines of effective(): a list of (line, step) with step = dict(kind, test, m2, full, pos) and pos one
    of 'first', 'second' (of a pair), 'tail' (odd last line of a run of >= 3), 'single' (a run of one), 'cutter'.  The position is
    arithmetic only where the loops pair lines: generic molecules and O2 in double precision (asm_run, eval_pair, lines_ms_asm), and
    the two lines per trip of the two-wavenumber loops.  CO2 everywhere and the float one-wavenumber loops take one line at a time:
    there the position says no more than where in its run a line sits, and the census does not ask for it.  Runs: a molecule's
    lines within one group, between cutters; 'asm' pairs them whatever their classes and the pair takes the more general step; the
    other families cut at every change of class as well and (double precision) pair within the sub-run."""
    out, i, n = [], 0, len(eff)
    while i < n:
        l = eff[i]
        if l["y"]:
            out.append((l, dict(kind=KIND[l["mol"]], test=False, m2=True, full=False, pos="cutter")))
            i += 1
            continue
        j = i
        key = (lambda q: (q["etest"], q["em2"], q["efull"])) if family != "asm" else (lambda q: None)
        while j < n and eff[j]["mol"] == l["mol"] and not eff[j]["y"] and (j == i or eff[j]["bit"] != 0) and key(eff[j]) == key(l):
            j += 1
        run = eff[i:j]
        for k in range(0, len(run) - 1, 2):
            a, b = run[k], run[k + 1]
            st = dict(kind=KIND[a["mol"]], test=a["etest"] or b["etest"], m2=a["em2"] or b["em2"], full=a["efull"])
            out.append((a, dict(st, pos="first")))
            out.append((b, dict(st, pos="second")))
        if len(run) % 2:
            a = run[-1]
            out.append((a, dict(kind=KIND[a["mol"]], test=a["etest"], m2=a["em2"], full=a["efull"], pos="single" if len(run) == 1 else "tail")))
        i = j
    return out


def ms_layout(nwn, nprof, nslot, ms_items=192):
    """modm_plan.hpp's choice for lines_ms_kernel, (G, CL): the restatement of tests/test_ms_prepare_passes.py."""
    from test_ms_prepare_passes import _layout

    got = _layout(nwn, nprof, ms_items, nslot)
    return None if got is None else got[:2]


def tiles(wn, tw):
    wn = np.asarray(wn)
    return [(float(wn[i]), float(wn[min(i + tw, len(wn)) - 1])) for i in range(0, len(wn), tw)]


def states_of(profiles):
    out = []
    for pr in profiles:
        for k in range(pr.nlay):
            out.append((float(pr.p[k]), float(pr.t[k]), frozenset(m + 1 for m in range(pr.nmol) if pr.wkl[k, m] != 0.0)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the measure
# ---------------------------------------------------------------------------------------------------------------------------------
def row_errors(got, exp):
    """E per (layer, molecule) = max over channels |got - exp| / max over channels |exp|; a row of zeros must be zeros: E = 0 then,
    inf otherwise."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    pk = np.abs(exp).max(axis=-1)
    d = np.abs(got - exp).max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(pk > 0, d / np.where(pk > 0, pk, 1.0), np.where(d == 0, 0.0, np.inf))
    return e


def sgl_bound(nlines: int) -> float:
    """(k + 16) x 2^-24 for a molecule of k lines: about sixteen float roundings in a two-resonance term, one more per line added."""
    return (nlines + 16) * EPS_SGL


# ---------------------------------------------------------------------------------------------------------------------------------
# the configurations the GPU module forces, and what each walks
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Config:
    """One forced configuration.  family: the mirror's walk; kind: real_kind; options: set_option pairs; nwn: channel counts; nw, wpl:
    waves per workgroup and wavenumbers per lane of the tile (lines_config / tile_waves); batch: seven profiles instead of one."""
    name: str
    family: str
    kind: int
    options: tuple
    nwn: tuple
    nw: int = 1
    wpl: int = 1
    batch: bool = False
    sounder: bool = False
    nslice: int = 1
    only: tuple = ()         # tags of the cases it runs (empty: every case of its channel range)


CONFIGS = {c.name: c for c in (
    Config("wn", "asm", 8, (("lines_kernel", "wn"), ("nslice", 1)), (1, 37, 64)),
    Config("ms", "ms", 8, (("lines_kernel", "ms"),), (5, 50, 64), batch=True),
    Config("dbl2", "dbl2", 8, (("nslice", 1),), (65, 128, 129, 256), wpl=2),
    Config("dbl2_tw1", "dbl2", 8, (("nslice", 1), ("tile_waves", 1)), (513,), nw=1, wpl=2),
    Config("dbl2_tw2", "dbl2", 8, (("nslice", 1), ("tile_waves", 2)), (513,), nw=2, wpl=2),
    Config("dbl2_tw4", "dbl2", 8, (("nslice", 1), ("tile_waves", 4)), (513,), nw=4, wpl=2),
    Config("sgl1", "sgl1", 4, (("nslice", 1),), (64,)),
    Config("sgl2", "sgl2", 4, (("nslice", 1),), (128, 200), wpl=2),
    Config("sgl2_sounder", "sgl2", 4, (("nslice", 1),), (128, 200), wpl=2, sounder=True),
    Config("slice3", "asm", 8, (("lines_kernel", "wn"), ("nslice", 3)), (37,), batch=True, nslice=3, only=("group",)),
)}
# the four-wavenumber float tile (nw = 1, wpl = 4 of lines_config): 200 sounder channels, 128 profiles x 64 layers = 8192 states
SGL4 = Config("sgl4_sounder", "sgl2", 4, (), (200,), wpl=4, sounder=True)


def cases_of(cfg: Config):
    out = []
    for c in CASES.values():
        if c.sounder != cfg.sounder or (cfg.only and not set(cfg.only) & set(c.tags)):
            continue
        if c.voigt and cfg.kind == 4:
            continue      # (single precision corrects no Voigt candidate afterwards: it walks the general loop, out of scope here)
        out.append(c)
    return out


def channels(case: Case, cfg: Config, nwn: int) -> np.ndarray:
    if cfg.sounder:
        return sounder_channels(nwn)
    return voigt_channels(case, nwn) if case.voigt else wide_channels(nwn)


def profiles(case: Case, cfg: Config, wn) -> list:
    return batch7(wn, case.test_mol) if cfg.batch else [base_profile(wn)]


def mirror(case: Case, cfg: Config, nwn: int, profs=None):
    """What `cfg` walks for `case` with nwn channels: per tile and slice the list walk() returns.  Asserts the margins, the channel
    distances and that no line can leave for a far field."""
    wn = channels(case, cfg, nwn)
    check_channels(case, wn)
    profs = profiles(case, cfg, wn) if profs is None else profs
    st = states_of(profs)
    if cfg.family == "ms":
        tl, group = [(float(wn[0]), float(wn[-1]))], None
    else:
        tl, group = tiles(wn, 64 * cfg.nw * cfg.wpl), 64
    out = []
    for lo, hi in tl:
        lines = classify(case, lo, hi, st, full_boundary=cfg.family == "sgl2")
        assert no_far_field(lines, lo, hi, cfg.nw, cfg.wpl), f"{case.name}: far-field candidates in the tile [{lo}, {hi}]"
        if cfg.family == "ms":
            nslot = len({m for m in case.mols})
            g = ms_layout(nwn, len(profs), nslot)
            assert g is not None
            group = g[1]
        n = len(lines)
        for s in range(cfg.nslice):
            vbeg, vend = (n * s) // cfg.nslice, (n * (s + 1)) // cfg.nslice
            eff = effective(lines, cfg.family, vbeg, vend, group)
            if cfg.family == "ms":     # O2 and CO2 take the tested forms there whatever the class
                for l in eff:
                    l["etest"] = l["etest"] or KIND[l["mol"]] != 0
            out.append(dict(tile=(lo, hi), slice=s, vbeg=vbeg, steps=walk(eff, cfg.family)))
    return out
