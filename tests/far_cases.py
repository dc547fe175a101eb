"""Cases for far_kernel (monortm_amd/csrc/far_kernel.hip) and a host mirror of the choices that decide what it runs.

The launcher gives a level of intervals 1, 2, 4 or 8 waves per workgroup (NWF) from
    steps = lines of the table per cm-1 x width of the level / molecules with lines / 128      (16, 32, 128 are the thresholds).
The random lists of the other far-field tests hold <= 4000 lines spread over five molecules: steps ~ 4, NWF = 1 everywhere.  Here the
lists are dense and hold one molecule (or one dense molecule and a few lines of a second), as a real line file does where one species
dominates: the launcher then takes the other variants by itself - no test sets MONORTM_FAR_WAVES.

Every case declares the NWF of each of its launches (`expect`).  plan() restates, in integer and double arithmetic, what the host does
with a case - the blocks of the line file it keeps, lines_config, the tile choice and the level count of modm_plan.hpp, the steps -> NWF rule
of launch_far - and geometry() what far_plan_kernel finds for one (interval, molecule, layer state): the Voigt guard, the seven FarGeom
indices, inheritance, the runs of far_kernel and the runs left to the tile.  census() walks the steps of far_kernel with them (which
lines a step holds, one or two resonances, its order from far_order restated in float32, the sign of A in far_slot_of).
tests/test_modm_plan_cpu.py holds plan() to modm_plan.hpp itself (host code, no GPU); tests/test_far_cpu.py asserts that the declared variants follow from the mirror with a margin and that the cases reach the branches
they were built for; tests/test_far_kernel.py reads the variants back from the launch counters and compares with the oracle.

Lists: molecule subsets of synth.synthetic_lines(80000, seed, vhi = just above the last wavenumber + 25), thinned to a line count.
Layers: picked from the 64 layers of synth.standard_atmosphere() - 0 is the surface layer (widest lines), 63 the top one (1.4 hPa, the
tightest Voigt guard).

Compared stretches (stretches()): whole tiles where tiles hold 128 wavenumbers; of wider tiles the 128 wavenumbers at each end that is
asked for (the oracle takes ~1.5 s per 10^7 line x wavenumber x layer evaluations, and a case has to stay at a few seconds; the
comparison with the in-kernel far field covers every wavenumber).
"""
from __future__ import annotations

import dataclasses
import functools
import types

import numpy as np

from monortm_amd import synth
from monortm_amd.tape3 import NLINEREC, LineRecords

H2O, CO2, O3, O2 = 1, 2, 3, 7
NMOL = 7
FAR_P, FAR_PREG, FAR_KAPPA, FAR_MAXLEV = 56, 32, 1.2, 6      # device_common.hpp, far_kernel.hip, lines_device.hpp
FAR_MOM_STRIDE, FAR_GEOM_INTS, FAR_SEG_INTS = FAR_P + 2, 8, 10
THRESHOLDS = (16.0, 32.0, 128.0)                             # launch_far: steps <= 16 -> 1, <= 32 -> 2, <= 128 -> 4, else 8
MARGIN = 0.10                                                # every level's steps stay this far (relative) from every threshold
NWF = (1, 2, 4, 8)
FAR_CAP, PHYS_CAP = 1 << 30, 2 << 30                         # api.hip (Ctx): the least workspace caps of a context
K_BOLTZ, K_AVOGAD, K_CLIGHT, K_T0, K_P0 = 1.3806503e-16, 6.02214199e23, 2.99792458e10, 296.0, 1013.25
# lightest isotopologue (the widest Doppler line) of the molecules that hold lines here, g / mol (TIPS / molec_mass of the reference);
# the guard's two sides are asserted 5 % apart wherever the mirror decides with them
LIGHTEST = {H2O: 18.010565, CO2: 43.989830, O3: 47.984745, 4: 44.001062, O2: 31.989830}
TOL_ORACLE, TOL_INKERNEL, FLOOR_MAX = 1e-10, 1e-11, 1e-11    # the far-field bounds of tests/test_hip_parity.py; the oracle's additivity
MAX_POINTS = 128                                             # wavenumbers compared at each end of a tile that is wider


def _subset(rec: LineRecords, sel) -> LineRecords:
    return LineRecords(**{k: getattr(rec, k)[sel] for k in ("vnu", "sp", "alfa", "epp", "mol", "hwhm", "tmpalf", "pshift", "iflg",
                                                             "brd_flg", "brd_dat", "sdep")})


@functools.lru_cache(maxsize=None)
def _base(seed: int, vhi: float) -> LineRecords:
    return synth.synthetic_lines(80000, seed=seed, vlo=0.05, vhi=vhi)


def molecule_lines(mol: int, n: int, seed: int, vhi: float, window=None) -> LineRecords:
    """n lines of one molecule: its records in the 80000-line list of `seed` (inside `window` = (lo, hi) cm-1 if given), thinned evenly."""
    rec = _base(seed, vhi)
    idx = np.flatnonzero(rec.mol % 100 == mol)
    if window is not None:
        idx = idx[(rec.vnu[idx] >= window[0]) & (rec.vnu[idx] <= window[1])]
    assert len(idx) >= n, f"molecule {mol}: {len(idx)} lines there, {n} wanted"
    return _subset(rec, idx[np.unique(np.round(np.linspace(0, len(idx) - 1, n)).astype(np.int64))])


def merged(*recs: LineRecords) -> LineRecords:
    keys = ("vnu", "sp", "alfa", "epp", "mol", "hwhm", "tmpalf", "pshift", "iflg", "brd_flg", "brd_dat", "sdep")
    cat = LineRecords(**{k: np.concatenate([getattr(r, k) for r in recs]) for k in keys})
    return _subset(cat, np.argsort(cat.vnu, kind="stable"))


@dataclasses.dataclass(frozen=True)
class Part:
    mol: int
    n: int
    seed: int
    window: tuple | None = None


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    parts: tuple            # of Part
    v1: float
    dv: float
    nwn: int
    expect: tuple           # NWF of every far_kernel launch of one call, sorted (one launch per level)
    layers: tuple = ((0, 63),)      # per profile: layers of the 64-layer standard atmosphere
    tile_waves: object = "auto"
    far_levels: int | None = None   # set_option("far_levels", ...) where the level count is forced (None: chosen by the call)
    zero: tuple = ()        # (profile, position in its layers, molecule): column amounts set to zero
    nslice: int = 0         # > 0: the case is also run with this many line slices
    single: bool = False    # also run with real_kind = 4
    tags: tuple = ()
    focus: int | None = None   # the molecule the tags speak about

    @property
    def wn(self) -> np.ndarray:
        return self.v1 + self.dv * np.arange(self.nwn)

    @property
    def vhi(self) -> float:
        """Upper end of the list: the file's blocks are kept up to the first that ends beyond the last wavenumber + 25."""
        return float(np.ceil(self.v1 + self.dv * (self.nwn - 1) + 25.0)) + 1.0


@functools.lru_cache(maxsize=None)
def records(case: Case) -> LineRecords:
    recs = [molecule_lines(p.mol, p.n, p.seed, case.vhi, p.window) for p in case.parts]
    return recs[0] if len(recs) == 1 else merged(*recs)


def profiles(case: Case, sel=slice(None)) -> list:
    """The case's profiles on wn[sel]: dvset = dv on the whole grid, 0 on a stretch (as the whole-tile test of test_fullsize.py)."""
    a = synth.standard_atmosphere(64)
    whole = isinstance(sel, slice) and sel == slice(None)
    out = []
    for ip, layers in enumerate(case.layers):
        lay = np.array(layers)
        wkl = a["wkl"][lay].copy()
        for p, k, mol in case.zero:
            if p == ip:
                wkl[k, mol - 1] = 0.0
        tz = np.concatenate([a["tz"][lay], a["tz"][lay[-1] + 1:lay[-1] + 2]])
        out.append(synth.Profile(wn=case.wn[sel], p=a["p"][lay], t=a["t"][lay], tz=tz, wkl=wkl, wbrodl=a["wbrodl"][lay], clw=a["clw"][lay],
                                 irt=3, dvset=case.dv if whole else 0.0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the host's choices
# ---------------------------------------------------------------------------------------------------------------------------------
def far_level_count(ntile: int, l: int) -> int:
    return (ntile + (1 << l) - 1) >> l


def far_level_offset(ntile: int, l: int) -> int:
    return sum(far_level_count(ntile, k) for k in range(l))


def lines_config(nwn: int, real_kind: int, states: int, span: float) -> tuple:
    """(waves per workgroup, wavenumbers per lane) of lines_kernel.hip."""
    if nwn <= 64:
        return 1, 1
    if real_kind == 4 and 128 < nwn <= 256 and states >= 8192 and span <= 12.5:
        return 1, 4
    if nwn <= 256:
        return 1, 2
    return 4, 2


def nwf_of(steps: float) -> int:
    return 1 if steps <= 16.0 else (2 if steps <= 32.0 else (4 if steps <= 128.0 else 8))


def far_xcd_share(mol_start, m: int) -> tuple:
    """(first XCD, XCDs) of molecule m (0-based): device_common.hpp."""
    base, n = mol_start[1], mol_start[NMOL + 1] - mol_start[1]
    s0, s1 = mol_start[m + 1] - base, mol_start[m + 2] - base
    if n <= 0 or s1 <= s0:
        return 0, 0
    lo = min((16 * s0 + n) // (2 * n), 7)
    hi = max(min((16 * s1 + n) // (2 * n), 8), lo + 1)
    return int(lo), int(hi - lo)


def kept_records(rec: LineRecords, v1: float, v2: float) -> np.ndarray:
    """Indices of the records the context holds: the file's blocks of 250 from the first that ends at or above v1 - 25 to the first
    that ends beyond v2 + 25 (line_table.cpp, lnfl_mod.f90:116, :160-165)."""
    keep = []
    for s in range(0, len(rec), NLINEREC):
        blk = np.arange(s, min(s + NLINEREC, len(rec)))
        if rec.vnu[blk].max() < max(0.0, v1 - 25.0):
            continue
        keep.append(blk)
        if rec.vnu[blk[-1]] > v2 + 25.0:
            break
    return np.concatenate(keep)


@functools.lru_cache(maxsize=None)
def plan(case: Case, real_kind: int = 8, tile_waves=None, far_levels=None) -> types.SimpleNamespace:
    """What one MODM call of the case does on the host, up to the launches of far_kernel."""
    rec, wn = records(case), case.wn
    assert np.all(rec.iflg == 0) and np.all(np.diff(rec.vnu) >= 0)
    tile_waves = case.tile_waves if tile_waves is None else tile_waves
    far_levels = case.far_levels if far_levels is None else far_levels
    nwn, v1, v2 = case.nwn, float(wn[0]), float(wn[-1])
    nprof, nlay_max = len(case.layers), max(len(l) for l in case.layers)
    kept = kept_records(rec, v1, v2)
    mol = rec.mol[kept] % 100
    order = np.argsort(mol, kind="stable")              # the table: molecule by molecule, file order inside
    table = kept[order]
    mol_start = np.zeros(NMOL + 34, np.int64)            # [mol] 1-based, as DevLines::mol_start
    for m in range(1, len(mol_start)):
        mol_start[m] = np.count_nonzero(mol < m)
    nlines = len(kept)
    lines_per_cm = nlines / max(float(rec.vnu[kept].max() - rec.vnu[kept].min()), 1.0)
    nactive = sum(1 for m in range(1, NMOL + 1) if mol_start[m + 1] > mol_start[m])
    nw, wpl = lines_config(nwn, real_kind, nprof * nlay_max, v2 - v1)

    def levels_for(tw):
        if nwn < 2:
            return 0
        nt = (nwn + tw - 1) // tw
        rho_tile = 0.5 * tw * (v2 - v1) / (nwn - 1)
        if FAR_KAPPA * rho_tile >= 25.0 - rho_tile or nt > 65535:
            return 0
        levels = 1
        while levels < FAR_MAXLEV and rho_tile * (1 << levels) <= 3.0 and far_level_count(nt, levels - 1) > 1:
            levels += 1
        return levels if far_levels is None else min(far_levels, FAR_MAXLEV)

    def bytes_for(tw, levels):
        nt = (nwn + tw - 1) // tw
        ni, states = far_level_offset(nt, levels), nprof * nlay_max
        return states * ni * NMOL * (FAR_MOM_STRIDE * 8 + FAR_GEOM_INTS * 4) + states * nt * NMOL * FAR_SEG_INTS * 4

    assert nprof * nlay_max * nlines * 48 <= PHYS_CAP
    if nw == 4 and wpl == 2 and far_levels != 0:
        dvm = (v2 - v1) / max(nwn - 1, 1)
        for cand in (1, 2):
            tw = 128 * cand
            lv = levels_for(tw)
            if nwn >= 4 * tw and lines_per_cm * 2.4 * (0.5 * tw * dvm) >= 1000.0 and lv > 0 and bytes_for(tw, lv) <= FAR_CAP:
                nw = cand
                break
    if tile_waves != "auto" and wpl >= 2:
        nw, wpl = int(tile_waves), 2
    tw = 64 * nw * wpl
    ntile = (nwn + tw - 1) // tw
    levels = levels_for(tw) if (wpl == 2 and ntile >= 4 and nlines > 0) else 0
    assert bytes_for(tw, max(levels, 1)) <= FAR_CAP
    rho_tile = 0.5 * tw * (v2 - v1) / max(nwn - 1, 1)
    steps, nwf = [], []
    for l in range(levels):                               # (launched top first; listed from the tiles up)
        rho_l = rho_tile * (1 << l)
        width = max(50.0 - 2.4 * rho_l, 4.4 * rho_l) if l == levels - 1 else 4.4 * rho_l
        steps.append(lines_per_cm * width / max(nactive, 1) / 128.0)
        nwf.append(nwf_of(steps[-1]))
    return types.SimpleNamespace(case=case, rec=rec, wn=wn, nwn=nwn, table=table, mol_start=mol_start, nlines=nlines, lines_per_cm=lines_per_cm,
                                 nactive=nactive, tw=tw, ntile=ntile, levels=levels, rho_tile=rho_tile, steps=steps, nwf=nwf,
                                 vnu=rec.vnu[table], max_abs_shift=float(2.0 * np.abs(rec.pshift[kept].astype(np.float64)).max()),
                                 ni=far_level_offset(ntile, levels))


def threshold_margin(steps: float) -> float:
    return min(abs(steps - t) / t for t in THRESHOLDS)


# ---------------------------------------------------------------------------------------------------------------------------------
# far_plan_kernel for one (interval, molecule, layer state)
# ---------------------------------------------------------------------------------------------------------------------------------
def layer_state(pr, lay: int) -> types.SimpleNamespace:
    P, T, wk, wbrod = float(pr.p[lay]), float(pr.t[lay]), pr.wkl[lay], float(pr.wbrodl[lay])
    rhorat = ((P / (K_BOLTZ * T)) * 1e3) / ((K_P0 / (K_BOLTZ * K_T0)) * 1e3)
    return types.SimpleNamespace(P=P, T=T, W=wk, WTOT=float(wk.sum()) + wbrod, RHORAT=rhorat)


def interval(pl, l: int, j: int) -> types.SimpleNamespace:
    t0, t1 = j << l, min(pl.ntile, (j + 1) << l)
    a, b = float(pl.wn[t0 * pl.tw]), float(pl.wn[min(pl.nwn, t1 * pl.tw) - 1])
    return types.SimpleNamespace(a=a, b=b, c=0.5 * (a + b), rho=0.5 * (b - a), first=t0 * pl.tw, last=min(pl.nwn, t1 * pl.tw) - 1)


def far_contains(g, i):
    i = np.asarray(i)
    return (((i >= g[0]) & (i < g[1])) | ((i >= g[2]) & (i < g[3]))) & (i >= g[4]) & ~((i >= g[5]) & (i < g[6]))


def _runs(lo: int, hi: int, breaks) -> list:
    """[lo, hi) cut at every breakpoint inside it, as the kernels' `while (pos < end)` loops do."""
    cuts = sorted({lo, hi} | {int(b) for b in breaks if lo < b < hi})
    return list(zip(cuts[:-1], cuts[1:]))


def geometry(pl, st, l: int, j: int, mol: int) -> types.SimpleNamespace:
    """FarGeom of (interval (l, j), molecule) in state st: g (seven indices into the table; zeros: no far lines), the level whose
    interval gave them (`src`; > l: inherited, None: nothing), the guard's margin where it decided, the tile's candidate window."""
    ms0, ms1 = int(pl.mol_start[mol]), int(pl.mol_start[mol + 1])
    v = pl.vnu[ms0:ms1]
    pad = pl.max_abs_shift * max(st.RHORAT, 1.0) + 1e-6
    W = float(st.W[mol - 1])
    molok = W != 0.0 and ms1 > ms0            # (the lists here: sorted, uncoupled, finite states)
    hwdmax = 0.0
    if molok:
        dop = np.sqrt(2.0 * np.log(2.0) * ((K_BOLTZ * st.T) / (LIGHTEST[mol] / K_AVOGAD))) / K_CLIGHT
        hwdmax = (float(v[-1]) + pad) * dop
    g, src, guard = (0,) * 7, None, []
    clo, chi = ms0, ms1
    jj = j
    for ll in range(l, pl.levels):
        cur = interval(pl, ll, jj)
        lhs, rhs = (FAR_KAPPA - 1.0) * cur.rho - 2.0 * pad, 100.0 * hwdmax * 1.000001
        farok = molok and cur.rho > 0.0 and lhs > rhs
        if molok and cur.rho > 0.0:
            guard.append(abs(lhs - rhs) / max(abs(rhs), 1e-300))
        if farok or ll == l:
            kr = FAR_KAPPA * cur.rho
            key = (cur.b - 25.0 + pad, cur.c - kr - pad, cur.c + kr + pad, cur.a + 25.0 - pad, kr - cur.c + pad, 25.0 - cur.b - pad,
                   25.0 - cur.a + pad, cur.a - 25.0 - pad, cur.b + 25.0 + pad)
            incl = (False, True, False, True, False, True, True, False, True)
            lo = [ms0 + int(np.searchsorted(v, k, side="right" if i else "left")) for k, i in zip(key, incl)]
            if ll == l:
                clo, chi = lo[7], max(lo[7], lo[8])
            if farok:
                g = (lo[0], lo[1], lo[2], lo[3]) + ((ms0, ms0, ms0) if mol == CO2 else (lo[4], lo[5], max(lo[5], lo[6])))
                src = ll
                break
        jj >>= 1
    if W == 0.0:
        clo = chi = ms0
    return types.SimpleNamespace(g=g, src=src, guard=min(guard) if guard else np.inf, clo=clo, chi=chi, ms0=ms0, ms1=ms1, molok=molok, pad=pad)


def kernel_runs(pl, st, l: int, j: int, mol: int) -> list:
    """The runs far_kernel expands for (interval, molecule): (pos, next, two) - the interval's far lines minus its parent's."""
    ge = geometry(pl, st, l, j, mol)
    gp = geometry(pl, st, l + 1, j >> 1, mol).g if l + 1 < pl.levels else (0,) * 7
    out = []
    for pos, nxt in _runs(ge.ms0, ge.ms1, ge.g + gp):
        if far_contains(ge.g, pos) and not far_contains(gp, pos):
            out.append((pos, nxt, mol != CO2 and pos < ge.g[5]))
    return out


def tile_runs(pl, st, j: int, mol: int) -> list:
    """The runs of candidate lines left to tile j (farseg): (first, end), joined where one continues the other."""
    ge = geometry(pl, st, 0, j, mol)
    out = []
    for pos, nxt in _runs(ge.clo, ge.chi, ge.g):
        if not far_contains(ge.g, pos):
            if out and out[-1][1] == pos:
                out[-1] = (out[-1][0], nxt)
            else:
                out.append((pos, nxt))
    return out


def anything_there(pl, st, l: int, j: int, mol: int) -> bool:
    """farmom's flag of (interval, molecule): it expands lines of its own or an ancestor does."""
    return any(kernel_runs(pl, st, ll, j >> (ll - l), mol) for ll in range(l, pl.levels))


# ---------------------------------------------------------------------------------------------------------------------------------
# the steps of far_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def line_physics(pl, st, mol: int):
    """(shifted centre, Lorentz half width) of every table line of the molecule in state st (line_physics_core without coupling and
    species broadening; for the census - the kernel reads physics_kernel's records)."""
    ms0, ms1 = int(pl.mol_start[mol]), int(pl.mol_start[mol + 1])
    r, idx = pl.rec, pl.table[ms0:ms1]
    alpf, alps = r.alfa[idx].astype(np.float64), r.hwhm[idx].astype(np.float64)
    if mol == O2:
        alpf = (alpf - 0.21 * alps) / (1.0 - 0.21)
    rho_self = st.RHORAT * float(st.W[mol - 1]) / st.WTOT
    rtx = np.exp(r.tmpalf[idx].astype(np.float64) * np.log(K_T0 / st.T))
    return r.vnu[idx] + r.pshift[idx].astype(np.float64) * st.RHORAT, alpf * rtx * (st.RHORAT - rho_self) + alps * rtx * rho_self


def far_order(dmin: float, rinv: float) -> int:
    """lines_device.hpp, in float32 as the device forms it."""
    f = np.float32
    z = f(dmin * rinv)
    rho = f(z + np.sqrt(np.maximum(f(z * z) - f(1.0), f(0.0)), dtype=np.float32))
    return int(min(FAR_P, max(8, int(f(34.5) / np.log(np.maximum(rho, f(1.0001)), dtype=np.float32)) + 3)))


def steps_of(pl, st, l: int, j: int, mol: int) -> list:
    """Every step (128 lines: two a lane) of far_kernel for (interval, molecule): dicts of lines, two, order, negA (a pole with
    h^2 > delta^2 - rho^2: the A < 0 branch of far_slot_of), run_lines (far lines of the step's run)."""
    iv = interval(pl, l, j)
    runs = kernel_runs(pl, st, l, j, mol)
    if not runs or iv.rho <= 0.0:
        return []
    ms0 = int(pl.mol_start[mol])
    xnu, hw = line_physics(pl, st, mol)
    out = []
    for pos, nxt, two in runs:
        for i0 in range(pos, nxt, 128):
            sl = slice(i0 - ms0, min(i0 + 128, nxt) - ms0)
            d = [xnu[sl] - iv.c] + ([-(xnu[sl] + iv.c)] if two else [])
            dmin = min(float(np.abs(x).min()) for x in d)
            neg = any(bool(np.any(hw[sl] ** 2 > x * x - iv.rho * iv.rho)) for x in d)
            out.append(dict(lines=sl.stop - sl.start, two=two, order=far_order(dmin, 1.0 / iv.rho), negA=neg, run_lines=nxt - pos,
                            kappa=dmin / iv.rho))
    return out


def states(case: Case):
    for ip, pr in enumerate(profiles(case)):
        for lay in range(pr.nlay):
            yield ip, lay, layer_state(pr, lay)


@functools.lru_cache(maxsize=None)
def census(case: Case, only: int | None = None) -> types.SimpleNamespace:
    """What the case reaches over all its states and intervals, for every molecule with lines or for `only` (double precision, the
    tiles the case runs with): counts of (interval, molecule, state) items, of steps and of runs."""
    pl = plan(case)
    c = types.SimpleNamespace(two=0, excl=0, e0=0, inherit=0, stub_parent=0, short_run_multiwave=0, idle_waves=0, negA=0, full_order=0, lds=0,
                              short_order=0, flag_only=0, no_parent=0, reexpand_only=0, orders=set(), min_guard=np.inf, min_kappa=np.inf)
    mols = [m for m in range(1, NMOL + 1) if pl.mol_start[m + 1] > pl.mol_start[m] and only in (None, m)]
    for _ip, _lay, st in states(case):
        for l in range(pl.levels):
            for j in range(far_level_count(pl.ntile, l)):
                iv = interval(pl, l, j)
                for mol in mols:
                    ge = geometry(pl, st, l, j, mol)
                    c.min_guard = min(c.min_guard, ge.guard)
                    if not ge.molok:
                        c.flag_only += 1
                        continue
                    c.inherit += ge.src is not None and ge.src > l
                    if l + 1 < pl.levels and interval(pl, l + 1, j >> 1).rho == 0.0 and anything_there(pl, st, l + 1, j >> 1, mol):
                        c.stub_parent += 1
                    own = kernel_runs(pl, st, l, j, mol)
                    up = l + 1 < pl.levels and anything_there(pl, st, l + 1, j >> 1, mol)
                    c.no_parent += bool(own) and l + 1 < pl.levels and not up
                    c.reexpand_only += (not own) and up
                    if iv.rho > 0.0 and ge.src == l:
                        c.excl += ge.g[6] > ge.g[5]
                        c.e0 += ge.g[4] > ge.ms0
                    for s in steps_of(pl, st, l, j, mol):
                        c.two += s["two"]
                        c.negA += s["negA"]
                        c.full_order += s["order"] == FAR_P
                        c.lds += s["order"] > FAR_PREG
                        c.short_order += s["order"] < FAR_PREG
                        c.orders.add(s["order"])
                        c.min_kappa = min(c.min_kappa, s["kappa"])
                        if pl.nwf[l] > 1 and s["run_lines"] < 128:
                            c.short_run_multiwave += 1
                    for pos, nxt, _two in own:
                        c.idle_waves += pl.nwf[l] > 1 and (nxt - pos + 127) // 128 < pl.nwf[l]
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# what is compared
# ---------------------------------------------------------------------------------------------------------------------------------
def stretches(case: Case) -> list:
    """(label, slice) of the wavenumbers held to the oracle: the first tile, the tiles either side of the first pair boundary, with three
    levels or more those either side of the first boundary between groups of four, and the last tile (a stub included) - of tiles wider
    than MAX_POINTS the MAX_POINTS wavenumbers at the end in question."""
    pl = plan(case)
    tw, nwn, k = pl.tw, pl.nwn, min(pl.tw, MAX_POINTS)
    out = [("first tile", slice(0, k)), ("pair boundary", slice(2 * tw - k, min(2 * tw + k, nwn)))]
    if pl.levels >= 3 and pl.ntile > 4:
        out.append(("four boundary", slice(4 * tw - k, min(4 * tw + k, nwn))))
    last0 = (pl.ntile - 1) * tw
    out.append(("last tile", slice(max(last0, nwn - k) if nwn - last0 > 1 else last0 - k, nwn)))
    # (few tiles: a stretch that lies inside an earlier one is not run twice)
    return [(w, s) for i, (w, s) in enumerate(out) if not any(o.start <= s.start and s.stop <= o.stop for _w, o in out[:i])]


def row_error(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """[nlay, nmol]: max over the stretch of |got - ref| / max over the stretch of |ref|; a row of zeros in the reference must be zeros
    (inf otherwise)."""
    peak = np.abs(ref).max(axis=-1)
    diff = np.abs(got - ref).max(axis=-1)
    return np.where(peak > 0, diff / np.where(peak > 0, peak, 1.0), np.where(diff > 0, np.inf, 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
CASES = {}


def _case(*a, **k):
    c = Case(*a, **k)
    assert c.name not in CASES
    CASES[c.name] = c
    return c


O3_LIST = Part(O3, 14600, 11)          # 430 lines per cm-1 on the 0.0035 cm-1 grids: 154 steps at the top, 13 at the tiles
O3_HALF = Part(O3, 14000, 11)          # beside a second molecule with lines (steps halve): 70 steps at the top
O3_DENSE = Part(O3, 19500, 11)         # 574 lines per cm-1: 20 steps for an interval of half-width 1.024
TWO_PROFILES = ((0, 63), (0, 63))

_case("o3_top8", (O3_LIST,), 0.5, 0.0035, 2100, (1, 8), nslice=3, single=True, tags=("generic",), focus=O3)
# (tiles, top) = (2, 4) needs steps_top / steps_tile <= 115.2 / 17.6 = 6.5; two levels chosen by the call give (50 - 4.8 r) / (4.4 r)
# >= 6.48 (r <= 1.5) and three or more give a top that is further away still: only a forced level count on a coarse grid gets there
_case("o3_top4_tile2", (Part(O3, 11700, 11),), 0.5, 0.0113, 2100, (2, 4), far_levels=2, tags=("generic", "forced_levels"), focus=O3)
_case("o3_three_levels", (Part(O3, 15200, 11),), 0.5, 0.0029, 2200, (1, 2, 8), tags=("generic",), focus=O3)
_case("co2_nwf4", (Part(CO2, 6000, 12),), 0.5, 0.004, 2100, (1, 4), single=True, tags=("co2",), focus=CO2)
_case("co2_nwf2", (Part(CO2, 2500, 12),), 0.5, 0.004, 2100, (1, 2), tags=("co2",), focus=CO2)
_case("o2_nwf4", (Part(O2, 6000, 13),), 0.5, 0.004, 2100, (1, 4), tags=("o2",), focus=O2)
# (from 0.2 cm-1, not 0.4: a line is cut off by e0 when it lies below 0.2 r - v1, and the top level has r = 2.048)
_case("h2o_two_resonances", (Part(H2O, 18000, 14),), 0.2, 0.002, 2600, (1, 2, 8), single=True, tags=("two", "excl", "e0"), focus=H2O)
_case("idle_waves", (O3_HALF, Part(CO2, 60, 12)), 0.5, 0.004, 2100, (1, 4), layers=TWO_PROFILES, zero=((1, 1, O3),),
      tags=("idle", "placement", "zero_column"), focus=CO2)
_case("ragged_batch", (O3_LIST,), 0.5, 0.0035, 2100, (1, 8), layers=((0, 30, 63), (0, 63)), tags=("ragged",), focus=O3)
_case("stub_tile", (Part(O3, 15050, 11),), 0.5, 0.004, 4 * 128 + 1, (1, 1, 2, 8), tile_waves=1, tags=("stub", "inherit", "stub_parent"), focus=O3)
_case("small_tiles_1", (O3_DENSE,), 0.5, 0.004, 1700, (1, 1, 2, 8), tile_waves=1, tags=("generic",), focus=O3)
_case("small_tiles_2", (O3_DENSE,), 0.5, 0.004, 1700, (1, 2, 8), tile_waves=2, tags=("generic",), focus=O3)
_case("narrow_tiles_wide_lines", (Part(O3, 17200, 11),), 0.5, 0.001, 2600, (1, 1, 1, 1, 2, 8), tile_waves=1,
      tags=("negA", "full_order", "short_order", "inherit"), focus=O3)
_case("far_only_molecule", (O3_HALF, Part(CO2, 300, 12, (12.0, 20.0))), 0.5, 0.004, 2100, (1, 4), tags=("far_only",), focus=CO2)
_case("near_clusters", (O3_HALF, Part(CO2, 24, 12, (4.21, 4.36))), 0.5, 0.004, 2048, (1, 4), tags=("near_cluster",), focus=CO2)

SGL_CASES = [n for n, c in CASES.items() if c.single]
RUNS = [(n, 8) for n in CASES] + [(n, 4) for n in SGL_CASES]
