"""The reference of tests/test_xsec_jac_cpu.py and tests/test_xsec_jacobian.py: the cross sections' optical depth ODXSEC as a function of
(P, T) ON THE BASE STATE'S DISCRETISATION, restated in numpy, and its derivatives in T and ln P.

A helper module like tests/jvar_truth.py and tests/xsec_cases.py (no fixture, no test); nothing here runs on a GPU or loads the
product's library.

MONORTM_XSEC_SUB / convolve of the reference (src/monortm_sub.F90:1540-1834) take a handful of discrete decisions from a layer's (P, T):
is the region processed and the wavenumber in range, the temperature bracket, the two clamps of hwd (hwd = max(hwd, hwdop);
hwd > hwpave), step against delvx, npts = int((v2x - v1x) / step), the walk or the linear branch, ind, and the trip at which the walk
stops.  plan() takes every one of them at the base (P, T), in plain double and in the reference's order of operations, so that they
ARE the reference's; evaluate() is the same finite sum at any (P', T') with those decisions held, in numpy longdouble.  With the
discretisation frozen the sum is analytic in (P', T'): its central differences converge as h^2, which the kernel's own re-planned
states do not (tests/test_xsec_jac_cpu.py keeps both facts).

The two table terms of a grid value, d / radfn(vv, tx / RADCN2) at either temperature of the bracket, do not depend on the state: a
plan holds them for every grid point the walk sums, and an evaluation costs the Lorentz weights and one dot product.

Reference derivatives: Richardson central differences of evaluate(), (4 D(h) - D(2h)) / 3, h = 0.1 K in T and 1e-3 in ln P, with the
same from h / 2 and h beside them - the self-spread, as jvar_truth has it.
"""
from __future__ import annotations

import types

import numpy as np

import xsec_cases as xc

LD = np.longdouble
RADCN2 = 1.4387752
H_T, H_LNP = 0.1, 1e-3                 # Richardson steps of the reference: h and 2 h (and h / 2 for the self-spread)
KERNEL_DT, KERNEL_DLNW = 1e-2, 1e-4    # the kernel's own half-steps (api.JAC_DT, api.JAC_DLNW)


def radfn(vi, xkt):
    """RADFN (src/lblrtm_sub.f90:36-97) in the precision of its arguments."""
    vi = np.asarray(vi)
    x = vi / xkt
    e = np.exp(-np.minimum(x, 50))
    return np.where(x <= 0.01, 0.5 * x * vi, np.where(x <= 10, vi * (1 - e) / (1 + e), vi))


_FLAT = {}


def flat(tabs):
    if id(tabs) not in _FLAT:
        _FLAT[id(tabs)] = tabs.flatten()
    return _FLAT[id(tabs)]


def plan(tabs, r: int, wn: float, P: float, T: float, all_wn=xc.WN):
    """The decisions of region r for the wavenumber wn of a layer at (P, T), and the state-independent table terms of every grid point
    its sum visits.  None: the region is not processed in a call of the wavenumbers all_wn, or wn lies outside its header's range."""
    reg, temps, pres, offs, pool = flat(tabs)
    _, v1f, v2f, nptsx, nt, xdop, v1x, v2x = reg[r]
    nptsx, nt = int(nptsx), int(nt)
    if not ((all_wn >= v1f - 1.0) & (all_wn <= v2f + 1.0)).any():
        return None
    if wn < v1x or wn > v2x:
        return None
    tx, pdx = temps[r], pres[r]
    # the bracket (:1677-1704): a layer exactly at a table temperature takes what `tave <= tx` picks
    c1, c2, bracket = 1.0, 0.0, False
    if nt == 1 or T <= tx[0]:
        i1 = i2 = 0
    else:
        it = 1
        while True:
            it += 1
            if it > nt:
                i1 = i2 = nt - 1
                break
            if T <= tx[it - 1]:
                i1, i2, bracket = it - 2, it - 1, True
                c1 = (T - tx[it - 1]) / (tx[it - 2] - tx[it - 1])
                c2 = 1.0 - c1
                break
    pd = c1 * pdx[i1] + c2 * pdx[i2]
    delvx = (v2x - v1x) / (nptsx - 1)
    hwdop = xdop * np.sqrt(T / 296.0)
    hwp = 0.1 * (P / 1013.0) * (273.15 / T)
    hwd = 0.1 * (pd / 1013.0) * (273.15 / T)
    dop = bool(hwdop > hwd)
    hwd = max(hwd, hwdop)
    widen = bool(hwd > hwp)
    if widen:
        hwp = 1.001 * hwd
    hwb = hwp - hwd
    step = 0.25 * hwb
    clip = bool(step > delvx)
    if clip:
        step = delvx
    npts = int((v2x - v1x) / step)
    step = (v2x - v1x) / npts
    ratio = step / hwb
    walk = bool(hwb / hwd > 0.1)
    pl = types.SimpleNamespace(r=r, wn=float(wn), i1=i1, i2=i2, bracket=bracket, dop=dop, widen=widen, clip=clip, npts=npts, step=step,
                               walk=walk, trips=0, xdop=xdop, tx=tx, pdx=pdx)
    d1, d2 = pool[offs[r][i1]: offs[r][i1] + nptsx], pool[offs[r][i2]: offs[r][i2] + nptsx]

    def terms(i, dt):
        """xspd's two terms at the 1-based points i of the file's grid, in dtype dt: d1 / radfn(vv, xkt1), d2 / radfn(vv, xkt2)"""
        i = np.asarray(i)
        ok = (i >= 1) & (i <= nptsx)
        ii = np.clip(i, 1, nptsx)
        vv = dt(v1x) + (ii - 1).astype(dt) * dt(delvx)
        return (np.where(ok, d1[ii - 1].astype(dt) / radfn(vv, dt(tx[i1]) / dt(RADCN2)), dt(0)),
                np.where(ok, d2[ii - 1].astype(dt) / radfn(vv, dt(tx[i2]) / dt(RADCN2)), dt(0)))

    def grid_terms(i, dt):
        """xspd_int's two terms at the points i of the resampled grid (:1779-1785); the index and the weight in double, as the
        reference forms them"""
        i = np.asarray(i)
        delvv = (v1x + i * step) - v1x
        ind = (delvv / delvx).astype(np.int64)
        cf = dt(1) * ((delvv - ind * delvx) / delvx)
        a1, a2 = terms(ind + 1, dt)
        b1, b2 = terms(ind + 2, dt)
        return (1 - cf) * a1 + cf * b1, (1 - cf) * a2 + cf * b2

    if not walk:
        ind = int((wn - v1x) / delvx)
        pl.ind = ind
        pl.cf = ((wn - v1x) - ind * delvx) / delvx
        pl.t1, pl.t2 = terms(np.array([ind, ind + 1]), LD)
        return pl
    ind = int((wn - v1x) / step)
    pl.ind = ind
    hwb2 = hwb * hwb

    def lor(i):
        dv = wn - (v1x + i * step)
        return hwb / (hwb2 + dv * dv)

    def xint(i):
        a, b = grid_terms(i, np.float64)
        return c1 * a + c2 * b

    first = np.array([ind, ind + 1])
    ans = float((lor(first) * xint(first)).sum())
    thr = ratio * 1e-6
    J, CH = 0, 128                                          # (chunks that grow: most walks stop within a few hundred trips)
    while True:   # the walk (:1797-1817) in double and in the reference's order: the running sum before trip j decides
        j = np.arange(J + 1, J + CH + 1)
        lo = np.where(v1x + (ind - j) * step > v1x, lor(ind - j) * xint(ind - j), 0.0)
        hi = np.where(v1x + (ind + j + 1) * step < v2x, lor(ind + j + 1) * xint(ind + j + 1), 0.0)
        inc = lo + hi
        run = np.cumsum(np.concatenate(([ans], inc)))       # run[k]: the sum before trip J + k + 1
        with np.errstate(divide="ignore", invalid="ignore"):
            stop = np.nonzero(inc / run[:-1] < thr)[0]
        if len(stop):
            pl.trips = J + int(stop[0]) + 1                 # the trip that met the criterion (and is not summed), as the trace counts
            nsum = J + int(stop[0])
            break
        ans = float(run[-1])
        J += CH
        CH = min(2 * CH, 4096)
        if ind - J < 0 and ind + J + 1 > npts:
            pl.trips = J
            nsum = J
            break
    j = np.arange(1, nsum + 1)
    lo_i, hi_i = ind - j, ind + j + 1
    lo_i, hi_i = lo_i[v1x + lo_i * step > v1x], hi_i[v1x + hi_i * step < v2x]
    pts = np.concatenate((first, lo_i, hi_i))
    pl.dv = (wn - (v1x + pts * step)).astype(LD)            # the grid is the plan's: its points as the reference's double has them
    pl.t1, pl.t2 = grid_terms(pts, LD)
    return pl


def evaluate(pl, P, T):
    """The region's term of ODXSEC per unit column amount at (P, T) on the plan pl: the frozen sum times radfn(wn, T / RADCN2),
    in longdouble.  P, T: scalars, or arrays of states [ns] -> [ns]."""
    P, T = np.atleast_1d(np.asarray(P, LD)), np.atleast_1d(np.asarray(T, LD))
    tx, pdx = pl.tx, pl.pdx
    c1, c2 = np.ones_like(T), np.zeros_like(T)
    if pl.bracket:   # the bracket's linear form, extrapolated where T leaves it; constant where the base has none
        c1 = (T - LD(tx[pl.i2])) / (LD(tx[pl.i1]) - LD(tx[pl.i2]))
        c2 = 1 - c1
    rf = radfn(LD(pl.wn), T / LD(RADCN2))
    x = c1[:, None] * pl.t1[None, :] + c2[:, None] * pl.t2[None, :]
    if not pl.walk:
        return ((1 - LD(pl.cf)) * x[:, 0] + LD(pl.cf) * x[:, 1]) * rf
    pd = c1 * LD(pdx[pl.i1]) + c2 * LD(pdx[pl.i2])
    hwp = LD(0.1) * (P / LD(1013.0)) * (LD(273.15) / T)
    hwd = LD(0.1) * (pd / LD(1013.0)) * (LD(273.15) / T)
    if pl.dop:
        hwd = LD(pl.xdop) * np.sqrt(T / LD(296.0))
    if pl.widen:
        hwp = LD(1.001) * hwd
    hwb = (hwp - hwd)[:, None]
    s = np.sum((hwb / (hwb * hwb + (pl.dv * pl.dv)[None, :])) * x, axis=1)
    return s * LD(pl.step) / LD(3.14159) * rf


class Frozen:
    """ODXSEC [nlay, nwn] of one profile as a function of (P', T') on the plans of its base state."""

    def __init__(self, tabs, pr):
        reg = flat(tabs)[0]
        self.pr, self.mol = pr, reg[:, 0].astype(int)
        self.nreg, self.nmol = len(reg), len(tabs.names)
        self.plans = [[[plan(tabs, r, w, pr.p[k], pr.t[k]) for r in range(self.nreg)] for w in xc.WN] for k in range(pr.nlay)]

    def units(self, states) -> np.ndarray:
        """Per molecule and unit column amount, at every state (dT, dlnP, mul) - T + dT and P exp(dlnP) or, mul, P (1 + dlnP), the
        kernel's own state: longdouble [ns, nmol, nlay, nwn]"""
        pr = self.pr
        out = np.zeros((len(states), self.nmol, pr.nlay, len(xc.WN)), LD)
        for k in range(pr.nlay):
            pk = np.array([LD(pr.p[k]) * ((1 + LD(dp)) if mul else np.exp(LD(dp))) for _, dp, mul in states], LD)
            tk = np.array([LD(pr.t[k]) + LD(dt) for dt, _, _ in states], LD)
            for iw in range(len(xc.WN)):
                for r, pl in enumerate(self.plans[k][iw]):
                    if pl is not None:
                        out[:, self.mol[r], k, iw] += evaluate(pl, pk, tk)
        return out

    def _sum(self, units, xamnt):
        xa = np.asarray(self.pr.xamnt if xamnt is None else xamnt, LD)      # [nlay, nmol]
        return np.einsum("smkw,km->skw", units, xa)

    def odxsec(self, xamnt=None, dT: float = 0.0, dlnP: float = 0.0, mul: bool = False) -> np.ndarray:
        return self._sum(self.units([(dT, dlnP, mul)]), xamnt)[0]

    def central_units(self, var: str, steps, mul: bool = False) -> list:
        """Central differences per molecule and unit amount over every step of `steps`: [longdouble [nmol, nlay, nwn]]"""
        st = [((s * h, 0.0, False) if var == "t" else (0.0, s * h, mul)) for h in steps for s in (1.0, -1.0)]
        u = self.units(st)
        return [(u[2 * i] - u[2 * i + 1]) / (2 * LD(h)) for i, h in enumerate(steps)]

    def central(self, var: str, h: float, xamnt=None, mul: bool = False) -> np.ndarray:
        return self._sum(np.stack(self.central_units(var, [h], mul)), xamnt)[0]

    def richardson_units(self, var: str):
        """-> (the derivative from h and 2 h, the same from h / 2 and h) per molecule and unit amount, longdouble [nmol, nlay, nwn]"""
        key = ("rich", var)
        if key not in self.__dict__:
            h = H_T if var == "t" else H_LNP
            half, one, two = self.central_units(var, [0.5 * h, h, 2 * h])
            self.__dict__[key] = ((4 * one - two) / 3, (4 * half - one) / 3)
        return self.__dict__[key]

    def richardson(self, var: str, xamnt=None):
        """-> (d ODXSEC / dT or d ln P from h and 2 h, the same from h / 2 and h), float64 [nlay, nwn]"""
        return tuple(np.asarray(self._sum(d[None], xamnt)[0], np.float64) for d in self.richardson_units(var))


_FROZEN = {}


def frozen(i: int) -> Frozen:
    """Profile i of xsec_cases' call `all` on the tables of xsec_cases, planned once per process."""
    if i not in _FROZEN:
        orc = xc.oracle(8)
        _FROZEN[i] = Frozen(orc.tabs, orc.profs["all"][i])
    return _FROZEN[i]


def layer_scale(d: np.ndarray) -> np.ndarray:
    """The measure of the CPU tests: a layer's largest magnitude, [nlay, 1]"""
    return np.abs(d).max(axis=1, keepdims=True) + 1e-300
