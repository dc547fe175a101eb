"""An extended-precision restatement of CALCTMR + RAD_UP_DN + RTM (reference src/RTMmono.f90:13-325), the input classes that stress
the way the radiance kernels regroup that loop, its derivatives in closed form (truth_adjoint), and the error measures of
tests/test_rtm_truth_cpu.py, tests/test_rtm_extremes.py and tests/test_adjoint_extremes.py.

A helper module like tests/common.py (no fixtures, no test).  Nothing here runs on a GPU or imports the product.

The restatement (truth) is NOT the reference's loop.  It states the same sums in a form that does not cancel, in numpy longdouble
(x87 extended, eps 1.1e-19; asserted at import):
  - the optical depth above and below a layer are direct sums of the other layers, never a running difference from ODTOT;
  - 1 - exp(-tau) is -expm1(-tau), exp(x) - 1 of the Planck function is expm1(x), log(1 + x) of TB and TMR is log1p(x);
  - every array argument may be longdouble already, so that differences of it resolve derivatives to ~1e-12.
It takes a whole ragged batch at once: O [nprof, lm, nwn], T [nprof, lm], TZ [nprof, lm + 1], nlay [nprof]; whatever lies beyond
nlay[p] (levels beyond nlay[p] + 1) is never used, NaN included.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "numpy longdouble is not an extended format on this platform: the truth would need mpmath"

RADCN1, RADCN2, TSKY = LD(1.191042722E-12), LD(1.4387752), LD(2.75)   # the doubles of the reference's phys_consts, widened
OUT = ("rup", "rdn", "trtot", "rad", "tb", "tmr")                      # the output order of monortm_hip_rtm and _rtm_scan
CLASSES = ("lognormal", "thin", "thinnest", "opaque_bottom", "opaque_top", "opaque_middle", "mixed", "underflow", "degenerate")
# the two classes on which the REFERENCE's own 1 - exp(-tau) cancels (tau <= 1e-8: 1 - exp(-tau) keeps 16 + log10(tau) digits)
CANCELLING = ("thinnest", "degenerate")
NWN = 70                                                               # one full block of 64 lanes and one with 6 live lanes
WN = np.geomspace(0.5, 57000.0, NWN)
DBL_TINY, DBL_DENORM = np.finfo(np.float64).tiny, 5e-324
SGL_FLOOR = 1e-30                                                      # the suite's rad_floor of REAL*4 outputs (tests/common.py compare)
BATCHES = {
    "A64": [1, 2, 7, 23, 24, 48, 64],   # few workgroups, nlay_max >= 48 -> G = 16: empty groups, one layer beside 64
    "B30": [5, 24, 30],                 # 24 <= nlay_max < 48            -> G = 8
    "C12": [3, 12],                     # nlay_max < 24                  -> G = 2
    "L200": [200],                      # one long profile               -> G = 16, 13 layers a thread
    "D48": [48] * 140,                  # >= 256 workgroups              -> G = 8 past the few-workgroups rule
}


def _planck(c3, v, T):
    """RADCN1 v^3 / (exp(RADCN2 v / T) - 1); 0 where the exponential overflows the extended range."""
    with np.errstate(all="ignore"):
        return c3 / np.expm1(v * (RADCN2 / T))


def truth(wn, nlay, irt, T, TZ, O, tmpsfc, emiss, reflc):
    """-> dict of longdouble [nprof, nwn]: rup, rdn, trtot, rad, tb, tmr, and the pieces the analytic surface derivatives need
    (surfrad, dsurfrad = dB/dT at the surface temperature RTM uses, cosmos)."""
    nlay, irt = np.asarray(nlay), np.asarray(irt)
    O, T, TZ = np.asarray(O, LD), np.asarray(T, LD), np.asarray(TZ, LD)
    nprof, lm, nwn = O.shape
    lay = np.arange(lm)[None, :] < nlay[:, None]                        # [nprof, lm]
    lev = np.arange(lm + 1)[None, :] <= nlay[:, None]
    O = np.where(lay[:, :, None], O, LD(0))                             # a padded layer: tau = 0 adds no term to any sum
    T, TZ = np.where(lay, T, LD(250)), np.where(lev, TZ, LD(250))
    v = np.asarray(wn, LD)[None, None, :]
    c3 = RADCN1 * (v * v * v)
    with np.errstate(all="ignore"):
        bb, bz = _planck(c3, v, T[:, :, None]), _planck(c3, v, TZ[:, :, None])     # [nprof, lm, nwn], [nprof, lm + 1, nwn]
        zero = np.zeros((nprof, 1, nwn), LD)
        below = np.concatenate([zero, np.cumsum(O, axis=1)[:, :-1]], axis=1)         # sum of the layers under layer l
        above = np.concatenate([np.cumsum(O[:, ::-1], axis=1)[:, ::-1][:, 1:], zero], axis=1)
        odtot = O.sum(axis=1)
        emis = -np.expm1(-O)
        pade = LD(0.193) * O + LD(0.013) * (O * O)
        rdn = (np.exp(-below) * emis * (bb + pade * bz[:, :-1]) / (1 + pade)).sum(axis=1)   # the lower level, RTMmono.f90:210-217
        rup = (np.exp(-above) * emis * (bb + pade * bz[:, 1:]) / (1 + pade)).sum(axis=1)    # the upper level, :197-204
        rup = np.where((irt != 3)[:, None], rup, LD(0))
        trtot = np.exp(-odtot)
        v, c3 = v[:, 0], c3[:, 0]
        tmr = RADCN2 * v / np.log1p(c3 / (rdn / -np.expm1(-odtot)))                  # CALCTMR: the sum is RDN's
        ts = np.where(irt == 1, np.asarray(tmpsfc, LD), TSKY)[:, None]
        x = v * (RADCN2 / ts)
        surfrad, cosmos = c3 / np.expm1(x), c3 / np.expm1(v * (RADCN2 / TSKY))
        dsurfrad = np.where(np.isfinite(np.exp(x)), surfrad * (np.exp(x) / np.expm1(x)) * (x / ts), LD(0))
        em, rf = np.asarray(emiss, LD), np.asarray(reflc, LD)
        i = irt[:, None]
        rad = np.where(i == 1, rup + trtot * (em * surfrad + rf * (rdn + trtot * cosmos)),
                       np.where(i == 2, rup + trtot * (rdn + trtot * cosmos), rdn + trtot * cosmos))
        tb = RADCN2 * v / np.log1p(c3 / rad)
    return dict(rup=rup, rdn=rdn, trtot=trtot, rad=rad, tb=tb, tmr=tmr, surfrad=surfrad, dsurfrad=dsurfrad, cosmos=cosmos, c3=c3)


def oracle(wn, nlay, irt, T, TZ, O, tmpsfc, emiss, reflc):
    """The CPU oracle's orc_rtm / orc_calctmr on the same batch -> dict of float64 [nprof, nwn] and tmpsfc as written back."""
    from oracle.pyoracle import lib

    L = lib()
    c = lambda x: np.ascontiguousarray(x, np.float64)  # noqa: E731
    wn = c(wn)
    nprof, nwn = len(nlay), len(wn)
    out = {k: np.zeros((nprof, nwn)) for k in OUT}
    ts_out = np.zeros(nprof)
    for p in range(nprof):
        n = int(nlay[p])
        t, tz, o = c(T[p, :n]), c(TZ[p, :n + 1]), c(O[p, :n])
        ts = C.c_double(float(tmpsfc[p]))
        with np.errstate(all="ignore"):
            L.orc_calctmr(n, nwn, wn, t, tz, o, out["tmr"][p])
            L.orc_rtm(1, int(irt[p]), nwn, wn, n, t, tz, o, C.byref(ts), out["rup"][p], out["trtot"][p], out["rdn"][p], c(reflc[p]),
                      c(emiss[p]), out["rad"][p], out["tb"][p])
        ts_out[p] = ts.value
    return out, ts_out


# ---- input classes ---------------------------------------------------------------------------------------------------------------
def optical_depths(cls: str, rng, nlay: int, nwn: int = NWN) -> np.ndarray:
    """[nlay, nwn] optical depths per layer of one column class; layer 0 is the lowest."""
    sh = (nlay, nwn)
    pw = lambda lo, hi: 10.0 ** rng.uniform(lo, hi, sh)  # noqa: E731
    third = (nlay + 2) // 3                               # at least one layer
    if cls == "lognormal":
        return np.clip(np.exp(rng.normal(np.log(7e-3), 1.6, sh)), 1e-5, 5.0)
    if cls == "thin":
        return pw(-8, -4)
    if cls == "thinnest":
        return pw(-12, -8)
    if cls in ("opaque_bottom", "opaque_top", "opaque_middle"):
        o, big = pw(-6, -1), pw(2, 4)
        if cls == "opaque_bottom":
            o[:third] = big[:third]
        elif cls == "opaque_top":
            o[nlay - third:] = big[nlay - third:]
        else:
            o[nlay // 2] = 1e6
        return o
    if cls == "mixed":
        return pw(-8, 3)
    if cls == "underflow":
        return 745.0 + 1e4 * rng.uniform(0.0, 1.0, sh)
    if cls == "degenerate":
        kind = rng.integers(0, 3, sh)
        return np.where(kind == 0, 0.0, np.where(kind == 1, 10.0 ** rng.uniform(-323.0, -308.0, sh), pw(-300, -10)))
    raise ValueError(cls)


class Batch:
    """Seeded RTM inputs of a ragged batch, float64; classes[p] names the class of profile p's optical depths.
    rounded(dtype) -> the arrays exactly as a context of that REAL kind receives them, padded with `fill` beyond nlay[p]."""

    def __init__(self, nlay, classes, seed, irt=(1, 2, 3)):
        rng = np.random.default_rng(seed)
        self.nlay = np.array(nlay, np.int32)
        self.nprof, self.lm, self.nwn = len(nlay), int(max(nlay)), NWN
        self.classes = [classes] * self.nprof if isinstance(classes, str) else list(classes)
        n, lm = self.nprof, self.lm
        self.irt = np.array([irt[i % len(irt)] for i in range(n)], np.int32)
        self.wn = WN
        self.O = np.zeros((n, lm, NWN))
        for p in range(n):
            self.O[p, :nlay[p]] = optical_depths(self.classes[p], rng, int(nlay[p]))
        self.T = rng.uniform(180.0, 320.0, (n, lm))
        self.TZ = rng.uniform(180.0, 320.0, (n, lm + 1))
        self.ts = rng.uniform(270.0, 310.0, n)
        self.em = rng.uniform(0.6, 1.0, (n, NWN))
        self.rf = 1.0 - self.em
        self.lay = np.arange(lm)[None, :] < self.nlay[:, None]
        self.lev = np.arange(lm + 1)[None, :] <= self.nlay[:, None]

    def rounded(self, dtype, fill=0.0, O=None):
        r = lambda x: np.ascontiguousarray(x, dtype)  # noqa: E731
        T, TZ, O = r(self.T), r(self.TZ), r(self.O if O is None else O)
        T[~self.lay], TZ[~self.lev], O[~self.lay] = fill, fill, fill
        return dict(T=T, TZ=TZ, O=O, ts=r(self.ts), em=r(self.em), rf=r(self.rf))

    def args(self, a, O=None):
        """The argument tuple of truth() / oracle() from rounded() arrays (O: other optical depths of the same shape)."""
        return (self.wn, self.nlay, self.irt, a["T"], a["TZ"], a["O"] if O is None else O, a["ts"], a["em"], a["rf"])

    def profiles_of(self, cls):
        return [p for p in range(self.nprof) if self.classes[p] == cls]


def cycled_classes(nprof: int, shift: int = 0):
    """Classes cycling over the profiles of a large batch, three profiles (irt 1, 2, 3) per class in a row."""
    return [CLASSES[(p // 3 + shift) % len(CLASSES)] for p in range(nprof)]


def make_batch(name: str, cls: str) -> Batch:
    """The seeded batch BATCHES[name] of one class (or "cycled") that the tests against the truth share."""
    seed = 7000 + 100 * list(BATCHES).index(name) + (CLASSES.index(cls) if cls != "cycled" else 50)
    nlay = BATCHES[name]
    return Batch(nlay, cycled_classes(len(nlay)) if cls == "cycled" else cls, seed)


# ---- the error measure -----------------------------------------------------------------------------------------------------------
def E(a, t, orc, real_kind: int = 8, denormal_slack: bool = False) -> float:
    """max |a - t| / |t| over the elements where t is finite and representable; inf when an element breaks one of the rules:
      - t finite, |t| >= tiny: a must be finite (it enters the maximum);
      - 0 < |t| < tiny, a value the output format holds without full relative precision, or not at all: real_kind 8, tiny = 2.2e-308
        (the smallest normal double), plain |a - t| / |t| - except with denormal_slack, which the callers set for TRTOT alone (the
        one field that is denormal outside `degenerate`: exp(-708 .. -745)): 2 denormal spacings are taken off |a - t|, one
        rounding of the result to the denormal grid and one of exp's; real_kind 4, tiny = 1e-30 (the suite's rad_floor), |a| <= 2e-30;
      - t zero or not finite: a equals the oracle's value orc, or both are NaN.
    a: float32 / float64 results, t: longdouble truth (or the oracle's doubles), orc: the oracle's doubles."""
    a, t, orc = np.asarray(a, LD), np.asarray(t, LD), np.asarray(orc, LD)
    tiny = LD(DBL_TINY) if real_kind == 8 else LD(SGL_FLOOR)
    with np.errstate(all="ignore"):
        fin = np.isfinite(t) & (t != 0)
        big, small = fin & (np.abs(t) >= tiny), fin & (np.abs(t) < tiny)
        ok_small = np.isfinite(a) if real_kind == 8 else np.abs(a) <= 2 * LD(SGL_FLOOR)
        ok_rest = (a == orc) | (np.isnan(a) & np.isnan(orc))
        if real_kind == 4:   # the oracle's double, as a float holds it
            o4 = orc.astype(np.float32).astype(LD)
            ok_rest |= (a == o4) | (np.abs(orc) < tiny) & (np.abs(a) <= 2 * LD(SGL_FLOOR))
        if np.any(small & ~ok_small) or np.any(~fin & ~ok_rest) or np.any(big & ~np.isfinite(a)):
            return float("inf")
        err = np.where(big, np.abs(a - t), LD(0))
        if real_kind == 8:
            slack = 2 * LD(DBL_DENORM) if denormal_slack else LD(0)
            err = np.where(small, np.maximum(np.abs(a - t) - slack, LD(0)), err)
        return float(np.max(np.where(big | small, err / np.abs(t), LD(0)), initial=0.0))


def same_pattern(a, b) -> bool:
    """The same NaN and the same zero pattern."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a == 0, b == 0))


# ---- differences of the truth ------------------------------------------------------------------------------------------------------
def dtb_drad(rad, c3, v):
    """dTB/dRAD of TB = RADCN2 v / log1p(c3 / RAD) in closed form (held to differences of TB by tests/test_rtm_truth_cpu.py)."""
    x = c3 / rad
    return RADCN2 * v * x / (np.log1p(x) ** 2 * (1 + x) * rad)


def truth_derivatives(b: Batch, a: dict, quantities=("rad", "tb")):
    """Richardson-extrapolated central differences (h and 2h: truncation O(h^4)) of the truth's RAD with respect to every layer's
    optical depth (h = 1e-7 max(tau, 1)), layer temperature and level temperature (h = 1e-3 K) -> {quantity: dict of k_o, k_t
    [nprof, lm, nwn], k_tz [nprof, lm + 1, nwn], k_sfc [nprof, 3, nwn] (analytic), q [nprof, nwn]}.  Rounding of the differences:
    eps / h = 1e-12 relative to RAD; truncation (x / T)^5 h^4 < 1e-10 of the derivative at hc v / kT = 455.
    The derivatives of TB are those of RAD times dTB/dRAD = RADCN2 v c3 / (ln^2(1 + c3 / RAD) (1 + c3 / RAD) RAD^2) in closed form:
    TB is logarithmic in RAD, and a step of 1e-7 is not small against a thin column's whole optical depth (1e-8 .. 1e-4 a layer) -
    differences of TB itself are off by 1e-2 there while those of RAD, which is all but linear in a thin tau, hold 1e-11."""
    base = {k: np.asarray(a[k], LD) for k in ("T", "TZ", "O")}
    t0 = truth(*b.args(a))
    rad = dict(k_o=np.zeros((b.nprof, b.lm, b.nwn), LD), k_t=np.zeros((b.nprof, b.lm, b.nwn), LD),
               k_tz=np.zeros((b.nprof, b.lm + 1, b.nwn), LD))

    def diff(name, idx, h):
        d = []
        for hh in (h, 2 * h):
            f = []
            for sgn in (1, -1):
                x = dict(base)
                x[name] = base[name].copy()
                x[name][:, idx] = x[name][:, idx] + sgn * hh
                f.append(truth(b.wn, b.nlay, b.irt, x["T"], x["TZ"], x["O"], a["ts"], a["em"], a["rf"])["rad"])
            d.append((f[0] - f[1]) / (2 * hh))
        return (4 * d[0] - d[1]) / 3

    with np.errstate(all="ignore"):
        for k in range(b.lm):
            act = b.lay[:, k][:, None]
            rad["k_o"][:, k] = np.where(act, diff("O", k, LD(1e-7) * np.maximum(base["O"][:, k], LD(1))), LD(0))
            rad["k_t"][:, k] = np.where(act, diff("T", k, LD(1e-3)), LD(0))
        for j in range(b.lm + 1):
            rad["k_tz"][:, j] = np.where(b.lev[:, j][:, None], diff("TZ", j, LD(1e-3)), LD(0))
        v = np.asarray(b.wn, LD)[None, :]
        dtb = dtb_drad(t0["rad"], t0["c3"], v)
        one = (b.irt == 1)[:, None, None]
        em = np.asarray(a["em"], LD)
        rad["k_sfc"] = np.where(one, np.stack([t0["trtot"] * em * t0["dsurfrad"], t0["trtot"] * t0["surfrad"],
                                               t0["trtot"] * (t0["rdn"] + t0["trtot"] * t0["cosmos"])], axis=1), LD(0))
        res = {}
        for q in quantities:
            dq = dtb[:, None, :] if q == "tb" else LD(1)
            res[q] = {k: np.where(v_ != 0, dq * v_, LD(0)) for k, v_ in rad.items()}
            res[q]["q"] = t0[q]
    return res


def truth_adjoint(wn, nlay, irt, T, TZ, O, tmpsfc, emiss, reflc, quantities=("rad", "tb")):
    """The derivatives of the truth's RAD and TB in closed form, from the sums of truth() itself, in the dict layout of
    truth_derivatives: {quantity: k_o, k_t [nprof, lm, nwn], k_tz [nprof, lm + 1, nwn], k_sfc [nprof, 3, nwn], q [nprof, nwn]}, longdouble.
    With t = exp(-tau), e = -expm1(-tau), p = 0.193 tau + 0.013 tau^2 and f(tau; Bz) = e (B + p Bz) / (1 + p), a layer's term of a sweep:
      RDN = sum_l exp(-below_l) f_l(Bz_l),  RUP = sum_l exp(-above_l) f_l(Bz_{l+1}),  TRTOT = exp(-sum tau), below / above direct sums;
      df/dtau = t (B + p Bz) / (1 + p) + e (0.193 + 0.026 tau) (Bz - B) / (1 + p)^2;
      dRDN/dtau_k = exp(-below_k) df_k/dtau - sum_{l>k} dn_l (tau_k lies below every higher layer), dRUP/dtau_k likewise with l < k;
      dB/dT = B x / T / -expm1(-x), x = hc v / kT, which no exponential overflows; level j is the lower level of layer j (RDN) and the
      upper level of layer j - 1 (RUP);
      RAD's three irt forms (RTMmono.f90:138-147) give dRAD/dRUP, dRAD/dRDN, dRAD/dTRTOT; TB's derivatives are RAD's times dtb_drad.
    Padded layers and levels are exactly 0; what lies beyond nlay[p] is never read.  tests/test_rtm_truth_cpu.py holds it to the
    independent differences of truth_derivatives."""
    nlay, irt = np.asarray(nlay), np.asarray(irt)
    t0 = truth(wn, nlay, irt, T, TZ, O, tmpsfc, emiss, reflc)
    O, T, TZ = np.asarray(O, LD), np.asarray(T, LD), np.asarray(TZ, LD)
    nprof, lm, nwn = O.shape
    lay = np.arange(lm)[None, :] < nlay[:, None]
    lev = np.arange(lm + 1)[None, :] <= nlay[:, None]
    O = np.where(lay[:, :, None], O, LD(0))
    T, TZ = np.where(lay, T, LD(250))[:, :, None], np.where(lev, TZ, LD(250))[:, :, None]
    v = np.asarray(wn, LD)[None, None, :]
    c3 = RADCN1 * (v * v * v)
    with np.errstate(all="ignore"):
        xl, xz = v * (RADCN2 / T), v * (RADCN2 / TZ)
        bb, bz = _planck(c3, v, T), _planck(c3, v, TZ)
        dbb, dbz = bb * (xl / T) / -np.expm1(-xl), bz * (xz / TZ) / -np.expm1(-xz)
        zero = np.zeros((nprof, 1, nwn), LD)
        below = np.concatenate([zero, np.cumsum(O, axis=1)[:, :-1]], axis=1)
        above = np.concatenate([np.cumsum(O[:, ::-1], axis=1)[:, ::-1][:, 1:], zero], axis=1)
        tdn, tup = np.exp(-below), np.exp(-above)
        t, e = np.exp(-O), -np.expm1(-O)
        p, dp = LD(0.193) * O + LD(0.013) * (O * O), LD(0.193) + LD(0.026) * O
        r = 1 / (1 + p)
        bzl, bzu = bz[:, :-1], bz[:, 1:]
        dn, up = tdn * e * (bb + p * bzl) * r, tup * e * (bb + p * bzu) * r
        dfdn = t * (bb + p * bzl) * r + e * dp * (bzl - bb) * (r * r)
        dfup = t * (bb + p * bzu) * r + e * dp * (bzu - bb) * (r * r)
        dn_above = np.concatenate([np.cumsum(dn[:, ::-1], axis=1)[:, ::-1][:, 1:], zero], axis=1)   # sum of dn_l, l > k
        up_below = np.concatenate([zero, np.cumsum(up, axis=1)[:, :-1]], axis=1)                     # sum of up_l, l < k
        drdn, drup = tdn * dfdn - dn_above, tup * dfup - up_below
        i = irt[:, None]
        tr, rdn, cosmos, surfrad = t0["trtot"], t0["rdn"], t0["cosmos"], t0["surfrad"]
        em, rf = np.asarray(emiss, LD), np.asarray(reflc, LD)
        cu = np.where(i == 3, LD(0), LD(1))
        cd = np.where(i == 1, tr * rf, np.where(i == 2, tr, LD(1)))
        ct = np.where(i == 1, em * surfrad + rf * rdn + 2 * rf * tr * cosmos, np.where(i == 2, rdn + 2 * tr * cosmos, cosmos))
        cu, cd, ct_tr = cu[:, None, :], cd[:, None, :], (ct * tr)[:, None, :]
        wz = e * p * r
        k_tz = np.zeros((nprof, lm + 1, nwn), LD)
        k_tz[:, :-1] += cd * tdn * wz * dbz[:, :-1]
        k_tz[:, 1:] += cu * tup * wz * dbz[:, 1:]
        one = (irt == 1)[:, None, None]
        rad = dict(k_o=np.where(lay[:, :, None], cu * drup + cd * drdn - ct_tr, LD(0)),
                   k_t=np.where(lay[:, :, None], (cu * tup + cd * tdn) * e * r * dbb, LD(0)),
                   k_tz=np.where(lev[:, :, None], k_tz, LD(0)),
                   k_sfc=np.where(one, np.stack([tr * em * t0["dsurfrad"], tr * surfrad, tr * (rdn + tr * cosmos)], axis=1), LD(0)))
        dtb = dtb_drad(t0["rad"], t0["c3"], v[0])
        res = {}
        for q in quantities:
            dq = dtb[:, None, :] if q == "tb" else LD(1)
            res[q] = {k: np.where(v_ != 0, dq * v_, LD(0)) for k, v_ in rad.items()}
            res[q]["q"] = t0[q]
    return res


def k_error(k, ref, q, sel=None) -> float:
    """max over (profile, channel) of max_layers |k - ref| / max(max_layers |ref|, 1e-6 |q|): a derivative is compared relative to the
    column's largest one, and to the project's own 1e-6 resolution of q where the column has none above rounding."""
    k, ref, q = np.asarray(k, LD), np.asarray(ref, LD), np.asarray(q, LD)
    if sel is not None:
        k, ref, q = k[sel], ref[sel], q[sel]
    with np.errstate(all="ignore"):
        scale = np.maximum(np.abs(ref).max(axis=1), LD(1e-6) * np.abs(q))
        err = np.abs(k - ref).max(axis=1) / scale
    if not np.all(np.isfinite(k)):
        return float("inf")
    return float(np.max(np.where(scale > 0, err, LD(0))))


# ---- measured figures ----------------------------------------------------------------------------------------------------------------
RECORD: dict = {}


def record(key: str, value: float) -> None:
    """Keep the worst figure per key; printed by the tests (-s) and written out by dump_record()."""
    value = float(value)
    if key not in RECORD or not (value <= RECORD[key]):
        RECORD[key] = value


def dump_record() -> None:
    """Write the figures to the file MONORTM_TRUTH_RECORD names (merged with what it holds), if it is set."""
    path = os.environ.get("MONORTM_TRUTH_RECORD")
    if not path or not RECORD:
        return
    old = {}
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    for k, v in RECORD.items():
        if k not in old or not (v <= old[k]):
            old[k] = v
    with open(path, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)
