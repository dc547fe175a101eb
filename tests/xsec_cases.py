"""The cases of tests/test_xsec_cpu.py and tests/test_xsec_kernel.py: the cross-section kernel (xsec_kernel.hip) against the oracle's
MONORTM_XSEC_SUB, cell by cell, with the oracle's trace of every walk (orc_xsec_trace) to say what a cell exercised.

A helper module like tests/continuum_cases.py (no fixture, no test).  Nothing here runs on a GPU or reads a file: the tables are
xsec.XsTables built in memory, handed to MonoRTM.set_xsec and to the oracle alike, so both see the same bits.

One table set, one list of channels, three profiles.  Regions (molecule: name [header range] delvx, what it is there for):
  CCL4  t3     [780, 786]     0.0125  three temperatures; the layers of profile 0 sit below / at the coldest, inside a bracket, at the
                                      middle, at the warmest and above the warmest table temperature
        edge   [790, 794]     0.0125  channels exactly at v1x, at v1x + 1e-9, just inside both ends, exactly at v2x
  F11   d1     [800, 805]     0.0125  two disjoint regions of one molecule ...
        d2     [812, 817]     0.015
        one    [830, 836]     0.015   ... and one with a single temperature
  F12   ov1    [850, 856]     0.0125  two regions that overlap on [855.5, 856]: three channels get both
        ov2    [855.5, 861.5] 0.0125
        pad    [880, 886]     0.015   FSCDXS bounds [878.5, 887.5]: channels inside the header range, between the two pairs of bounds,
                                      within 1 cm-1 outside the FSCDXS bounds, exactly at v1fx - 1
        skip   [900, 904]     0.02    no channel within 1 cm-1 of it, channels on either side: never processed
  HNO3  wide   [920, 960]     0.02    60 channels 0.618... apart over a band with far wings: walks that end by the criterion deep inside
                                      the data, some after thousands of trips
  N2O5  neg    [980, 990]     0.0125  every 97th sample negative (measured files have them): the criterion is met at once there
        ragged [1000, 1008]   0.0125  the first (coldest) file is 160 points short: zeros from 1006 on, cold layers, channels in the tail
No region is finer than 0.0125 cm-1: thr = 1e-6 x step / hwb must stay above 1e-7 at 1000 mb, where hwb is 0.09 cm-1.

Layers of profile 0: 1000 mb down to 0.5 mb.  High pressure: walk with the step clipped to delvx; middle: step = 0.25 hwb; below the
pressure of the measurements (7 .. 90 mb): the linear branch.  Profiles 1 and 2 (4 and 7 layers) make the batch ragged.

Calls: one per molecule with every other molecule's column at zero (a cell is then ONE molecule's sum), and one with all five at
random amounts.  real_kind = 4 sees P, T and XAMNT rounded to float32; the oracle is then given those values.
"""
from __future__ import annotations

import dataclasses
import types

import numpy as np

from monortm_amd import synth, xsec

NAMES = ["CCL4", "F11", "F12", "HNO3", "N2O5"]
TOL_DBL = 1e-9             # a walk that stops one trip off moves its cell by >= min thr >= 1e-7; reordered sums and contracted
                           # multiply-adds over <= 4e4 terms are estimated at 1e-12
TOL_SGL = 2.0 ** -23       # the one rounding of the store (a float32 ulp is at most 2^-23 of the value)
TOL_SUM = 1e-12            # O = ... + ODXSEC + ... (modm.f90:268), of O
MIN_CRIT, MIN_IDX, MIN_NPTS, MIN_THR, MIN_SW = 1e-8, 1e-6, 1e-9, 1e-7, 1e-6
NEG_EVERY, NEG_AT = 97, 48
RAGGED_SHORT = 160

#        molecule, name, v1, v2, delvx, [(T, pressure of the measurement in mb)], band centre, width, peak, (FSCDXS pad below, above)
_SPEC = [(0, "t3", 780.0, 786.0, 0.0125, [(210.0, 7.0), (250.0, 25.0), (295.0, 70.0)], 783.4, 1.1, 5e-18, (0., 0.)),
         (0, "edge", 790.0, 794.0, 0.0125, [(220.0, 10.0), (290.0, 40.0)], 792.3, 0.9, 4e-18, (0., 0.)),
         (1, "d1", 800.0, 805.0, 0.0125, [(216.0, 30.0), (296.0, 90.0)], 802.1, 1.0, 4e-18, (0., 0.)),
         (1, "d2", 812.0, 817.0, 0.015, [(216.0, 20.0), (296.0, 50.0)], 815.2, 1.3, 2e-18, (0., 0.)),
         (1, "one", 830.0, 836.0, 0.015, [(270.0, 20.0)], 833.3, 1.2, 3e-18, (0., 0.)),
         (2, "ov1", 850.0, 856.0, 0.0125, [(230.0, 12.0), (290.0, 35.0)], 853.9, 1.2, 3e-18, (0., 0.)),
         (2, "ov2", 855.5, 861.5, 0.0125, [(230.0, 15.0), (290.0, 45.0)], 857.6, 1.4, 2e-18, (0., 0.)),
         (2, "pad", 880.0, 886.0, 0.015, [(225.0, 9.0), (295.0, 30.0)], 883.2, 1.1, 4e-18, (1.5, 1.5)),
         (2, "skip", 900.0, 904.0, 0.02, [(225.0, 9.0), (295.0, 30.0)], 902.0, 0.8, 4e-18, (0., 0.)),
         (3, "wide", 920.0, 960.0, 0.02, [(208.0, 5.0), (253.0, 20.0), (297.0, 60.0)], 941.0, 4.0, 5e-18, (0., 0.)),
         (4, "neg", 980.0, 990.0, 0.0125, [(215.0, 8.0), (293.0, 28.0)], 985.5, 1.9, 3e-18, (0., 0.)),
         (4, "ragged", 1000.0, 1008.0, 0.0125, [(222.0, 6.0), (290.0, 24.0)], 1004.4, 1.6, 3e-18, (0., 0.))]
REGION_NAMES = [s[1] for s in _SPEC]

_GOLD = 0.6180339887
_CHANNELS = {
    "t3": [780.4137, 781.2893, 782.6071, 783.3519, 784.7743, 785.6317],
    "edge": [790.0, 790.0 + 1e-9, 790.0031, 790.9137, 792.4877, 793.9969, 794.0],
    "d1": [800.7171, 802.3391, 804.1573],
    "d2": [812.9113, 814.4471, 816.2039],
    "one": [830.8571, 832.4093, 833.9737, 835.2219],
    "ov": [851.3137, 853.7291, 855.1173, 855.6211, 855.7603, 855.9341, 857.2719, 859.8113, 860.9377],
    "pad": [877.5, 877.9171, 879.2173, 881.4391, 883.6617, 885.1939, 886.7411, 888.1313],
    "skip": [898.7319, 905.3127],
    "wide": list(921.1371 + _GOLD * np.arange(60)),
    "neg": list(980.6113 + 0.97 * _GOLD * np.arange(15)) + [981.4553, 983.3947, 986.3041, 987.2759],
    "ragged": [1001.3171, 1003.9253, 1005.4419, 1006.5137, 1007.2861, 1007.8433],
}
WN = np.array(sorted(v for vs in _CHANNELS.values() for v in vs))

#           P [mb], T [K] - profile 0: the pressure sweep, and every position against the temperatures of t3 (210, 250, 295)
#           (no layer at the pressure of a measurement: hwb would be zero there, and the step with it)
_LAYERS = [[(1000.0, 296.3), (700.0, 295.0), (400.0, 271.7), (250.0, 250.0), (150.0, 230.4), (88.0, 210.0), (47.0, 204.6),
            (18.5, 221.3), (4.5, 240.9), (0.5, 262.2)],
           [(850.0, 288.4), (300.0, 243.1), (57.0, 216.0), (11.0, 228.7)],
           [(950.0, 291.9), (520.0, 270.0), (200.0, 222.0), (110.0, 207.3), (34.3, 215.2), (8.2, 233.6), (2.0, 219.4)]]
NLAYS = tuple(len(x) for x in _LAYERS)


def region(name: str) -> int:
    return REGION_NAMES.index(name)


def _band(v, centre, width, peak):
    x = (v - centre) / width
    return peak * (np.exp(-x * x) * (1 + 0.3 * np.sin(37 * x) + 0.2 * np.cos(11 * x)) + 0.02)


def tables() -> xsec.XsTables:
    """The table set: smooth bands with fine structure (the recipe of xsec.synthetic_library), in memory."""
    rng = np.random.default_rng(20261019)
    tabs = xsec.XsTables(names=list(NAMES), regions=[[] for _ in NAMES])
    for mol, name, v1, v2, dv, tps, c, w, pk, pad in _SPEC:
        npts = int(round((v2 - v1) / dv)) + 1
        v = v1 + dv * np.arange(npts)
        data = []
        for k, (tt, _) in enumerate(tps):
            shape = _band(v, c, w * (tt / 296.0) ** 0.5, pk * (296.0 / tt) ** 0.7) * (1 + 0.05 * rng.standard_normal(npts).cumsum() / np.sqrt(npts))
            vals = np.maximum(shape, pk * 1e-3)
            if name == "neg":
                vals[NEG_AT::NEG_EVERY] *= -0.6
            if name == "ragged" and k == 0:
                vals = vals[: npts - RAGGED_SHORT]
            data.append(vals)
        mass = xsec.XS_SPECIES[xsec.species_index(NAMES[mol])][1]
        xdop = 3.58115E-07 * (0.5 * (v1 + v2)) * np.sqrt(296.0 / mass)
        tabs.regions[mol].append(xsec.XsRegion(v1 - pad[0], v2 + pad[1], np.array([t for t, _ in tps]), np.array([p for _, p in tps]),
                                               data, float(xdop), v1, v2, npts))
    return tabs


def _profile(i: int) -> synth.Profile:
    p, t = (np.array(x) for x in zip(*_LAYERS[i]))
    air = 2.1e22 * p                                   # a column of air per layer, molecules / cm^2
    vmr = np.array([0.004, 4e-4, 3e-7, 3.2e-7, 1.5e-7, 1.7e-6, 0.209])
    tz = np.concatenate(([t[0] + 1.5], 0.5 * (t[:-1] + t[1:]), [t[-1] - 1.5]))
    return synth.Profile(wn=WN, p=p, t=t, tz=tz, wkl=air[:, None] * vmr[None, :], wbrodl=0.781 * air, clw=np.zeros(len(p)),
                         xs_names=list(NAMES), xamnt=np.zeros((len(p), len(NAMES))))


def calls() -> list:
    """[(label, [profile 0, 1, 2])]: `only<m>` with the column of molecule m alone, `all` with the five at random amounts.  The
    states (P, T) are the same in every call."""
    rng = np.random.default_rng(77)
    base = [_profile(i) for i in range(len(_LAYERS))]
    amounts = [1e15 * np.sqrt(pr.p / 1000.0)[:, None] * rng.uniform(0.5, 2.0, (pr.nlay, len(NAMES))) for pr in base]
    out = []
    for m in range(len(NAMES)):
        onehot = np.zeros(len(NAMES))
        onehot[m] = 1.0
        out.append((f"only{m}", [dataclasses.replace(pr, xamnt=a * onehot) for pr, a in zip(base, amounts)]))
    out.append(("all", [dataclasses.replace(pr, xamnt=a.copy()) for pr, a in zip(base, amounts)]))
    return out


def to_f32(pr: synth.Profile) -> synth.Profile:
    """The profile a real_kind = 4 context sees: every REAL input rounded to float32 (and widened again, for the oracle)."""
    r = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    return dataclasses.replace(pr, p=r(pr.p), t=r(pr.t), tz=r(pr.tz), wkl=r(pr.wkl), wbrodl=r(pr.wbrodl), clw=r(pr.clw),
                               emiss=r(pr.emiss), reflc=r(pr.reflc), tmpsfc=float(np.float32(pr.tmpsfc)), xamnt=r(pr.xamnt))


_ORACLE = {}


def oracle(kind: int = 8) -> types.SimpleNamespace:
    """The oracle on every call and profile, computed once per process: .odx[label][profile] = ODXSEC [nlay, nwn],
    .trace[profile] (the walks do not depend on the amounts), .profs[label] the profiles as the context of `kind` sees them,
    .seconds the time all of it took."""
    if kind in _ORACLE:
        return _ORACLE[kind]
    import time
    from concurrent.futures import ThreadPoolExecutor

    from oracle import pyoracle

    tabs = tables()
    t0 = time.perf_counter()
    res = types.SimpleNamespace(tabs=tabs, odx={}, trace=None, profs={}, seconds=0.0)
    for label, profs in calls():
        if kind == 4:
            profs = [to_f32(p) for p in profs]
        res.profs[label] = profs
    jobs = [(label, i) for label, profs in res.profs.items() for i in range(len(profs))]

    def job(j):
        p = res.profs[j[0]][j[1]]
        return pyoracle.xsec_trace(WN, p.p, p.t, tabs, p.xamnt, trace=(j[0] == "all"))

    with ThreadPoolExecutor(max_workers=6) as pool:          # (the library call releases the interpreter lock)
        runs = dict(zip(jobs, pool.map(job, jobs)))
    for label, profs in res.profs.items():
        res.odx[label] = [runs[label, i][0] for i in range(len(profs))]
    res.trace = [runs["all", i][1] for i in range(len(res.profs["all"]))]
    res.seconds = time.perf_counter() - t0
    _ORACLE[kind] = res
    return res

