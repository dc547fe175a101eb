"""The cases, the error measure and the census of tests/test_continuum_cpu.py and tests/test_finish_kernels.py: the continuum, cloud
and total optical depths of MODM (continuum_kernel.hip), slot by slot and launch variant by launch variant.

A helper module like tests/rtm_truth.py (no fixture, no test).  Nothing here runs on a GPU or loads the product's library; the
pure-Python input builders monortm_amd.synth / monortm_amd.tape3 are all it takes from the package.

Line file: the 1672 bytes that a TAPE3 holds ahead of its first line block (as test_edge_empty_line_list_and_wide_grid cuts them).
Without lines O_BY_MOL is zero, and O, OC and O_CLW are the work of the finish kernel alone.

Launch variants (modm_plan.hpp, restated in variant()): `mw` finish_mw_kernel, `high` finish_kernel<HIGH>, `par` <PAR>, `q4` <Q4>, `plain64` /
`plain256` finish_kernel with 64 / 256 threads.  A case names the variant every one of its runs must reach; the GPU test asserts it
with monortm_hip_counter.

Calls.  The continuum factors XSELF .. XRAYL are arguments of a MODM CALL, not of a profile, so a run is a series of calls over the same
batch of profiles:
  main      seeded factors in (0.3, 1.7), liquid cloud in every second profile, irt 1 / 3 mixed
  only0..6  factor k alone (cntnm = e_k), no cloud: O is then that ONE term.  This is how the Rayleigh term (added into O only,
            ~1e-11 of O in the 10 micron window beside the others) and every addend of O's sum are seen with plain conditioning, and
            how every factor is zero in some call (the kernels store the zeros of a dead pass directly).
Profile i of a run is synth.perturbed_profile(seed of the case * 1000 + i, ...): every (profile, layer) state differs.

Range restriction: no run mixes a channel below 3 cm-1 with one at or above 820 (the reference's Rayleigh term over its radiation
term returns NaN there: tests/test_fuzz_gpu.py, seed 50269).
"""
from __future__ import annotations

import dataclasses
import math
import os

import numpy as np

from monortm_amd import synth, tape3

VARIANTS = ("mw", "high", "par", "q4", "plain64", "plain256")     # the order of monortm_hip_counter 2 .. 7
NFAC = 7                                                           # XSELF, XFRGN, XCO2C, XO3CN, XO2CN, XN2CN, XRAYL
SLOT_OF_FACTOR = (0, 0, 1, 2, 3, 4, None)                          # slot of OC a factor feeds; Rayleigh goes into O alone
E_FLOOR = 1e-4                                                     # of a row's peak: limits the relative measure, excludes no cell
TOL_DBL = 1e-10
TOL_SGL = 2.0 ** -23
TOL_CLW = 1e-12                                                    # ODCLW_TKC of tests/test_function_kat.py


def header_only_tape3(path: str) -> str:
    """A TAPE3 that ends ahead of its first block of lines."""
    tmp = path + ".tmp10"
    tape3.write_tape3(tmp, synth.synthetic_lines(10))
    with open(tmp, "rb") as f:
        head = f.read()[: 1664 + 8]
    os.remove(tmp)
    with open(path, "wb") as f:
        f.write(head)
    return path


def nptabs(v1: float, v2: float) -> int:
    """Width of the 1 cm-1 ABSRB grid of a call whose first / last wavenumbers are v1 / v2 (modm.f90:180-185)."""
    v1abs = int(v1) - 3.0
    v2abs = int(v2 + 3.0 + 0.5)
    return int((v2abs - v1abs) / 1.0 + 1.5)


def variant(wn: np.ndarray, nprof: int, nlay_max: int, cus: int, generic: bool = False) -> str:
    """The launch variant a call takes: the rule of modm_plan.hpp, restated from its description, so that the case table can be checked
    on a machine without a GPU for any count of compute units."""
    npt, nwn, last = nptabs(wn[0], wn[-1]), len(wn), float(wn[-1])
    if last < 820.0 and npt <= 1000 and not generic:
        return "mw"
    if last > 1340.0:
        return "high"
    if nprof * nlay_max < 16 * cus:
        return "par"
    if npt <= 64 and nwn <= 128:
        return "q4"
    return "plain64" if (npt <= 256 and nwn <= 128) else "plain256"


def alive(k: int, v1: float, v2: float) -> bool:
    """Whether the term of factor k can be non-zero for channels in [v1, v2] (the spectral tests of CONTNM, contnm.f90)."""
    if k in (0, 1):
        return v2 > -20.0 and v1 < 20000.0
    if k == 2:
        return v2 > -20.0 and v1 < 10000.0
    if k == 3:
        return v2 > 8920.0 and v1 < 54000.0
    if k == 4:
        return v2 > 1340.0
    if k == 5:
        return (v2 > -10.0 and v1 < 350.0) or (v2 > 2001.77 and v1 < 4910.0)
    return v2 >= 820.0


@dataclasses.dataclass
class Run:
    label: str
    wn: np.ndarray
    expect: str                  # the variant this run must count
    dvset: float = 0.0
    generic: bool = False        # set_option("finish", "generic")


@dataclasses.dataclass
class Case:
    name: str
    seed: int
    runs: list
    nlays: tuple                 # layers per profile, cycling
    nprof: int | None = None     # None: enough (profile, layer) workgroups to leave <PAR> behind, from the device's compute units

    def nprofiles(self, cus: int) -> int:
        return self.nprof if self.nprof is not None else math.ceil(16 * cus / max(self.nlays)) + 2

    def nlay_of(self, i: int) -> int:
        return self.nlays[i % len(self.nlays)]


def _rand(seed: int, n: int, lo: float, hi: float) -> np.ndarray:
    return np.sort(np.random.default_rng(seed).uniform(lo, hi, n))


def _last_wn_for_nptabs(first: float, want: int) -> float:
    """The last wavenumber that makes the ABSRB grid `want` points wide: V2ABS = int(v2 + 3.5) = V1ABS + want - 1."""
    v2 = (int(first) - 3.0) + want - 1 - 3.5 + 0.25
    assert nptabs(first, v2) == want
    return v2


def _cases() -> list:
    q4_wn = _rand(11, 37, 900.0, 950.0)
    e820 = _rand(17, 30, 700.0, 819.0)
    hi = _rand(23, 30, 1250.0, 1339.0)
    n2 = _rand(19, 64, 351.0, 420.0)
    mw = {n: _rand(100 + n, n, 0.05, 300.0) for n in (64, 65, 128, 129, 256, 257)}
    between = _rand(29, 200, 6.0, 990.0)
    last1000, last1001 = _last_wn_for_nptabs(5.5, 1000), _last_wn_for_nptabs(5.5, 1001)
    return [
        Case("q4_ragged", 1, [Run("", q4_wn, "q4")], (63, 62, 61, 17, 1)),        # nlay_max 63: the last workgroup serves three layers
        Case("q4_grid", 2, [Run("", 900.0 + 0.4 * np.arange(128), "q4", dvset=0.4)], (63, 5)),
        Case("plain64", 3, [Run("", _rand(13, 100, 830.0, 1050.0), "plain64")], (63, 40)),
        Case("plain256_wide", 4, [Run("", _rand(14, 100, 825.0, 1335.0), "plain256")], (63, 40)),
        Case("plain256_nwn", 5, [Run("", _rand(15, 129, 900.0, 950.0), "plain256")], (63, 40)),
        Case("par", 6, [Run("", q4_wn, "par")], (20, 7), nprof=3),
        Case("edge820", 7, [Run("819.99", np.append(e820, 819.99), "mw"), Run("820.0", np.append(e820, 820.0), "par")], (20,), nprof=3),
        # The rule reads "last wavenumber < 820 AND NPTABS <= 1000".  With a first wavenumber >= 0 the grid of a range that ends
        # below 820 is at most 827 points wide, so the second clause never decides: both widths end near 998 cm-1 and take <PAR>, with
        # four sets of a 1000- / 1001-point grid in LDS.  The third run is the widest grid finish_mw_kernel can meet from 5.5 cm-1.
        Case("nptabs", 8, [Run("1000", np.concatenate(([5.5], between, [last1000])), "par"),
                           Run("1001", np.concatenate(([5.5], between, [last1001])), "par"),
                           Run("widest_mw", np.concatenate(([5.5], between[between < 819.0], [819.99])), "mw")], (12,), nprof=2),
        Case("n2_edge", 9, [Run(str(f), np.concatenate(([f], n2)), "mw") for f in (349.9, 350.0, 350.5)], (20,), nprof=3),
        Case("frgn600", 10, [Run("", _rand(16, 257, 560.0, 640.0), "mw")], (5,), nprof=3),       # FSCAL: table up to 600, closed form above
        Case("mw_chunks", 11, [Run(str(n), mw[n], "mw") for n in (64, 65, 128, 129, 256, 257)]
             + [Run("grid", 0.05 + 2.3 * np.arange(129), "mw", dvset=2.3)], (9, 4), nprof=3),
        Case("mw_generic", 11, [Run(str(n), mw[n], "par", generic=True) for n in (64, 257)], (9, 4), nprof=3),   # = mw_chunks' inputs
        Case("high_edge", 12, [Run("1340.0", np.append(hi, 1340.0), "par"), Run("1340.5", np.append(hi, 1340.5), "high")], (20, 7), nprof=5),
    ]


CASES = {c.name: c for c in _cases()}
SGL_CASES = (("q4_ragged", ""), ("plain64", ""), ("edge820", "819.99"), ("edge820", "820.0"), ("mw_chunks", "65"))


def main_factors(case: Case) -> np.ndarray:
    return np.random.default_rng(7000 + case.seed).uniform(0.3, 1.7, NFAC)


def profiles(case: Case, run: Run, nprof: int, first: int = 0) -> list:
    """Profiles first .. first + nprof - 1 of the run's batch with the main call's factors."""
    fac = main_factors(case)
    out = []
    for i in range(first, first + nprof):
        pr = synth.perturbed_profile(case.seed * 1000 + i, run.wn, nlay=case.nlay_of(i), cloud=(i % 2 == 0), irt=(1 if i % 3 == 0 else 3))
        pr.dvset = run.dvset
        pr.cntnm = fac.copy()
        out.append(pr)
    return out


def calls(profs: list) -> list:
    """[(label, profiles)]: the main call and the seven one-factor calls (cntnm = e_k, no cloud) over the same states."""
    out = [("main", profs)]
    for k in range(NFAC):
        e = np.zeros(NFAC)
        e[k] = 1.0
        out.append((f"only{k}", [dataclasses.replace(p, cntnm=e.copy(), clw=np.zeros_like(p.clw)) for p in profs]))
    return out


def to_f32(pr):
    """The profile a real_kind = 4 context sees: every REAL input rounded to float32 (and widened again, for the oracle)."""
    r = lambda a: None if a is None else np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    return dataclasses.replace(pr, p=r(pr.p), t=r(pr.t), tz=r(pr.tz), wkl=r(pr.wkl), wbrodl=r(pr.wbrodl), clw=r(pr.clw),
                               emiss=r(pr.emiss), reflc=r(pr.reflc), tmpsfc=float(np.float32(pr.tmpsfc)))


def E(got, exp) -> float:
    """max over rows (the last axis: channels) of max |got - exp| / max(|exp|, 1e-4 x the row's peak of |exp|).  A row whose exp is all
    zero must be exactly zero in got; anything else - a NaN included - is inf."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    if exp.size == 0:
        return 0.0
    den = np.maximum(np.abs(exp), E_FLOOR * np.abs(exp).max(axis=-1, keepdims=True))
    diff = np.abs(got - exp)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, diff / den, np.where(diff == 0, 0.0, np.inf))
    r = np.where(np.isfinite(got) & np.isfinite(exp), r, np.inf)
    return float(r.max())


def under_floor(exp) -> float:
    """Share of the cells of non-zero rows that lie under the floor of E."""
    exp = np.abs(np.asarray(exp, np.float64))
    pk = exp.max(axis=-1, keepdims=True)
    live = np.broadcast_to(pk > 0, exp.shape)
    return float((exp < E_FLOOR * pk)[live].mean()) if live.any() else 0.0


def census(run: Run, dumps: dict) -> None:
    """dumps: call label -> [oracle Dump per profile].  Asserts what the cases are there for: everything finite; in the call of a
    factor that the range makes alive some profile has a non-zero peak in that factor's slot (O itself for Rayleigh) and nothing
    anywhere else; a dead factor leaves exact zeros; the main call's factors are all switched on and it holds a cloud."""
    v1, v2 = float(run.wn[0]), float(run.wn[-1])
    assert not (v1 < 3.0 and v2 >= 820.0), "range restriction: the reference returns NaN here"
    for label, ds in dumps.items():
        for d in ds:
            assert all(np.isfinite(getattr(d, f)).all() for f in ("o", "oc", "o_clw", "rad", "tb")), (run.label, label)
            assert not np.asarray(d.o_by_mol).any(), "the line file holds lines"
    for k in range(NFAC):
        ds, slot = dumps[f"only{k}"], SLOT_OF_FACTOR[k]
        peak = max(float(np.abs(d.o).max()) for d in ds)
        assert (peak > 0) == alive(k, v1, v2), f"run {run.label}: factor {k} alive = {alive(k, v1, v2)} but the peak of its term is {peak:g}"
        for d in ds:
            assert not d.o_clw.any()
            other = np.delete(d.oc, slot, axis=1) if slot is not None else d.oc
            assert not other.any(), f"factor {k} alone fills another slot"
    main = dumps["main"]
    assert any(d.o_clw.any() for d in main) and any(not d.o_clw.any() for d in main)
    for s in range(5):
        want = any(alive(k, v1, v2) for k in range(NFAC) if SLOT_OF_FACTOR[k] == s)
        assert any(np.abs(d.oc[:, s]).max() > 0 for d in main) == want, (run.label, s)
