"""What entitles tests/test_finish_kernels.py to its reference and its cases, checked without a GPU:
  - the CPU oracle's continuum and cloud optical depths equal the reference's own, slot by slot, under the error measure E of
    tests/continuum_cases.py (compare() of tests/common.py floors a slot at 1e-6 of the cell's TOTAL optical depth: beside lines a
    continuum slot can be wholly wrong and pass);
  - the cases are what they claim to be: every term the spectral range makes alive is non-zero somewhere, every factor is zero
    somewhere, everything is finite, and the case table names the launch variant that the dispatch rule gives.
"""
import numpy as np
import pytest

import continuum_cases as cc
from common import Golden, golden_names
from oracle.pyoracle import Oracle

# profiles of a big batch that the census looks at: profile i does not depend on the size of the batch, so what holds for the first
# few holds for the whole
CENSUS_PROFILES = 6


@pytest.fixture(scope="module")
def tape3_path(workdir):
    return cc.header_only_tape3(f"{workdir}/TAPE3_continuum_cpu")


def test_error_measure():
    exp = np.array([[1.0, 1e-6, 0.0], [0.0, 0.0, 0.0]])
    assert cc.E(exp, exp) == 0.0
    assert cc.E(exp + np.array([[0.0, 1e-8, 0.0], [0.0, 0.0, 0.0]]), exp) == pytest.approx(1e-4)      # under the floor: 1e-8 / 1e-4
    assert cc.E(exp + np.array([[1e-3, 0.0, 0.0], [0.0, 0.0, 0.0]]), exp) == pytest.approx(1e-3)
    assert cc.E(exp + np.array([[0.0, 0.0, 0.0], [0.0, 1e-300, 0.0]]), exp) == np.inf                  # a zero row must stay zero
    assert cc.E(np.where(exp == 1.0, np.nan, exp), exp) == np.inf
    assert cc.E(np.zeros((2, 0)), np.zeros((2, 0))) == 0.0
    assert cc.under_floor(exp) == pytest.approx(2 / 3)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case_census(name, tape3_path):
    case = cc.CASES[name]
    for run in case.runs:
        # (64 ... 304 compute units: whatever device runs the GPU tests, the batch is sized to reach the named variant)
        for cus in (64, 256, 304):
            n = case.nprofiles(cus)
            assert cc.variant(run.wn, n, max(case.nlays), cus, run.generic) == run.expect, (name, run.label, cus)
        assert np.all(np.diff(run.wn) > 0)
        n = min(case.nprofiles(256), CENSUS_PROFILES)
        profs = cc.profiles(case, run, n)
        assert {p.nlay for p in profs} == set(case.nlays[:n]) and {p.irt for p in profs} <= {1, 3}
        assert (cc.main_factors(case) > 0).all()
        orc = Oracle(tape3_path, run.wn[0], run.wn[-1])
        cc.census(run, {label: [orc.run(p) for p in ps] for label, ps in cc.calls(profs)})
        orc.close()


def test_every_variant_has_a_case():
    assert {r.expect for c in cc.CASES.values() for r in c.runs} == set(cc.VARIANTS)
    for name, label in cc.SGL_CASES:
        assert any(r.label == label for r in cc.CASES[name].runs)


def _has_xsec(g) -> bool:
    return any(p.xs_names for p in g.profiles)


def test_oracle_continuum_matches_reference_slot_by_slot(workdir):
    """Every double-precision fixture of the compiled reference without cross-sections: the oracle's OC (each of the five slots a row
    of its own per layer) and O_CLW within 1e-13 of the reference's under E.  Observed on the 42 fixture profiles: OC exactly equal in every slot, O_CLW 7.2e-15 at worst (cloud_updown)."""
    worst, n = 0.0, 0
    for name in golden_names():
        g = Golden(name, workdir)
        if _has_xsec(g):
            continue
        orc = Oracle(g.tape3, g.profiles[0].wn[0], g.profiles[0].wn[-1])
        for i, (pr, exp) in enumerate(zip(g.profiles, g.expected)):
            got = orc.run(pr)
            e_oc, e_clw = cc.E(got.oc, exp.oc), cc.E(got.o_clw, exp.o_clw)
            worst, n = max(worst, e_oc, e_clw), n + 1
            assert e_oc <= 1e-13 and e_clw <= 1e-13, f"{name}[{i}]: E(oc) = {e_oc:g}, E(o_clw) = {e_clw:g}"
        orc.close()
    print(f"oracle against the reference: {n} fixture profiles, worst E = {worst:g}")
    assert n >= 30
