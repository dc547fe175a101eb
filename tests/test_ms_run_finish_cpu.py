"""The fixtures of tests/ms_finish_cases.py on the CPU: each has the shape its case is about, and the FORM of the host identity that
tests/test_ms_run_finish.py holds the GPU to bit for bit - total = line sums in molecule order + continuum + cloud - holds for the
oracle's own arrays (the oracle adds in its own order and rounding, so to a few ulp there, not to the bit)."""
import numpy as np
import pytest

import ms_finish_cases as mc
from monortm_amd import tape3


@pytest.fixture(scope="module")
def built():
    return {k: f() for k, f in mc.CASES.items()}


def test_shapes(built):
    rec, profs = built["ragged"]
    assert profs[0].nwn == 33 and len(profs) == 11 and sorted({p.nlay for p in profs}) == [2, 3, 5]
    rec, profs = built["long_runs"]
    mol = rec.mol % 100
    assert 140 <= int((mol == 1).sum()) <= 150 and all(8 <= int((mol == m).sum()) <= 12 for m in (2, 3, 4, 7))
    rec, profs = built["columns_a"]
    mol = rec.mol % 100
    hi = max(p.wn[-1] for p in profs)
    assert rec.vnu[mol == 4].min() > hi + 25.0 + 1.0 and (mol == 1).any()   # N2O: beyond every channel's 25 cm-1
    assert not profs[2].wkl[:, 0].any() and profs[1].wkl[:, 0].all()
    rec, profs = built["columns_b"]
    assert not ((rec.mol % 100) == 1).any() and ((rec.mol % 100) == 2).any()
    rec, profs = built["rare_shapes"]
    assert len(profs) == 7 and profs[0].nlay == 6 and profs[0].p[-1] < 0.05 and (rec.iflg == 1).any()
    rec, profs = built["species_broadening"]
    assert len(profs) == 7 and profs[0].nlay == 4 and all(p.ibrd == 1 for p in profs) and rec.brd_flg.any()


@pytest.mark.parametrize("name", list(mc.CASES))
def test_identity_form_on_the_oracle(name, built, workdir):
    from oracle.pyoracle import Oracle

    rec, profs = built[name]
    t3 = f"{workdir}/TAPE3_msfin_cpu_{name}"
    tape3.write_tape3(t3, rec)
    orc = Oracle(t3, profs[0].wn[0], profs[0].wn[-1])
    if name == "rare_shapes":
        orc.census(reset=True)
    for p in profs[:3]:
        d = orc.run(p)
        o, h = np.asarray(d.o, np.float64), mc.host_total(d)
        assert np.isfinite(o).all() and (o > 0).all()
        assert np.max(np.abs(o - h) / o) <= 8 * np.finfo(np.float64).eps
    if name == "rare_shapes":
        assert orc.census()["voigt"] > 0   # (the Voigt branch is live at six layers too)
    if name == "columns_a":
        d = orc.run(profs[2])
        assert not d.o_by_mol[:, 0, :].any() and not d.o_by_mol[:, 3, :].any() and d.o_by_mol[:, 2, :].any()
    orc.close()
