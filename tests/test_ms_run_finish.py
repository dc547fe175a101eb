"""The end of a molecule run in lines_ms_kernel (monortm_amd/csrc/lines_ms_kernel.hip, the "run complete" block of the chunk loop):
the sums of the run come back from the walk in registers, the radiation terms and the sum over the molecules are fetched in one
round trip, selects form the products and only the stores are predicated.  The fixtures (tests/ms_finish_cases.py) are the smallest
batches at which that seam can go wrong; every one is held

  (a) to lines_kernel at the 1e-11 of tests/test_ms_kernel.py,
  (b) to the oracle at the tolerance of its batch fuzz (RTOL),
  (c) to a host identity that is exact: the total optical depth equals, bit for bit, the sequential float64 sum
      ((((sum of O_BY_MOL in molecule order) + 0.) + 0.) + soc) + od_clw that finish_mw_kernel forms from the kernel's sum over the
      molecules - which pins the order and the bits of that accumulation without a second build."""
import numpy as np
import pytest

import ms_finish_cases as mc
from common import RTOL, compare
from monortm_amd import api, tape3
from test_ms_kernel import _close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


def _run(t3, profs, kernel):
    rt = api.MonoRTM(t3, profs[0].wn[0], profs[0].wn[-1])
    rt.set_option("lines_kernel", kernel)
    out = rt.run(profs)
    rt.close()
    return out


@pytest.fixture(scope="module")
def results(workdir, gpu):
    """Per case, computed once: the profiles, lines_kernel's results, lines_ms_kernel's, the oracle's."""
    from oracle.pyoracle import Oracle

    cache = {}

    def get(name):
        if name not in cache:
            rec, profs = mc.CASES[name]()
            t3 = f"{workdir}/TAPE3_msfin_{name}"
            tape3.write_tape3(t3, rec)
            orc = Oracle(t3, profs[0].wn[0], profs[0].wn[-1])
            exp = [orc.run(p) for p in profs]
            orc.close()
            cache[name] = (t3, profs, _run(t3, profs, "wn"), _run(t3, profs, "ms"), exp)
        return cache[name]

    return get


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _three_checks(name, res):
    t3, profs, wn_out, ms_out, exp = res
    for i, p in enumerate(profs):
        what = f"{name} profile {i} (nlay {p.nlay})"
        _close(ms_out[i], wn_out[i], what)                                         # (a)
        compare(ms_out[i], exp[i], rtol=RTOL, what=f"ms vs oracle, {what}")        # (b)
        o = np.asarray(ms_out[i].o, np.float64)                                    # (c)
        assert o.shape == (p.nlay, p.nwn) and np.isfinite(o).all()
        h = mc.host_total(ms_out[i])
        bad = np.argwhere(_bits(o) != _bits(h))
        assert bad.size == 0, f"{what}: the total is not the sequential sum of its parts at (layer, channel) {bad[:4].tolist()}"
    # (the forced kernel really ran: its line sums differ from lines_kernel's in the last bits somewhere in the batch)
    assert any(not np.array_equal(a.o_by_mol, b.o_by_mol) for a, b in zip(ms_out, wn_out))


@pytest.mark.parametrize("name", ["ragged", "long_runs", "rare_shapes", "species_broadening"])
def test_run_finish(name, results):
    _three_checks(name, results(name))


def test_run_finish_columns(results):
    """A state without a column of the first molecule that has lines, a molecule whose lines all lie outside the window, and a batch
    whose sum over the molecules starts at molecule 2."""
    res = results("columns_a")
    _three_checks("columns_a", res)
    ms_out = res[3]
    assert not ms_out[2].o_by_mol[:, 0, :].any()                    # no H2O column: exactly zero ...
    assert all(ms_out[i].o_by_mol[:, 0, :].all() for i in (0, 1, 3, 4, 5, 6))   # ... while the other states of the wave sum
    assert ms_out[2].o_by_mol[:, 2, :].all()
    assert not any(d.o_by_mol[:, 3, :].any() for d in ms_out)       # N2O: never walked, zeroed by the prologue
    res = results("columns_b")
    _three_checks("columns_b", res)
    assert not any(d.o_by_mol[:, 0, :].any() for d in res[3]) and all(d.o_by_mol[:, 1, :].any() for d in res[3])


def test_run_finish_reproducible(results):
    t3, profs, _, first, _ = results("ragged")
    again = _run(t3, profs, "ms")
    for a, b in zip(first, again):
        for f in ("o", "o_by_mol", "rad", "tb"):
            assert np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))), f
