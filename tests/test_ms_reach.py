"""The slot masks, the dense word and the Voigt shortcut of lines_ms_kernel on the GPU: the constructed cases of tests/ms_reach_cases.py,
forced with `lines_kernel = ms`, against the oracle and against lines_kernel.  tests/test_ms_reach_cpu.py shows on the CPU that a mask
bit missing for any claimed line moves a named cell of O_BY_MOL by at least 1e-4 of itself; here that cell is held at 1e-6.

Per (list, channel set, batch):
    oracle          compare() at RTOL = 1e-6; per_molecule_errors() <= RTOL (no floor from the layer total: it sees an edge line);
                    the named cell of every claimed line within RTOL of the oracle's value
    lines_kernel    the existing 1e-11 between the two line kernels, every profile
    the kernel ran  over the module, lines_ms_kernel's sums differ from lines_kernel's in the last bits
The pattern lists run with ms_items = 64 and 192 (chunks of 9 or 10 and of 21 or 32 lines: the chunk boundaries cut the groups
differently).  The Voigt list: the oracle's census counts Voigt evaluations on the batch.  The NaN batch: the wave-mates of the
profile with the NaN pressure as everywhere else, that profile with the oracle's NaN positions.
"""
import dataclasses

import numpy as np
import pytest

import ms_reach_cases as mr
from common import RTOL, compare, compare_nan_aware, per_molecule_errors
from monortm_amd import api
from test_ms_kernel import _close

pytestmark = pytest.mark.gpu

_DIFFERS = {"n": 0, "runs": 0}
RUNS = mr.runs()


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


def _run(t3, profs, kernel, ms_items=None):
    wn = profs[0].wn
    rt = api.MonoRTM(t3, wn[0], wn[-1])
    rt.set_option("lines_kernel", kernel)
    if ms_items is not None:
        rt.set_option("ms_items", ms_items)
    got = rt.run(profs)
    rt.close()
    return got


def _one(workdir, key, ms_items=None):
    from oracle.pyoracle import Oracle

    ll, kind = RUNS[key]
    wn = ll.wn
    profs = mr.batch(kind, wn)
    t3 = mr.write(ll, workdir)
    cells = mr.named_cells(ll, kind, workdir) if kind != "nan" else {}
    ms = _run(t3, profs, "ms", ms_items)
    ref = _run(t3, profs, "wn")
    orc = Oracle(t3, wn[0], wn[-1])
    orc.census(reset=True)
    for i, pr in enumerate(profs):
        what = f"{key} profile {i}" + ("" if ms_items is None else f" ms_items {ms_items}")
        exp = orc.run(pr)
        if np.isnan(pr.p).any():
            compare_nan_aware(ms[i], exp, rtol=RTOL, what=what)
            continue
        # (a channel that no line reaches has no optical depth at all - cntnm = 0 - and the oracle's TMR is 0 / 0 there: the same
        # positions must be NaN here, everything else is compared as usual)
        assert not any(np.isnan(np.asarray(getattr(exp, f))).any() for f in ("o", "o_by_mol", "rad", "tb", "trtot", "rup", "rdn")), what
        errs = (compare_nan_aware if np.isnan(exp.tmr).any() else compare)(ms[i], exp, rtol=RTOL, what=what)
        pm = per_molecule_errors(ms[i], exp)
        print(f"{what}: o_by_mol {errs['o_by_mol']:.2e} tb {errs['tb']:.2e} per molecule {np.max(pm[~np.isnan(pm)], initial=0.0):.2e}")
        assert not (pm > RTOL).any(), f"{what}: per-molecule errors {pm}"
        for c, (prof, lay, m, ch, rel, val) in cells.items():
            if prof != i:
                continue
            g, e = float(ms[i].o_by_mol[lay, m, ch]), float(exp.o_by_mol[lay, m, ch])
            l = ll.lines[c]
            print(f"{what}: cell of the {l.role} line of slot {l.slot} ({l.side}): {abs(g - e) / abs(e):.2e} (the line is {rel:.2e} of it)")
            assert e == val and abs(g - e) <= RTOL * abs(e), (f"{what}: layer {lay} molecule {m + 1} channel {ch}: {g:.17g}, oracle {e:.17g} - the cell of the {l.role} line "
                                                              f"at {l.vnu:.3f} cm-1 (slot {l.slot}, {l.side}), which is {rel:.2e} of it")
        nan = np.isnan(exp.tmr)   # (the same NaN positions in both kernels - they are the oracle's, asserted above for ms - then the 1e-11)
        assert np.array_equal(np.isnan(ref[i].tmr), nan), what
        _close(dataclasses.replace(ms[i], tmr=np.where(nan, 0.0, ms[i].tmr)), dataclasses.replace(ref[i], tmr=np.where(nan, 0.0, ref[i].tmr)), what)
        _DIFFERS["n"] += int(not np.array_equal(ms[i].o_by_mol, ref[i].o_by_mol))
    _DIFFERS["runs"] += 1
    census = orc.census()
    orc.close()
    return census


@pytest.mark.parametrize("key", [k for k in RUNS if not k.startswith(("patterns", "voigt")) and not k.endswith("-nan")])
def test_edges_of_the_slots(workdir, gpu, key):
    """hi / lo / neg x dense / mask on every channel set: the dense lines need the dense word (a state of RHORAT 5.84 beside ordinary
    ones in the wave; and the candidate window's max(RHORAT, 1) at the tile's own ends), the mask lines the margin of the words."""
    _one(workdir, key)


@pytest.mark.parametrize("ms_items", [64, 192])
@pytest.mark.parametrize("key", [k for k in RUNS if k.startswith("patterns")])
def test_patterns_through_the_groups(workdir, gpu, key, ms_items):
    """A lone reaching line at every position of the groups of four, the pairs and the single lines, in both chunkings."""
    _one(workdir, key, ms_items)


def test_voigt_candidate_by_its_shift(workdir, gpu):
    """The shift brings a channel within 100 Doppler widths: the near_lb shortcut must still search (1e-6 against the oracle, whose
    census shows that the case does evaluate Voigt shapes)."""
    (key,) = [k for k in RUNS if k.startswith("voigt")]
    census = _one(workdir, key)
    assert census["voigt"] > 0


@pytest.mark.parametrize("key", [k for k in RUNS if k.endswith("-nan")])
def test_nan_state_in_a_wave(workdir, gpu, key):
    """A NaN pressure in one state makes its wave dense (no masks); its wave-mates are held as everywhere else."""
    _one(workdir, key)


def test_zz_the_forced_kernel_ran(gpu):
    if _DIFFERS["runs"]:
        assert _DIFFERS["n"] > 0, "lines_ms_kernel returned lines_kernel's bits everywhere: was it launched?"
