"""The fused prepare trip of lines_ms_kernel (ms_prepare_trip in monortm_amd/csrc/lines_ms_kernel.hip: a lane prepares its line
for all two or three states it serves in one straight trip) against the pass loop it replaces for plain chunks, and against the
oracle.  Option `ms_prepare` = "fused" (the default: the trip wherever it applies) / "passes" (the pass loop for every chunk) puts
both paths through the same inputs in one build; `lines_kernel = ms` forces the kernel onto these small batches.

The shapes are the smallest at which the trip can go wrong:
  ragged      7 profiles x 3 layers x 50 channels x the 500-line list: six states a wave in three passes' worth (one full group and a
              group of one profile), one profile of the full group with fewer layers (an inactive state in a wave), one state
              without a column of one molecule; 500 candidates = 15 chunks of 32 lines + a tail of 20 (lanes without a line)
  ns2_g8      9 profiles x 2 layers x 40 channels: eight states a wave in two passes' worth, and a group of one profile
  ns2_real    the real-file-like list (tests/golden/real_like.npz's file) through its 40 sounder channels, 7 profiles x 2 layers:
              seven states a wave, isotopologues 1-5, molecules beyond the seventh, coupled O2 pairs between plain chunks
  tail        a 333-line list on 40 channels: the last chunk holds 13 lines whatever the chunk length (333 = 13 mod 16, 21 and 32)
  special     bench.py's c2lc shape cut down to 7 profiles x its 4 top layers (model top 0.004 hPa, channels on line centres, every
              O2 line coupled): plain and non-plain chunks alternate, Voigt candidates make the trip hand chunks back
  nan         the ragged shape with a NaN temperature in one state: the reference stops in TIPS_2003 (no partition sum), and so
              must both paths (MONORTM_ETEMP) - the wave that holds the state has walked its prepare stage by then
  nan_column  the ragged shape with a NaN column amount in one state: the reference adds the NaN terms (modm.f90:384, :432), the
              state's widths are NaN and the trip hands its chunks back
(a) the two paths give identical bits in every output; (b) the fused run agrees with the oracle, profile by profile, at the
tolerance tests/test_ms_kernel.py uses for that comparison."""
import dataclasses

import numpy as np
import pytest

from common import FIELDS, RTOL, compare, compare_nan_aware
from monortm_amd import api, synth, tape3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


def _ragged(nan=None):
    rec = synth.synthetic_lines(500)
    wn = synth.c2_channels(50)
    profs = [synth.perturbed_profile(40 + i, wn, nlay=(2 if i == 2 else 3), cloud=(i == 5), irt=(1 if i == 1 else 3)) for i in range(7)]
    profs[4].wkl[1, 2] = 0.0   # no O3 in one state of the full group
    if nan == "t":
        profs[3].t[1] = np.nan
    if nan == "column":
        profs[3].wkl[1, 0] = np.nan
    return rec, {}, profs


def _ns2_g8():
    wn = synth.c2_channels(40)
    return synth.synthetic_lines(500), {}, [synth.perturbed_profile(60 + i, wn, nlay=2, irt=(1 if i % 4 == 0 else 3)) for i in range(9)]


def _ns2_real():
    rec, kw, _ = synth.real_like_file()
    wn = synth.sounder_channels()
    return rec, kw, [synth.perturbed_profile(80 + i, wn, nlay=2, ztop_km=60.0) for i in range(7)]


def _tail():
    rec = synth.synthetic_lines(333, seed=41)
    n = int((rec.iflg >= 0).sum())
    assert n == 333 and all(n % cl == 13 for cl in (16, 32)) and n % 21 != 0
    wn = synth.c2_channels(40, seed=9)
    return rec, {}, [synth.perturbed_profile(100 + i, wn, nlay=3) for i in range(7)]


def _special():
    import bench

    rec, profs, _, _, _ = bench.build_workload("c2lc", 0, 7)
    top = [dataclasses.replace(p, p=p.p[-4:], t=p.t[-4:], tz=p.tz[-5:], wkl=p.wkl[-4:], wbrodl=p.wbrodl[-4:], clw=p.clw[-4:]) for p in profs]
    return rec, {}, top


CASES = {"ragged": _ragged, "ns2_g8": _ns2_g8, "ns2_real": _ns2_real, "tail": _tail, "special": _special, "nan": lambda: _ragged(nan="t"),
         "nan_column": lambda: _ragged(nan="column")}
ETEMP = 4   # MONORTM_ETEMP: the reference's STOP in TIPS_2003
_RUNS = {}


def _runs(name, workdir):
    """The case's file and profiles and its two runs (computed once, shared by the two tests of the case)."""
    if name not in _RUNS:
        rec, kw, profs = CASES[name]()
        t3 = f"{workdir}/TAPE3_msfused_{name}"
        tape3.write_tape3(t3, rec, **kw)
        out = {}
        for mode in ("fused", "passes"):
            rt = api.MonoRTM(t3, profs[0].wn[0], profs[0].wn[-1])
            rt.set_option("lines_kernel", "ms")
            rt.set_option("ms_prepare", mode)
            try:
                out[mode] = rt.run(profs)
            except api.MonoRTMError as e:   # (kept: the two paths must stop alike)
                out[mode] = e.code
            rt.close()
        _RUNS[name] = (t3, profs, out["fused"], out["passes"])
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_fused_trip_is_bitwise_the_pass_loop(name, workdir, gpu):
    _, profs, fused, passes = _runs(name, workdir)
    if name == "nan":
        assert fused == ETEMP and passes == ETEMP, f"NaN temperature: fused -> {fused!r}, passes -> {passes!r}, not the temperature stop"
        return
    assert not isinstance(fused, int) and not isinstance(passes, int), f"{name}: error code {fused!r} / {passes!r}"
    for i in range(len(profs)):
        for f in FIELDS:
            x, y = np.asarray(getattr(fused[i], f)), np.asarray(getattr(passes[i], f))
            assert np.array_equal(x, y, equal_nan=True), f"{name} profile {i}: {f} differs between ms_prepare = fused and passes " \
                                                         f"(max |difference| {np.nanmax(np.abs(x - y)):.3e})"


@pytest.mark.parametrize("name", list(CASES))
def test_fused_trip_matches_oracle(name, workdir, gpu):
    from oracle.pyoracle import Oracle, OracleError

    t3, profs, fused, _ = _runs(name, workdir)
    orc = Oracle(t3, profs[0].wn[0], profs[0].wn[-1])
    if name == "nan":
        with pytest.raises(OracleError, match="TIPS"):
            orc.run(profs[3])
        orc.close()
        assert fused == ETEMP
        return
    assert not isinstance(fused, int), f"{name}: error code {fused!r}"
    seen_nan = False
    for i, pr in enumerate(profs):
        exp = orc.run(pr)
        if np.isnan(pr.wkl).any():   # (the reference's NaN stays in the profile that holds it: positions must coincide)
            compare_nan_aware(fused[i], exp, rtol=RTOL, what=f"fused vs oracle {name}[{i}]")
            seen_nan = True
        else:
            compare(fused[i], exp, rtol=RTOL, what=f"fused vs oracle {name}[{i}]")
    orc.close()
    assert seen_nan == (name == "nan_column")


def test_ms_prepare_option_values(workdir, gpu):
    """`ms_prepare` knows auto / fused / passes and refuses anything else (a mistyped switch must not run silently)."""
    rec = synth.synthetic_lines(20, seed=3)
    t3 = f"{workdir}/TAPE3_msfused_opt"
    tape3.write_tape3(t3, rec)
    wn = synth.c2_channels(10)
    rt = api.MonoRTM(t3, wn[0], wn[-1])
    for v in ("auto", "fused", "passes"):
        rt.set_option("ms_prepare", v)
    with pytest.raises(api.MonoRTMError):
        rt.set_option("ms_prepare", "trip")
    rt.close()
