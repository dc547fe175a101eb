"""Fixtures for the seam around a molecule run in lines_ms_kernel (tests/test_ms_run_finish.py, tests/test_ms_run_finish_cpu.py):
the smallest batches at which the end of a run - the sums handed back from the walk, the radiation term, the sum over the
molecules - can go wrong, and the host identity that pins the order and the bits of that sum.

Everything is built from monortm_amd.synth (and bench.py's recipes for the c2lc / c4brd shapes); nothing is read from disk."""
import numpy as np

from monortm_amd import synth, tape3

_COLS = ("vnu", "sp", "alfa", "epp", "mol", "hwhm", "tmpalf", "pshift", "iflg", "brd_flg", "brd_dat", "sdep")


def take(rec: tape3.LineRecords, keep) -> tape3.LineRecords:
    """The records `keep` (mask or indices) of a list without coupling records (every record is a line of its own)."""
    assert not (rec.iflg != 0).any()
    return tape3.LineRecords(**{k: getattr(rec, k)[keep] for k in _COLS})


def ragged():
    """33 channels: seven lanes a state, nine states a wave - lanes 5 and 6 of a state lack the fifth slot, so kvalid differs between
    the lanes; 11 profiles: a last wave with two live states; 2 / 3 / 5 layers under nlay_max 5: waves whose states end at different
    layers.  200 lines over five molecules: every run is shorter than a chunk, several runs complete inside one chunk."""
    wn = synth.c2_channels(33, seed=33)
    lays = (5, 2, 3, 5, 3, 2, 5, 5, 2, 3, 5)
    profs = [synth.perturbed_profile(400 + i, wn, nlay=lays[i], cloud=(i % 3 == 0), irt=(1 if i % 4 == 0 else 3)) for i in range(11)]
    return synth.synthetic_lines(200, seed=3301), profs


def long_runs():
    """About 150 lines of one molecule (H2O, the first in the file: its run is parked and resumed over several chunks and ends in
    mid-chunk) and about 10 of each other one; 50 channels, 7 profiles (two waves of six and one state), 4 layers."""
    big = synth.synthetic_lines(1200, seed=4402)
    mol = big.mol % 100
    keep = np.zeros(len(big), bool)
    keep[np.flatnonzero(mol == 1)[::3][:150]] = True
    for m in (2, 3, 4, 7):
        idx = np.flatnonzero(mol == m)
        keep[idx[:: max(1, len(idx) // 10)][:10]] = True
    rec = take(big, keep)
    wn = synth.c2_channels(50, seed=50)
    profs = [synth.perturbed_profile(500 + i, wn, nlay=4, cloud=(i == 2)) for i in range(7)]
    return rec, profs


def columns_a():
    """Channels below 6 cm-1 (windows end at 31 cm-1), N2O lines only above 35 cm-1: molecule 4 is never walked and its O_BY_MOL
    stays what the prologue wrote.  Profile 2 has no H2O column at all - the first molecule with lines: its state's optical depth is
    exactly 0 while the five other states of its wave sum."""
    big = synth.synthetic_lines(260, seed=5503)
    mol = big.mol % 100
    rec = take(big, ~((mol == 4) & (big.vnu < 35.0)))
    assert ((rec.mol % 100) == 4).any()
    wn = synth.c2_channels(50, seed=51, hi=6.0)
    profs = [synth.perturbed_profile(600 + i, wn, nlay=4) for i in range(7)]
    profs[2].wkl[:, 0] = 0.0
    return rec, profs


def columns_b():
    """No H2O line in the list: the first molecule that is walked (the one that starts the sum over the molecules) is CO2."""
    big = synth.synthetic_lines(260, seed=5504)
    rec = take(big, (big.mol % 100) != 1)
    wn = synth.c2_channels(50, seed=52)
    profs = [synth.perturbed_profile(650 + i, wn, nlay=3) for i in range(7)]
    return rec, profs


def rare_shapes():
    """bench.py's c2lc recipe at 7 profiles x 6 layers: every O2 line first-order coupled (general_term), 10 % speed dependent, the
    model top at 0.004 hPa and 12 channels on line centres (the Voigt scan corrects the sums of a run that then completes)."""
    import bench

    rec, p64, _, _, _ = bench.build_workload("c2lc", 0, 1)
    wn = p64[0].wn
    profs = [synth.perturbed_profile(i, wn, nlay=6, ztop_km=93.0) for i in range(7)]
    return rec, profs


def species_broadening():
    """bench.py's c4brd recipe at 7 profiles x 4 layers: the IBRD instantiation of the kernel."""
    import bench

    rec, p64, _, _, _ = bench.build_workload("c4brd", 0, 1)
    wn = p64[0].wn
    profs = [synth.perturbed_profile(i, wn, nlay=4) for i in range(7)]
    for q in profs:
        q.ibrd = 1
    return rec, profs


CASES = {"ragged": ragged, "long_runs": long_runs, "columns_a": columns_a, "columns_b": columns_b, "rare_shapes": rare_shapes,
         "species_broadening": species_broadening}


def host_total(d) -> np.ndarray:
    """What finish_mw_kernel makes of the line sums (continuum_kernel.hip, stage D): with sequential float64 adds,
    ((((sum over the molecules in molecule order) + 0.) + 0.) + soc) + od_clw, soc = ((((0. + OC0) + OC1) + 0.) + 0.) + OC4.
    The sum over the molecules starts at the first one; the exact zeros of molecules that were never walked change no bit."""
    obm = np.asarray(d.o_by_mol, np.float64)
    oc = np.asarray(d.oc, np.float64)
    s = obm[:, 0, :].copy()
    for m in range(1, obm.shape[1]):
        s = s + obm[:, m, :]
    soc = np.zeros_like(s)
    soc = soc + oc[:, 0, :]
    soc = soc + oc[:, 1, :]
    soc = soc + 0.0
    soc = soc + 0.0
    soc = soc + oc[:, 4, :]
    o = s + 0.0
    o = o + 0.0
    o = o + soc
    return o + np.asarray(d.o_clw, np.float64)
