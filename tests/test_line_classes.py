"""The class loops of the line sum against the oracle, line list by line list (tests/line_class_cases.py: constructed lists whose
classes are known by construction; tests/test_line_classes_cpu.py: the claims, the census of what is reached, the reference's own floor).

Measure: per (layer, molecule) row of O_BY_MOL, E = max over channels |got - exp| / max over channels |exp| - relative to the row's own
peak, no floor from the layer total; a row the oracle leaves at zero must be zero.  exp is oracle.pyoracle.Oracle on the inputs the
context sees (a real_kind = 4 context: the REAL inputs rounded to float32 first).
    double precision   E <= 1e-11  (the bound between the project's own two line kernels, tests/test_ms_*; the reference's summation
                       order moves a row by 7e-16: test_reference_rows_are_sums_of_single_line_rows); 1e-10 for the row that holds the
                       Voigt candidate (the device W4 is pinned at 1e-11)
    single precision   E <= (k + 16) x 2^-24 for a molecule of k lines (lc.sgl_bound)
Every ms and every sliced run is also compared with lines_kernel, unsliced, on the same batch, at 1e-11.

Configurations (lc.CONFIGS), forced with lines_kernel / nslice / tile_waves / real_kind:
    wn            lines_kernel<double>, one wavenumber per lane (lines_asm.hpp)       nwn 1, 37, 64        every list
    ms            lines_ms_kernel (lines_ms_asm.hpp), seven profiles                   nwn 5, 50, 64        every list
    dbl2          double, two wavenumbers per lane (eval_pair / eval_fast / ..)        nwn 65, 128, 129, 256; 513 with tile_waves 1, 2, 4
    sgl1 / sgl2   single precision, one / two wavenumbers per lane                     nwn 64 / 128, 200 (and the FULL lists on 0.3 - 6.5 cm-1)
    sgl4          the nw = 1, wpl = 4 float tile: 200 sounder channels, 128 x 64 states   the FULL lists; oracle on profiles 0, 64, 127
    slice3        wn with nslice = 3, seven profiles                                   the group lists (slices cut the runs)

Table offsets (H2O 1, CO2 2, O3 3, O2 7 in that order; checked against monortm_hip_line_count in test_table_offsets):
    group_bit0 / 1 / 62 / 63   0 / 1 / 62 / 63 H2O lines, O3 lines at 0-4 / 1-5 / 62-66 / 63-67, O2 behind them
    group_two                  50 H2O lines, O3 at 50 .. 99          (groups 0, 1)
    group_three                3 H2O lines, O3 at 3 .. 132           (groups 0, 1, 2; nslice = 3: slices [0, 44), [44, 88), [88, 133))
    group_three_o2             60 H2O lines, O2 at 60 .. 129         (groups 0, 1, 2)
    island_*                   12 H2O lines, then n CO2, n O3, n O2 lines of the same zone
Observed E per configuration: LABNOTES section 14.
"""
import dataclasses

import numpy as np
import pytest

import line_class_cases as lc
from monortm_amd import api, tape3

pytestmark = pytest.mark.gpu

_FILES, _ORACLE, _WORST, _DIFFERS = {}, {}, {}, {"ms": 0}


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


def _file(workdir, case):
    if case.name not in _FILES:
        path = f"{workdir}/TAPE3_lc_{case.name}"
        tape3.write_tape3(path, lc.records(case))
        _FILES[case.name] = path
    return _FILES[case.name]


def _to_f32(pr):
    r = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    return dataclasses.replace(pr, p=r(pr.p), t=r(pr.t), tz=r(pr.tz), wkl=r(pr.wkl), wbrodl=r(pr.wbrodl), clw=r(pr.clw), emiss=r(pr.emiss),
                               reflc=r(pr.reflc), tmpsfc=float(np.float32(pr.tmpsfc)))


def _expected(workdir, case, key, profs, idx):
    """The oracle's O_BY_MOL of profs[i], i in idx: computed once per (case, channel set, batch kind, precision of the inputs)."""
    from oracle.pyoracle import Oracle

    k = (case.name,) + key
    if k not in _ORACLE:
        wn = profs[0].wn
        orc = Oracle(_file(workdir, case), wn[0], wn[-1])
        _ORACLE[k] = {i: orc.run(profs[i]).o_by_mol for i in idx}
        orc.close()
        for v in _ORACLE[k].values():
            v.setflags(write=False)
    return _ORACLE[k]


def _run(workdir, case, cfg, profs, options=None):
    wn = profs[0].wn
    rt = api.MonoRTM(_file(workdir, case), wn[0], wn[-1], real_kind=cfg.kind)
    for k, v in (cfg.options if options is None else options):
        rt.set_option(k, v)
    got = rt.run(profs)
    rt.close()
    return got


def _check_rows(case, cfg, nwn, got, exp, what, voigt_row=None, steps=None):
    """E of every row against the bound of its precision; the failure names configuration, case, layer, molecule and the steps that
    walked the molecule's lines."""
    e = lc.row_errors(got, exp)
    worst = 0.0
    for lay in range(e.shape[0]):
        for m in range(e.shape[1]):
            mol = m + 1
            if cfg.kind == 4:
                tol = lc.sgl_bound(case.nlines(mol))
            else:
                tol = lc.TOL_VOIGT if voigt_row == (lay, mol) else lc.TOL_DBL
            if not e[lay, m] <= tol:
                k = int(np.argmax(np.abs(got[lay, m] - exp[lay, m])))
                walked = "" if steps is None else " steps: " + " ".join(
                    f"{l['zone']}[{l['index']}]@{l['bit']}:{'T' if s['test'] else 'U'}{'M' if s['m2'] else '1'}{'F' if s['full'] else ''}/{s['pos']}"
                    for w in steps for l, s in w["steps"] if l["mol"] == mol)
                raise AssertionError(f"{what}: layer {lay} molecule {mol} E = {e[lay, m]:.3e} > {tol:.3e}, worst at channel {k} "
                                     f"(got {got[lay, m, k]:.17g}, oracle {exp[lay, m, k]:.17g}).{walked}")
            worst = max(worst, float(e[lay, m]) / (1.0 if cfg.kind == 8 else tol))   # (single precision: as a fraction of the row's bound)
    return worst


def _note(cfg, case, worst):
    for tag in case.tags or ("other",):
        k = (cfg.name, tag)
        _WORST[k] = max(_WORST.get(k, 0.0), worst)


def _one_config(workdir, cfg, case):
    for nwn in cfg.nwn:
        wn = lc.channels(case, cfg, nwn)
        profs = lc.profiles(case, cfg, wn)
        if cfg.kind == 4:
            profs = [_to_f32(p) for p in profs]
        steps = lc.mirror(case, cfg, nwn, profs)
        exp = _expected(workdir, case, (nwn, cfg.sounder, cfg.batch, cfg.kind), profs, range(len(profs)))
        got = _run(workdir, case, cfg, profs)
        vrow = (3, case.voigt[0]) if case.voigt else None
        worst = 0.0
        for i, g in enumerate(got):
            worst = max(worst, _check_rows(case, cfg, nwn, g.o_by_mol, exp[i], f"{cfg.name} {case.name} nwn={nwn} profile {i}", vrow, steps))
        if cfg.batch:   # ... and against lines_kernel, unsliced, on the same batch
            ref = _run(workdir, case, cfg, profs, options=(("lines_kernel", "wn"), ("nslice", 1)))
            for i, (g, r) in enumerate(zip(got, ref)):
                e = lc.row_errors(g.o_by_mol, r.o_by_mol)
                assert e.max() <= lc.TOL_DBL, f"{cfg.name} {case.name} nwn={nwn} profile {i}: rows differ by {e.max():.3e} from lines_kernel unsliced"
                if cfg.family == "ms":
                    _DIFFERS["ms"] += int(not np.array_equal(g.o_by_mol, r.o_by_mol))
            assert not got[3].o_by_mol[:, case.test_mol - 1, :].any(), "the profile without a column of the molecule under test"
        _note(cfg, case, worst)
        print(f"E {cfg.name} {case.name} nwn={nwn}: {worst:.2e}" + (" of the bound" if cfg.kind == 4 else ""))


def _ids(cfg_name):
    return [c.name for c in lc.cases_of(lc.CONFIGS[cfg_name])]


def test_table_offsets(workdir, gpu):
    """The table holds the molecules' lines in the numbers the layouts of the module docstring assume."""
    for name, want in (("group_bit0", {1: 0, 3: 5, 7: 5}), ("group_bit1", {1: 1, 3: 5}), ("group_bit62", {1: 62, 3: 5}), ("group_bit63", {1: 63, 3: 5}),
                       ("group_two", {1: 50, 3: 50}), ("group_three", {1: 3, 3: 130}), ("group_three_o2", {1: 60, 7: 70}), ("island_U1_3", {1: 12, 2: 3, 3: 3, 7: 3}),
                       ("cut_middle", {7: 9})):
        case = lc.CASES[name]
        rt = api.MonoRTM(_file(workdir, case), 0.5, 40.0)
        for mol, n in want.items():
            assert rt.line_count(mol) == n == case.nlines(mol), f"{name}: molecule {mol} holds {rt.line_count(mol)} lines"
        assert rt.line_count(0) == len(case.lines)
        rt.close()


@pytest.mark.parametrize("name", _ids("wn"))
def test_wn_one_wavenumber_per_lane(workdir, gpu, name):
    """lines_kernel<double>, one wavenumber per lane: the assembly walk of lines_asm.hpp, nwn = 1, 37, 64."""
    _one_config(workdir, lc.CONFIGS["wn"], lc.CASES[name])


@pytest.mark.parametrize("name", _ids("ms"))
def test_ms_seven_profiles(workdir, gpu, name):
    """lines_ms_kernel with nwn = 5, 50, 64: seven profiles (a last group of one state at nwn = 50, a state without a column of the
    molecule under test), against the oracle and against lines_kernel."""
    _one_config(workdir, lc.CONFIGS["ms"], lc.CASES[name])


@pytest.mark.parametrize("name", _ids("dbl2"))
def test_double_two_wavenumbers_per_lane(workdir, gpu, name):
    """The C++ pair loops: nwn = 65, 128, 129 (a second tile of one channel), 256, and 513 in tiles of one, two and four waves."""
    for cfg in ("dbl2", "dbl2_tw1", "dbl2_tw2", "dbl2_tw4"):
        _one_config(workdir, lc.CONFIGS[cfg], lc.CASES[name])


@pytest.mark.parametrize("name", _ids("sgl1"))
def test_single_precision(workdir, gpu, name):
    """The float loops: nwn = 64 (one wavenumber per lane), 128 and 200 (two per lane, packed form)."""
    for cfg in ("sgl1", "sgl2"):
        _one_config(workdir, lc.CONFIGS[cfg], lc.CASES[name])


@pytest.mark.parametrize("name", _ids("sgl2_sounder"))
def test_single_precision_full_class(workdir, gpu, name):
    """The FULL lists on the sounder range, 128 and 200 channels in two-wavenumber tiles."""
    _one_config(workdir, lc.CONFIGS["sgl2_sounder"], lc.CASES[name])


@pytest.mark.parametrize("name", _ids("sgl2_sounder"))
def test_single_precision_four_wavenumber_tile(workdir, gpu, name):
    """The nw = 1, wpl = 4 tile of lines_config: float, 200 channels over 6.2 cm-1, 128 copies of a 64-layer profile (8192 states);
    the oracle on the first, a middle and the last profile."""
    cfg, case = lc.SGL4, lc.CASES[name]
    wn = lc.sounder_channels(200)
    profs = [_to_f32(p) for p in lc.big_batch(wn, 128, 64)]
    assert len(profs) * profs[0].nlay >= 8192 and wn[-1] - wn[0] <= 12.5
    idx = (0, 64, 127)
    steps = lc.mirror(case, cfg, 200, [profs[i] for i in idx])
    exp = _expected(workdir, case, ("sgl4",), profs, idx)
    got = _run(workdir, case, cfg, profs)
    worst = max(_check_rows(case, cfg, 200, got[i].o_by_mol, exp[i], f"{cfg.name} {case.name} profile {i}", None, steps) for i in idx)
    _note(cfg, case, worst)
    print(f"E {cfg.name} {case.name}: {worst:.2e} of the bound")


@pytest.mark.parametrize("name", _ids("slice3"))
def test_three_slices(workdir, gpu, name):
    """nslice = 3 on the seven profiles (one without a column of the molecule under test): the slice boundaries cut the runs of the
    group lists, and a slice's 64-line groups start at its own first line."""
    _one_config(workdir, lc.CONFIGS["slice3"], lc.CASES[name])


def test_zz_report(gpu):
    """The worst E per configuration and kind of list (the figures of LABNOTES section 14; single precision: the worst E / bound), and that forcing lines_ms_kernel did change
    the kernel: its rows differ from lines_kernel's in the last bits somewhere."""
    print()
    for (cfg, tag), w in sorted(_WORST.items()):
        print(f"worst E {cfg:14s} {tag:8s} {w:.2e}")
    if any(k[0] == "ms" for k in _WORST):
        assert _DIFFERS["ms"] > 0, "lines_ms_kernel returned lines_kernel's bits everywhere: was it launched?"
