"""The column layout of the microwave finish kernel (continuum_kernel.hip: finish_mw_kernel_col, a workgroup per profile and block of
64 layers, set-up and coarse stage with lane = layer) against the layer layout (finish_mw_kernel, a workgroup per layer) and the oracle.

The two layouts differ in which index the lanes hold, not in the arithmetic: every array must be bitwise the same.  Each case makes
one context and the same calls with option finish_mw = layer and = column, and asserts
  * np.array_equal on O, OC, O_CLW, O_BY_MOL and the six spectral outputs,
  * monortm_hip_counter(9) moved by exactly the column calls, counter 2 (finish_mw_kernel's variant) by all of them,
  * the column result within continuum_cases.TOL_DBL / TOL_SGL / TOL_CLW of the oracle (the tolerances of tests/test_finish_kernels.py).
Shapes are the smallest at which the layout can go wrong: ragged layer counts (1, 3, 6 of 6: the zero fill, a wave without a layer),
a layer count that no wave count divides (7), a second block of layers (66), 1 .. 130 channels (one, two and three blocks of 64), a
dvset grid, cloud in no / one / every layer, a layer without H2O, every continuum factor alone, cross sections, line files that are
header-only / 20 lines / forced through lines_ms_kernel / sliced (where the layer layout must stay), both precisions, a graph replay.
"""
import dataclasses
import types

import numpy as np
import pytest

import continuum_cases as cc
from common import RTOL, compare
from monortm_amd import api, synth, tape3

pytestmark = pytest.mark.gpu

COLUMN_COUNTER = 9
FIELDS = ("o", "o_by_mol", "oc", "o_clw", "rup", "rdn", "trtot", "rad", "tb", "tmr")


@pytest.fixture(scope="module")
def dev(workdir):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    t20 = f"{workdir}/TAPE3_mw_column_20"
    tape3.write_tape3(t20, synth.synthetic_lines(20, seed=5, vlo=0.3, vhi=30.0))
    t500 = f"{workdir}/TAPE3_mw_column_500"
    tape3.write_tape3(t500, synth.synthetic_lines(500, seed=6, vlo=0.3, vhi=30.0))
    return types.SimpleNamespace(t0=cc.header_only_tape3(f"{workdir}/TAPE3_mw_column"), t20=t20, t500=t500)


def _chan(seed: int, n: int, lo: float = 0.3, hi: float = 25.0) -> np.ndarray:
    """n channels in [lo, hi): up to 25 cm-1 the coarse arrays of 64 layers fit the 40 KB of a column workgroup (30 cm-1 is just over)."""
    return np.sort(np.random.default_rng(seed).uniform(lo, hi, n))


def _profiles(seed: int, wn, nlays, dvset=0.0, cloud="some"):
    """Profile i: synth.perturbed_profile of a state of its own with nlays[i] layers.  cloud: none | some (liquid in 2 - 4 layers of every
    second profile) | middle (one layer) | all (every layer)."""
    out = []
    for i, nl in enumerate(nlays):
        pr = synth.perturbed_profile(seed * 1000 + i, wn, nlay=nl, cloud=(cloud == "some" and i % 2 == 0), irt=(1 if i % 3 == 0 else 3))
        clw = pr.clw.copy()
        if cloud == "middle":
            clw[:] = 0.0
            clw[nl // 2] = 0.03
        elif cloud == "all":
            clw[:] = np.random.default_rng(seed + i).uniform(0.005, 0.05, nl)
        elif cloud == "none":
            clw[:] = 0.0
        pr = dataclasses.replace(pr, clw=clw)
        pr.dvset = dvset
        pr.cntnm = np.random.default_rng(7000 + seed).uniform(0.3, 1.7, cc.NFAC)
        out.append(pr)
    return out


def both_layouts(rt, call, ncalls: int = 1, column_expected: bool = True):
    """call() under finish_mw = layer and = column: (layer result, column result), with the launch counters asserted."""
    res = {}
    for mode in ("layer", "column"):
        rt.set_option("finish_mw", mode)
        mw0, col0 = rt.counter(api.FINISH_COUNTER0), rt.counter(COLUMN_COUNTER)
        res[mode] = call()
        assert rt.counter(api.FINISH_COUNTER0) - mw0 == ncalls, f"finish_mw = {mode}: not {ncalls} launch(es) of the microwave finish"
        want = ncalls if (mode == "column" and column_expected) else 0
        assert rt.counter(COLUMN_COUNTER) - col0 == want, f"finish_mw = {mode}: counter 9 moved by {rt.counter(COLUMN_COUNTER) - col0}, not {want}"
    rt.set_option("finish_mw", "auto")
    return res["layer"], res["column"]


def assert_same_bits(a, b, what: str):
    for i, (x, y) in enumerate(zip(a, b)):
        for f in FIELDS:
            assert np.array_equal(getattr(x, f), getattr(y, f), equal_nan=True), f"{what}: profile {i}, {f} differs between the layouts"


def hold_to_oracle(t3, profs, got, kind: int, what: str):
    from oracle.pyoracle import Oracle

    orc = Oracle(t3, profs[0].wn[0], profs[0].wn[-1])
    tol = cc.TOL_DBL if kind == 8 else cc.TOL_SGL
    for i, (p, g) in enumerate(zip(profs, got)):
        x = orc.run(p)
        e_oc, e_clw = cc.E(g.oc, x.oc), cc.E(g.o_clw, x.o_clw)
        print(f"E {what} [{i}] real_kind={kind}: oc={e_oc:.2e} o_clw={e_clw:.2e}")
        assert e_oc <= tol, f"{what} [{i}]: OC off the oracle by {e_oc:.3g}"
        assert e_clw <= (cc.TOL_CLW if kind == 8 else cc.TOL_SGL), f"{what} [{i}]: O_CLW off the oracle by {e_clw:.3g}"
        if kind == 8:
            compare(g, x, rtol=RTOL, what=f"{what} [{i}]")
        else:
            compare(g, x, rtol=5e-5, what=f"{what} [{i}]", rad_floor=1e-30)   # (SGL_VS_DBL of tests/test_finish_kernels.py)
    orc.close()


# name: (channels, dvset, layers per profile, cloud, real_kind)
SHAPES = {
    "ragged_50": (_chan(1, 50), 0.0, (1, 3, 6), "some", 8),                 # zero fill, a wave without a layer
    "ragged_50_sgl": (_chan(1, 50), 0.0, (1, 3, 6), "some", 4),
    "one_channel": (_chan(2, 1), 0.0, (7,), "middle", 8),                  # seven layers: no wave count divides them
    "five_channels_two_blocks": (_chan(3, 5), 0.0, (66, 40), "some", 8),   # 66 layers: a second block of two
    "64_channels": (_chan(4, 64), 0.0, (7, 2), "all", 8),
    "65_channels": (_chan(5, 65), 0.0, (7,), "some", 8),                   # a second block of channels
    "65_channels_sgl": (_chan(5, 65), 0.0, (7,), "some", 4),
    "130_channels": (_chan(6, 130), 0.0, (5, 3), "all", 8),                # three blocks
    "grid_40": (0.5 + 0.7 * np.arange(40), 0.7, (6, 3, 1), "none", 8),      # dvset != 0
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_column_is_bitwise_the_layer_layout_and_holds_the_oracle(name, dev):
    wn, dvset, nlays, cloud, kind = SHAPES[name]
    profs = _profiles(sum(map(ord, name)), wn, nlays, dvset, cloud)
    if kind == 4:
        profs = [cc.to_f32(p) for p in profs]
    rt = api.MonoRTM(dev.t0, wn[0], wn[-1], real_kind=kind)
    lay, col = both_layouts(rt, lambda: rt.run(profs))
    rt.close()
    assert_same_bits(lay, col, name)
    if cloud != "some":   # (`some`: wherever the profile is between 255 and 285 K)
        assert any(d.o_clw.any() for d in col) == (cloud != "none")
    hold_to_oracle(dev.t0, profs, col, kind, name)


def test_every_factor_alone_and_a_layer_without_h2o(dev):
    """The one-factor calls of continuum_cases (cntnm = e_k, no cloud: a dead branch stores its zeros) and a layer whose H2O column is 0."""
    wn = _chan(7, 50)
    profs = _profiles(70, wn, (6, 5, 1), cloud="some")
    wkl = profs[1].wkl.copy()
    wkl[2, 0] = 0.0
    profs[1] = dataclasses.replace(profs[1], wkl=wkl)
    rt = api.MonoRTM(dev.t0, wn[0], wn[-1])
    for label, ps in cc.calls(profs):
        lay, col = both_layouts(rt, lambda: rt.run(ps))
        assert_same_bits(lay, col, label)
        if label == "main":
            assert not col[1].oc[2, 0].any() and col[1].oc[0, 0].any()   # the self / foreign slot of the layer without H2O
            hold_to_oracle(dev.t0, ps, col, 8, "factors main")
        elif label in ("only3", "only4", "only6"):                      # O3, O2, Rayleigh: nothing below 820 cm-1
            assert not any(d.o.any() for d in col), label
        else:
            assert any(d.o.any() for d in col), label
            hold_to_oracle(dev.t0, ps[:1], col[:1], 8, f"factors {label}")
    rt.close()


def test_cross_sections_are_added(dev):
    """ODXSEC present (ixsect = 1, the tables and states of tests/xsec_cases.py on its channels below 820 cm-1)."""
    import xsec_cases as xc

    wn = xc.WN[xc.WN < 800.0]
    assert len(wn) >= 3
    profs = [dataclasses.replace(p, wn=wn) for p in dict(xc.calls())["all"]]
    rt = api.MonoRTM(dev.t0, wn[0], wn[-1])
    rt.set_xsec(xc.tables())
    lay, col = both_layouts(rt, lambda: rt.modm(profs, ixsect=1))
    rt.close()
    for k, what in enumerate(("O", "O_BY_MOL", "OC", "O_CLW", "ODXSEC")):
        assert np.array_equal(lay[k], col[k]), what
    O, _, OC, _, ODX = col
    assert ODX.any() and np.all(np.isfinite(O))
    for i, p in enumerate(profs):
        want = ODX[i, : p.nlay] + OC[i, : p.nlay].sum(axis=1)
        assert cc.E(O[i, : p.nlay], want) <= xc.TOL_SUM, i


@pytest.mark.parametrize("how", ["lines_kernel", "lines_ms_kernel"])
def test_with_lines(how, dev):
    """A 20-line file: O_BY_MOL and the line sums come from lines_kernel / (forced) lines_ms_kernel, the finish reads them."""
    wn = _chan(8, 50)
    profs = _profiles(80, wn, (6, 3, 7), cloud="some")
    rt = api.MonoRTM(dev.t20, wn[0], wn[-1])
    assert rt.line_count(0) > 0
    if how == "lines_ms_kernel":
        rt.set_option("lines_kernel", "ms")
    lay, col = both_layouts(rt, lambda: rt.run(profs))
    rt.close()
    assert_same_bits(lay, col, how)
    assert all(d.o_by_mol.any() for d in col)
    hold_to_oracle(dev.t20, profs, col, 8, how)


def test_sliced_line_lists_keep_the_layer_layout(dev):
    """One profile on 500 lines: the line list is sliced and the slices are summed inside the finish kernel - finish_mw_kernel's work,
    whatever the option says."""
    wn = _chan(9, 50)
    profs = _profiles(90, wn, (6,), cloud="some")
    rt = api.MonoRTM(dev.t500, wn[0], wn[-1])
    lay, col = both_layouts(rt, lambda: rt.run(profs), column_expected=False)
    rt.close()
    assert_same_bits(lay, col, "sliced")


def test_a_range_too_wide_for_the_lds_keeps_the_layer_layout(dev):
    wn = _chan(10, 20, 0.3, 400.0)      # ~400 coarse items x 64 layers: beyond the 40 KB of a column workgroup
    profs = _profiles(100, wn, (4, 2), cloud="none")
    rt = api.MonoRTM(dev.t0, wn[0], wn[-1])
    lay, col = both_layouts(rt, lambda: rt.run(profs), column_expected=False)
    rt.close()
    assert_same_bits(lay, col, "wide range")


def _batch(dev, wn, nlays, layout, ends=None):
    import torch

    profs = _profiles(110, wn, nlays, cloud="some")
    rt = api.MonoRTM(dev.t0, 0.3, 200.0)
    rt.set_option("finish_mw", layout)
    db = api.DeviceBatch(rt, profs)
    if ends is not None:
        db.wn_ends = np.ascontiguousarray(ends, np.float64)
    return torch, profs, rt, db


def test_graph_replay_and_padded_layers(dev):
    """The column layout recorded into a HIP graph and replayed twice: array for array the stream launches of the layer layout, the
    layers a profile does not have exactly zero whatever the arrays held.  The spectral range handed in (wn_ends) is narrower than the
    channels, so the outer channels lie outside [V1ABS + 1, V2ABS - 1] and take no continuum (`inside` is false)."""
    wn = _chan(11, 50, 0.5, 40.0)
    ends = (10.2, 30.3)
    torch, profs, rt_l, db_l = _batch(dev, wn, (6, 1, 3), "layer", ends)
    db_l.step()
    torch.cuda.synchronize()
    db_l.check()
    ref = db_l.dumps(profs)
    rt_l.close()
    outer = (wn < 8.0) | (wn > 32.0)
    assert outer.any() and not outer.all()
    assert not any(d.oc[:, :, outer].any() for d in ref) and all(d.oc[:, :, ~outer].any() for d in ref)

    torch, profs, rt, db = _batch(dev, wn, (6, 1, 3), "column", ends)
    before = rt.counter(COLUMN_COUNTER)
    db.capture()
    assert rt.counter(COLUMN_COUNTER) - before == 2     # the warm step and the recorded one
    for _ in range(2):
        for t in (db.O, db.OBM, db.OC, db.OCLW, db.RAD, db.TB, db.TMR):
            t.fill_(float("nan"))
        db.replay()
        torch.cuda.synchronize()
        db.check()
        assert rt.counter(COLUMN_COUNTER) - before == 2  # a replay does not enter the host side
        assert_same_bits(ref, db.dumps(profs), "graph replay")
        O, OC, OCLW, OBM = (t.cpu().numpy() for t in (db.O, db.OC, db.OCLW, db.OBM))
        for i, p in enumerate(profs):
            for a in (O, OC, OCLW, OBM):
                assert not a[i, p.nlay:].any() and np.isfinite(a[i]).all(), (i, p.nlay)
    rt.close()


def test_a_new_range_inside_a_capture_is_refused(dev):
    """The first call for a spectral range builds its item records, which allocates: inside a stream capture it is refused with the
    message that says what to do, in the column layout as in the layer layout."""
    wn = _chan(12, 50)
    torch, profs, rt, db = _batch(dev, wn, (6, 3), "column")
    db.step()                       # every workspace of this shape exists from here on
    torch.cuda.synchronize()
    db2 = api.DeviceBatch(rt, [dataclasses.replace(p, wn=wn + 100.0) for p in profs])   # same shape, a range not served yet
    g = torch.cuda.CUDAGraph()
    with pytest.raises(api.MonoRTMError) as e:
        with torch.cuda.graph(g):
            db2.step()
    assert api.ERRORS[e.value.code] == "EUNSUPPORTED"
    assert "cannot be set up inside a stream capture: run one step outside the capture first" in str(e.value)
    torch.cuda.synchronize()
    db2.step()                      # outside the capture it is served
    torch.cuda.synchronize()
    db2.check()
    assert np.isfinite(db2.O.cpu().numpy()).all()
    rt.close()


def test_option_values(dev):
    """`finish_mw` knows auto / layer / column and refuses anything else (a mistyped switch must not run silently); counters 8, 15, 20
    and -1 stay unknown."""
    wn = _chan(13, 5)
    rt = api.MonoRTM(dev.t0, wn[0], wn[-1])
    for v in ("auto", "layer", "column", ""):
        rt.set_option("finish_mw", v)
    for bad in ("Column", "col", "1", "on"):
        with pytest.raises(api.MonoRTMError) as e:
            rt.set_option("finish_mw", bad)
        assert e.value.code == 6
    assert rt.counter(COLUMN_COUNTER) == 0
    assert all(rt.counter(k) == -1 for k in (8, 15, 20, -1))
    # auto: a batch of three profiles is far from filling the chip with column workgroups - the layer layout serves it
    rt.run(_profiles(130, wn, (6, 3, 1)))
    assert rt.counter(COLUMN_COUNTER) == 0 and rt.counter(api.FINISH_COUNTER0) == 1
    rt.close()
