"""Census of tests/xsec_cases.py on the oracle's trace (orc_xsec_trace), without a GPU: what entitles tests/test_xsec_kernel.py to hold
the cross-section kernel to 1e-9.

The kernel is compiled with contracted multiply-adds, the oracle without; the kernel sums 64 trips by a scan, the oracle one by one.
Such differences stay at the rounding level unless they flip an integer or a comparison.  The census shows that no cell of the
cases comes near one: the stopping criterion stays at least 1e-8 (relative) from its threshold in every trip of every walk, no index
sits within 1e-6 of an integer, int() of the number of resampled points is 1e-9 away from the next integer, no layer lies within 1e-6
of one of its three switches (hwd > hwpave, 0.25 hwb > delvx, hwb / hwd > 0.1), and a trip moves a cell by at least thr >= 1e-7.  And it
shows that the cases reach what they were built for: every branch, every position of a layer against the table temperatures, stops on
each of the 64 lanes, in the first block of 64 trips and beyond the hundredth, and stops by leaving both ends of the spectrum.

Index margin: two channels are taken out besides wn = v1x (whose quotient is exactly 0).  At wn = v1x + 1e-9 the quotient is about 1e-7:
that close to 0 in absolute terms, but 1e9 roundings away from it.  At wn = v2x it is (v2x - v1x) / ((v2x - v1x) / npts): two divisions
that the oracle and the kernel both round to nearest on identical operands once npts agrees, which the npts margin vouches for.
With regions no finer than 0.0125 cm-1 (thr >= 1e-7 at 1000 mb asks for that) no step brings either of them to 1e-6.
"""
import numpy as np
import pytest

import xsec_cases as xc
from oracle.pyoracle import XS_BRANCHES, XS_STOP_BOTH_ENDS, XS_STOP_CRITERION

UNPROCESSED, OUTSIDE, WALK, LINEAR = range(len(XS_BRANCHES))
KINDS = pytest.mark.parametrize("kind", [8, 4])


def stack(orc, field):
    """[nreg, layers of the three profiles one after the other, nwn]"""
    return np.concatenate([getattr(t, field) for t in orc.trace], axis=1)


def layers(orc):
    profs = orc.profs["all"]
    return np.concatenate([p.p for p in profs]), np.concatenate([p.t for p in profs])


def chan(v: float) -> int:
    i = int(np.searchsorted(xc.WN, v))
    assert xc.WN[i] == v
    return i


def position(t: float, temps) -> str:
    """Where the bracket search of MONORTM_XSEC_SUB (:1677-1704) puts a layer temperature."""
    if len(temps) == 1:
        return "single"
    if t < temps[0]:
        return "below"
    if t > temps[-1]:
        return "above"
    for k, tk in enumerate(temps):
        if t == tk:
            return "at_coldest" if k == 0 else "at_warmest" if k == len(temps) - 1 else "at_middle"
    return "inside"


@KINDS
def test_oracle_run_is_quick_and_finite(kind):
    orc = xc.oracle(kind)
    print(f"oracle on the cross-section cases, real_kind = {kind}: {orc.seconds:.2f} s")
    assert orc.seconds < 5.0
    for label, odx in orc.odx.items():
        for a in odx:
            assert np.isfinite(a).all(), label
    br = stack(orc, "branch")
    for f, where in (("thr", br == WALK), ("crit_margin", br == WALK), ("idx_margin", br >= WALK), ("npts_margin", br >= OUTSIDE),
                     ("sw_margin", br >= OUTSIDE)):
        assert np.isfinite(stack(orc, f)[where]).all(), f


@KINDS
def test_every_branch_and_position_occurs(kind):
    orc = xc.oracle(kind)
    br, trips, thr = stack(orc, "branch"), stack(orc, "trips"), stack(orc, "thr")
    P, T = layers(orc)
    tabs = orc.tabs
    regs = [r for rs in tabs.regions for r in rs]
    for b in (UNPROCESSED, OUTSIDE, WALK, LINEAR):
        assert (br == b).any(), XS_BRANCHES[b]
    # three temperatures: every position, each in a walk
    r = xc.region("t3")
    seen = {position(T[l], regs[r].temps) for l in range(len(T)) if (br[r, l] == WALK).any()}
    assert seen >= {"below", "at_coldest", "inside", "at_middle", "at_warmest", "above"}, seen
    # one temperature: walk and linear cells
    r = xc.region("one")
    assert len(regs[r].temps) == 1 and (br[r] == WALK).any() and (br[r] == LINEAR).any()
    # two disjoint regions of one molecule, each with cells of its own; two overlapping ones that share channels
    for name in ("d1", "d2"):
        assert (br[xc.region(name)] >= WALK).any()
    assert not ((br[xc.region("d1")] >= WALK) & (br[xc.region("d2")] >= WALK)).any()
    both = (br[xc.region("ov1")] >= WALK) & (br[xc.region("ov2")] >= WALK)
    assert len(np.flatnonzero(both.any(axis=0))) >= 3
    # FSCDXS bounds wider than the header's
    r = xc.region("pad")
    g = regs[r]
    assert g.v1 < g.v1h and g.v2 > g.v2h
    inside = (xc.WN >= g.v1h) & (xc.WN <= g.v2h)
    between = ((xc.WN >= g.v1) & (xc.WN < g.v1h)) | ((xc.WN > g.v2h) & (xc.WN <= g.v2))
    rim = ((xc.WN >= g.v1 - 1.0) & (xc.WN < g.v1)) | ((xc.WN > g.v2) & (xc.WN <= g.v2 + 1.0))
    assert inside.any() and between.sum() >= 2 and rim.sum() >= 2 and xc.WN[chan(g.v1 - 1.0)] == g.v1 - 1.0
    assert (br[r][:, inside] >= WALK).all() and (br[r][:, between | rim] == OUTSIDE).all()
    # a region that no channel comes within 1 cm-1 of, with channels on either side
    r = xc.region("skip")
    g = regs[r]
    assert (br[r] == UNPROCESSED).all() and (xc.WN < g.v1 - 1.0).any() and (xc.WN > g.v2 + 1.0).any()
    assert (br[[k for k in range(len(regs)) if k != r]] != UNPROCESSED).all()
    # exact edges, in walks and in the linear branch
    r = xc.region("edge")
    g = regs[r]
    delvx = (g.v2h - g.v1h) / (g.npts - 1)
    for v in (g.v1h, g.v1h + 1e-9, g.v2h):
        assert (br[r][:, chan(v)] == WALK).any() and (br[r][:, chan(v)] == LINEAR).any(), v
    assert g.v1h + 1e-9 > g.v1h
    ind0 = np.flatnonzero((xc.WN > g.v1h + 1e-9) & (xc.WN < g.v1h + delvx))
    last = np.flatnonzero((xc.WN > g.v2h - delvx) & (xc.WN < g.v2h))
    assert len(ind0) and len(last)                      # just inside each end: ind = 0 and the last grid interval
    assert (br[r][:, ind0] == LINEAR).any() and (br[r][:, last] == LINEAR).any()
    assert (br[r][:, ind0] == WALK).any() and (br[r][:, last] == WALK).any()
    # pressure sweep, in every region: the step clipped to delvx (thr = 1e-6 step / hwb is then under 0.25e-6 by more than the
    # recomputation of the step takes, 1 / npts < 0.4 %), step = 0.25 hwb, and the linear branch under the pressure of the measurements
    assert P.max() == 1000.0 and P.min() == 0.5
    walk = br == WALK
    for name in xc.REGION_NAMES:
        if name == "skip":
            continue
        r = xc.region(name)
        assert (walk[r] & (thr[r] < 0.24e-6)).any() and (walk[r] & (thr[r] > 0.249e-6)).any(), name
        low = P < regs[r].pres_mb.min()
        inr = (xc.WN >= regs[r].v1h) & (xc.WN <= regs[r].v2h)
        assert low.any() and (br[r][low][:, inr] == LINEAR).all(), name
    # wide region: most walks end by the criterion, deep inside the data
    r = xc.region("wide")
    sk = stack(orc, "stopkind")
    assert (walk[r] & (sk[r] == XS_STOP_CRITERION)).sum() > 0.8 * walk[r].sum() and trips[r].max() > 6400
    # negative samples: stops in the first block
    r = xc.region("neg")
    assert min(np.min(d) for d in regs[r].data) < 0 and (walk[r] & (trips[r] <= 64)).sum() >= 3
    # ragged file: a layer at or under the coldest temperature reads the short file alone; channels in its zero tail, walk and linear
    r = xc.region("ragged")
    g = regs[r]
    assert len(g.data[0]) < len(g.data[-1]) == g.npts
    tail = xc.WN[(xc.WN <= g.v2h)] > g.v1h + (g.v2h - g.v1h) / (g.npts - 1) * len(g.data[0])
    tail = np.flatnonzero(xc.WN <= g.v2h)[tail]
    cold = T <= g.temps[0]
    assert len(tail) >= 2 and (br[r][cold][:, tail] == WALK).any() and (br[r][cold][:, tail] == LINEAR).any()


@KINDS
def test_stops_cover_lanes_blocks_and_both_kinds(kind):
    orc = xc.oracle(kind)
    walk, trips, sk = stack(orc, "branch") == WALK, stack(orc, "trips"), stack(orc, "stopkind")
    assert (trips[walk] >= 1).all() and np.isin(sk[walk], (XS_STOP_CRITERION, XS_STOP_BOTH_ENDS)).all()
    crit = walk & (sk == XS_STOP_CRITERION)
    lanes = np.bincount((trips[crit] - 1) % 64, minlength=64)
    print(f"real_kind = {kind}: {walk.sum()} walks, {crit.sum()} end by the criterion ({(trips[crit] <= 64).sum()} in the first block, "
          f"{(trips[crit] > 6400).sum()} after more than 100 blocks), {(walk & (sk == XS_STOP_BOTH_ENDS)).sum()} by leaving both ends; "
          f"fewest stops on a lane {lanes.min()}, longest walk {trips.max()} trips; {(stack(orc, 'branch') == LINEAR).sum()} linear cells")
    assert (lanes > 0).all(), lanes
    assert (trips[crit] <= 64).sum() >= 3
    assert (trips[walk] > 64 * 100).any()
    assert (walk & (sk == XS_STOP_BOTH_ENDS)).any()


@KINDS
def test_margins(kind):
    """No cell is excused, but for the index margin of the three exact-edge channels (the module's docstring)."""
    orc = xc.oracle(kind)
    br = stack(orc, "branch")
    walk, inr = br == WALK, br >= WALK
    thr, crit, idx, npts, sw = (stack(orc, f) for f in ("thr", "crit_margin", "idx_margin", "npts_margin", "sw_margin"))
    print(f"real_kind = {kind}: min thr {thr[walk].min():.3g}, criterion margin {crit[walk].min():.3g}, npts margin {npts[inr].min():.3g}, "
          f"switch margin {sw[inr].min():.3g}")
    assert thr[walk].min() >= xc.MIN_THR
    assert crit[walk].min() >= xc.MIN_CRIT
    assert npts[inr].min() >= xc.MIN_NPTS
    assert sw[inr].min() >= xc.MIN_SW
    regs = [r for rs in orc.tabs.regions for r in rs]
    worst = np.inf
    for r, g in enumerate(regs):
        held = inr[r] & ~np.isin(xc.WN, (g.v1h, g.v1h + 1e-9, g.v2h))[None, :]
        if held.any():
            worst = min(worst, idx[r][held].min())
        assert (idx[r][inr[r] & (xc.WN == g.v1h)[None, :]] == 0).all()
        # the two channels left out are what the docstring says they are: a quotient of ~1e-7 (1e8 roundings above 0), and npts itself
        assert (idx[r][inr[r] & (xc.WN == g.v1h + 1e-9)[None, :]] >= 1e-8).all()
        assert (idx[r][inr[r] & (xc.WN == g.v2h)[None, :]] <= 1e-9).all()
    print(f"real_kind = {kind}: index margin {worst:.3g}")
    assert worst >= xc.MIN_IDX


@KINDS
def test_cells_without_data_are_exactly_zero(kind):
    """A cell of a one-molecule call none of whose regions is processed with the channel in range is exactly zero; the others hold
    something in at least one layer (so that the GPU test compares numbers, not zeros)."""
    orc = xc.oracle(kind)
    regs = [(m, r) for m, rs in enumerate(orc.tabs.regions) for r in rs]
    for m in range(len(xc.NAMES)):
        mine = [k for k, (mm, _) in enumerate(regs) if mm == m]
        for i, tr in enumerate(orc.trace):
            live = (tr.branch[mine] >= WALK).any(axis=0)
            odx = orc.odx[f"only{m}"][i]
            assert not odx[~live].any()
            assert np.count_nonzero(odx[live]) > 0.9 * live.sum()
