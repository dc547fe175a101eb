"""The cases of tests/far_cases.py without a GPU: the far_kernel variants they declare follow from the mirror of the host's choices with
a margin to every threshold, the census of the mirror shows that each case reaches the branch it was built for, and the oracle's own
additivity - the noise floor of the measure tests/test_far_kernel.py uses - is two decades below that module's tightest bound.
Run with -s for the margins, the census and the floors."""
import numpy as np
import pytest

import far_cases as fc
from far_cases import CO2, O3
from monortm_amd import tape3

GUARD_MARGIN = 0.05     # the Voigt guard of far_plan_kernel: its two sides differ by at least this wherever the mirror decides with them


def _tagged(tag):
    return [n for n, c in fc.CASES.items() if tag in c.tags]


# ---------------------------------------------------------------------------------------------------------------------------------
# the variants
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", fc.RUNS)
def test_declared_variants_follow_from_the_mirror(name, kind):
    """steps of every level >= 10 % away from 16, 32 and 128; the NWF multiset the case declares is the mirror's."""
    case = fc.CASES[name]
    pl = fc.plan(case, kind)
    assert pl.levels >= 1 and pl.ntile >= 4
    print(f"{name} real_kind={kind}: tiles of {pl.tw}, {pl.ntile} tiles, {pl.nlines} lines held ({pl.lines_per_cm:.0f} per cm-1, {pl.nactive} molecules), "
          + ", ".join(f"level {l}: {s:.1f} steps -> {n} (margin {fc.threshold_margin(s):.2f})" for l, (s, n) in enumerate(zip(pl.steps, pl.nwf))))
    for l, s in enumerate(pl.steps):
        assert fc.threshold_margin(s) >= fc.MARGIN, f"{name}: level {l} has {s:.2f} steps"
    assert tuple(sorted(pl.nwf)) == case.expect
    if case.far_levels is None:
        assert "forced_levels" not in case.tags
    else:
        assert pl.levels == case.far_levels
    # bounds of a case: <= 2 profiles, <= 3 layers, <= 2600 wavenumbers, ~20000 lines
    assert len(case.layers) <= 2 and max(len(l) for l in case.layers) <= 3 and case.nwn <= 2600 and len(fc.records(case)) <= 20000
    assert sum(s.stop - s.start for _w, s in fc.stretches(case)) <= 800


def test_every_variant_is_expected_somewhere():
    dbl = {n for c in fc.CASES.values() for n in c.expect}
    sgl = {n for name in fc.SGL_CASES for n in fc.CASES[name].expect}
    assert dbl == {1, 2, 4, 8} and {2, 4, 8} <= sgl
    assert set(fc.SGL_CASES) == {"o3_top8", "co2_nwf4", "h2o_two_resonances"}
    for name in fc.SGL_CASES:     # (the same launches in both precisions: lines_config differs below 257 wavenumbers only)
        assert fc.plan(fc.CASES[name], 4).nwf == fc.plan(fc.CASES[name], 8).nwf
    # the natural cases: launched with more than one wave below a top level of more, and at the top alone
    assert any(c.far_levels is None and len([n for n in c.expect if n > 1]) >= 2 for c in fc.CASES.values())
    assert sum(c.nslice > 0 for c in fc.CASES.values()) == 1


def test_case_list():
    """An edit that drops a case shows here."""
    assert list(fc.CASES) == ["o3_top8", "o3_top4_tile2", "o3_three_levels", "co2_nwf4", "co2_nwf2", "o2_nwf4", "h2o_two_resonances", "idle_waves",
                              "ragged_batch", "stub_tile", "small_tiles_1", "small_tiles_2", "narrow_tiles_wide_lines", "far_only_molecule",
                              "near_clusters"]
    assert {fc.CASES[n].tile_waves for n in ("small_tiles_1", "small_tiles_2", "narrow_tiles_wide_lines")} == {1, 2}
    assert fc.CASES["stub_tile"].nwn == 4 * fc.plan(fc.CASES["stub_tile"]).tw + 1
    assert len({len(l) for l in fc.CASES["ragged_batch"].layers}) == 2
    for c in fc.CASES.values():     # the surface layer and the top layer in every profile
        assert all(l[0] == 0 and l[-1] == 63 for l in c.layers)


# ---------------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_census_guard_margin_and_multiwave_work(name):
    """Wherever the mirror decides with the Voigt guard its two sides are 5 % apart (the mirror's Doppler width is typed, not read from
    the product's tables); every case has steps of both kinds - cut below 32 terms and carried into the LDS sums - and no far line
    nearer than kappa = 1.2 half-widths."""
    c = fc.census(fc.CASES[name])
    print(f"{name}: " + " ".join(f"{k}={v if isinstance(v, (int, np.integer)) else round(float(v), 4)}" for k, v in vars(c).items() if k != "orders")
          + f" orders {min(c.orders)}..{max(c.orders)}")
    assert c.min_guard >= GUARD_MARGIN
    assert c.min_kappa >= fc.FAR_KAPPA and c.lds > 0 and c.short_order > 0


def test_census_two_resonances():
    for name in _tagged("two"):
        c = fc.census(fc.CASES[name])
        assert c.two > 0 and c.excl > 0 and c.e0 > 0, vars(c)
        assert any(n > 1 for n in fc.CASES[name].expect)
    assert not fc.census(fc.CASES["co2_nwf4"]).two and not fc.census(fc.CASES["co2_nwf4"]).excl      # CO2 has no negative resonance


def test_census_inheritance_and_one_wavenumber_parent():
    for name in _tagged("inherit"):
        assert fc.census(fc.CASES[name]).inherit > 0
    case = fc.CASES["stub_tile"]
    pl, c = fc.plan(case), fc.census(case)
    last = fc.interval(pl, 0, pl.ntile - 1)
    assert last.first == last.last == case.nwn - 1 and last.rho == 0.0
    # the stub, its parent and its grandparent hold one wavenumber and take the far lines of the top level; two of them are parents
    assert [fc.interval(pl, l, (pl.ntile - 1) >> l).rho == 0.0 for l in range(pl.levels)] == [True, True, True, False]
    assert c.stub_parent == 2 * len(list(fc.states(case))) and c.inherit >= 3 * len(list(fc.states(case)))
    assert pl.nwf[-1] > 1


def test_census_idle_waves_and_zero_column():
    case = fc.CASES["idle_waves"]
    pl = fc.plan(case)
    few = fc.census(case, CO2)
    assert few.idle_waves > 0 and few.short_run_multiwave > 0
    sts = list(fc.states(case))
    top = pl.levels - 1
    assert pl.nwf[top] > 1
    for _ip, _lay, st in sts:        # every run of the few-line molecule under the multi-wave variant leaves waves >= 1 without a step
        for j in range(fc.far_level_count(pl.ntile, top)):
            assert all(nxt - pos < 128 for pos, nxt, _t in fc.kernel_runs(pl, st, top, j, CO2))
    assert sum(1 for _ip, _lay, st in sts if st.W[O3 - 1] == 0.0) == 1
    assert fc.census(case, O3).flag_only == pl.ni and few.flag_only == 0
    # placement: the heavy molecule on several XCDs, the other on one
    assert fc.far_xcd_share(pl.mol_start, O3 - 1)[1] > 1 and fc.far_xcd_share(pl.mol_start, CO2 - 1)[1] == 1
    assert fc.far_xcd_share(pl.mol_start, 0) == (0, 0)


def test_census_wide_lines_and_orders():
    for name in _tagged("negA"):
        c = fc.census(fc.CASES[name])
        assert c.negA > 0 and c.full_order > 0 and c.short_order > 0 and fc.FAR_P in c.orders and min(c.orders) < fc.FAR_PREG, vars(c)
    assert fc.far_order(1.2, 1.0) == fc.FAR_P and fc.far_order(1.9, 1.0) < fc.FAR_PREG and fc.far_order(1e6, 1.0) == 8


def test_census_far_only_molecule_and_near_clusters():
    case = fc.CASES["far_only_molecule"]
    pl, top = fc.plan(case), fc.plan(case).levels - 1
    for _ip, _lay, st in fc.states(case):
        for j in range(pl.ntile):       # no tile walks a line of the molecule, no tile expands one: the parent's series alone
            assert not fc.tile_runs(pl, st, j, CO2) and not fc.kernel_runs(pl, st, 0, j, CO2)
            assert fc.anything_there(pl, st, 0, j, CO2)
        assert all(fc.kernel_runs(pl, st, top, j, CO2) for j in range(fc.far_level_count(pl.ntile, top)))
    case = fc.CASES["near_clusters"]
    pl, top = fc.plan(case), fc.plan(case).levels - 1
    assert top == 1
    for _ip, _lay, st in fc.states(case):
        assert not any(fc.kernel_runs(pl, st, top, j, CO2) for j in range(fc.far_level_count(pl.ntile, top)))     # far for no parent
        served = [bool(fc.kernel_runs(pl, st, 0, j, CO2)) for j in range(pl.ntile)]
        assert served == [True, False, True, True]       # (tile 1 holds the cluster)
    assert fc.census(case, CO2).no_parent == 3 * len(list(fc.states(case)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference: the table the mirror expects, and the floor of the measure
# ---------------------------------------------------------------------------------------------------------------------------------
def _distinct_cases():
    seen, out = set(), []
    for name, c in fc.CASES.items():
        key = (c.parts, c.v1, c.dv, c.nwn, c.layers, c.zero, tuple((s.start, s.stop) for _w, s in fc.stretches(c)))
        if key not in seen:
            seen.add(key)
            out.append(name)
    return out


@pytest.mark.parametrize("name", _distinct_cases())
def test_reference_floor(name, workdir):
    """The line sum is linear in the line set: on every compared stretch the oracle's rows for the odd and the even records add up to its
    rows for the whole list, to 1e-11 of the row's peak (the measure of tests/test_far_kernel.py).  The oracle keeps the lines the
    mirror expects the context to keep."""
    from oracle.pyoracle import Oracle

    case = fc.CASES[name]
    rec, wn, pl = fc.records(case), case.wn, fc.plan(case)
    paths = [f"{workdir}/TAPE3_farcpu_{name}{s}" for s in ("", "_odd", "_even")]
    tape3.write_tape3(paths[0], rec)
    for par, p in ((1, paths[1]), (0, paths[2])):
        tape3.write_tape3(p, fc._subset(rec, np.arange(len(rec)) % 2 == par))
    orcs = [Oracle(p, wn[0], wn[-1]) for p in paths]
    for mol in range(1, fc.NMOL + 1):
        assert orcs[0].nlines(mol) == pl.mol_start[mol + 1] - pl.mol_start[mol], mol
    worst = 0.0
    for what, sl in fc.stretches(case):
        for ip, pr in enumerate(fc.profiles(case, sl)):
            whole, odd, even = (o.run(pr).o_by_mol for o in orcs)
            e = fc.row_error(odd + even, whole)
            assert np.isfinite(e).all()
            worst = max(worst, float(e.max()))
            for mol in range(1, fc.NMOL + 1):       # rows of the molecules with lines and a column are not empty
                has = pl.mol_start[mol + 1] > pl.mol_start[mol]
                assert np.array_equal(np.abs(whole[:, mol - 1]).max(axis=-1) > 0, has & (pr.wkl[:, mol - 1] != 0)), (what, ip, mol)
    for o in orcs:
        o.close()
    print(f"additivity floor {name}: {worst:.2e}")
    assert worst < fc.FLOOR_MAX, f"{name}: {worst:.2e}"
