"""Every Jacobian variable of DESIGN.md section 3.11 and the molecule slots on the GPU, from the infrared to the ultraviolet, against the
CPU oracle chained with the closed-form adjoint of the truth (tests/jvar_truth.py; held on the CPU by
tests/test_jacobian_vars_truth_cpu.py).  Nine fixtures between 1338 and 57783 cm-1 - where XO3CN, XO2CN, XRAYL and the infrared
branches of XN2CN are live, finish_kernel<HIGH> runs under jac_states and every OC slot carries a value - and one microwave case
for SCLCPL, SCLHW and Y0RES.  Factors are off 1 (an absolute and a relative step differ) and the scalars off their defaults.

Measure and bound: rel_err with w_floor of tests/test_jacobian.py, 1e-6, or 10 x the self-spread of a finite-difference reference
where that is larger (jvar_truth.Ref.bound); a slot whose reference is identically 0 must be exactly 0; no (case, variable) is skipped.
Run with -s for the figures (LABNOTES section 26)."""
import time

import numpy as np
import pytest

import jvar_truth as jt
import rtm_truth
from monortm_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


@pytest.fixture(scope="module")
def contexts(workdir, gpu):
    """name -> (case, MonoRTM), opened on first use."""
    made = {}

    def get(name):
        if name not in made:
            c = jt.case(name, workdir)
            made[name] = (c, api.MonoRTM(c.tape3, c.wn[0], c.wn[-1]))
        return made[name]

    yield get
    for _, rt in made.values():
        rt.close()


def launches(rt) -> int:
    return sum(rt.counter(k) for k in range(2, 8))   # one finish launch per MODM evaluation


def jacobian(rt, prs, variables, quantity="tb", what=""):
    n0, t0 = launches(rt), time.perf_counter()
    res = rt.jacobian(prs, mols=variables, quantity=quantity)
    dt = time.perf_counter() - t0
    print(f"{what}: {len(prs)} profiles, {len(variables)} variables, {launches(rt) - n0} MODM launches, {dt * 1e3:.0f} ms")
    assert res["vars"].tolist() == api.jac_codes(variables).tolist()
    return res


def check_call(res, prs, refs, variables, what):
    """Every slot of every profile against its reference; the padding layers exactly 0."""
    assert res["k_w"].shape == (len(prs), max(p.nlay for p in prs), len(variables), prs[0].nwn)
    for p, (pr, ref) in enumerate(zip(prs, refs)):
        n = pr.nlay
        for i, v in enumerate(variables):
            e = jt.check_slot(res["k_w"][p, :n, i], ref, v, f"{what}[{p}]")
            rtm_truth.record(f"jvar {jt.var_name(v)}", e)
        assert np.all(res["k_w"][p, n:] == 0), (what, p, "padding")
    rtm_truth.dump_record()


# ---- 1. every case, one extended launch with scalar launches between ------------------------------------------------------------
@pytest.mark.parametrize("name", jt.NAMES)
def test_every_slot_matches_the_reference(contexts, workdir, name):
    """3 profiles x (3 + 2 x 6) = 45 per-layer states (39 where a variable is left out): all of them in ONE extended MODM launch, and
    two launches per scalar variable behind it."""
    c, rt = contexts(name)
    refs = jt.case_reference(name, workdir)
    n0 = launches(rt)
    res = jacobian(rt, c.profiles, c.variables, what=name)
    nlv = sum(1 for v in c.variables if v in ("p", "wbrod") or not isinstance(v, str))
    assert 3 * (3 + 2 * nlv) <= 64 and launches(rt) - n0 < 3 + 2 * len(c.variables), "not the extended launch"
    check_call(res, c.profiles, refs, c.variables, name)
    for p, (pr, ref) in enumerate(zip(c.profiles, refs)):
        assert jt.rel_err(res["tb"][p], ref.q, axis=0) <= jt.TOL and jt.rel_err(res["o"][p, :pr.nlay], ref.o, axis=0) <= jt.TOL


# ---- 2. one launch per state ------------------------------------------------------------------------------------------------------
def test_one_launch_per_state_equals_the_extended_launch(contexts, workdir):
    """nir_o2_bands with 5 profiles: 5 x (3 + 2 x 6) = 75 > 64 per-layer states, so every state is a launch of its own.  Held to the
    reference, and to the 3-profile call on the common profiles at 1e-11 (the project's bound between two launch shapes of MODM).
    The line sum's slice count is pinned, as tests/test_jacobian_vars.py::test_molecule_slots_in_the_extended_launch does and for its
    reason: MODM picks it from the states of a launch, sums in another order then, and the differences divide O's last bit by 2 eps."""
    name = "nir_o2_bands"
    c, rt = contexts(name)
    five = c.profiles + c.extra_profiles(2)
    refs = jt.case_reference(name, workdir) + [jt.reference(jt.oracle_of(c), p, c.variables) for p in five[3:]]
    try:
        rt.set_option("nslice", 4)
        n0 = launches(rt)
        big = jacobian(rt, five, c.variables, what=f"{name}, 5 profiles")
        n1 = launches(rt)
        small = jacobian(rt, c.profiles, c.variables, what=f"{name}, 3 profiles")
        n2 = launches(rt)
    finally:
        rt.set_option("nslice", "auto")
    nstate = 3 + 2 * len(c.variables)
    assert n1 - n0 >= nstate - 1 and n2 - n1 <= 1 + 2 * len(jt.FACTORS), (n1 - n0, n2 - n1, nstate)
    check_call(big, five, refs, c.variables, f"{name}, 5 profiles")
    errs = {}
    for p, pr in enumerate(c.profiles):
        for i, v in enumerate(c.variables):
            a = small["k_w"][p, :, i]
            errs[p, jt.var_name(v)] = jt.rel_err(big["k_w"][p, :, i], a, axis=0, floor=jt.w_floor(a)) if a.any() else float(np.abs(big["k_w"][p, :, i]).max())
    print({k: f"{e:.1e}" for k, e in errs.items()})
    assert max(errs.values()) <= 1e-11, {k: e for k, e in errs.items() if e > 1e-11}


# ---- 3. the other entries ---------------------------------------------------------------------------------------------------------
def test_radiance_slots_match_the_reference(contexts, workdir):
    name = "ir_n2_overtone"
    c, rt = contexts(name)
    refs = jt.case_reference(name, workdir, quantity="rad")
    res = jacobian(rt, c.profiles, c.variables, quantity="rad", what=f"{name}, rad")
    check_call(res, c.profiles, refs, c.variables, f"{name}, rad")
    for p, ref in enumerate(refs):
        assert jt.rel_err(res["rad"][p], ref.q, axis=0) <= jt.TOL


def test_scan_jacobian_slots_match_the_reference(contexts, workdir):
    """Two slant paths, factors 1.0 and 2.5 in every layer: the reference is truth_adjoint at path x O, times path x dO/dtheta."""
    name = "vis_o2_aband_chappuis"
    c, rt = contexts(name)
    lm = max(p.nlay for p in c.profiles)
    path = np.array([1.0, 2.5])[:, None] * np.ones((1, lm))
    t0 = time.perf_counter()
    res = rt.scan_jacobian(c.profiles, path, mols=c.variables)
    print(f"{name}, scan: {(time.perf_counter() - t0) * 1e3:.0f} ms")
    assert res["vars"].tolist() == api.jac_codes(c.variables).tolist()
    plain = jt.case_reference(name, workdir)
    for p, pr in enumerate(c.profiles):
        n = pr.nlay
        ref = jt.reference(jt.oracle_of(c), pr, c.variables, path=path[:, :n])
        for i, v in enumerate(c.variables):
            e = jt.check_slot(res["k_w"][p, :, :n, i], ref, v, f"{name}, scan[{p}]")
            rtm_truth.record(f"jvar scan {jt.var_name(v)}", e)
            assert np.array_equal(ref.slots[v][0], plain[p].slots[v])          # the path of factor 1 is the vertical one
        assert np.all(res["k_w"][p, :, n:] == 0)
    rtm_truth.dump_record()


@pytest.mark.parametrize("edge", list(jt.EDGE_FACTORS))
@pytest.mark.parametrize("name", jt.EDGE_CASES)
def test_edge_factors_match_the_one_sided_reference(contexts, workdir, name, edge):
    """All seven factors exactly 0, and all at 5e-5 inside (0, eps]: the pair of states is fac + 2 eps / fac (modm_scalar), and the slot
    still holds d/dfac.  1e-6 flat: the reference is exact-linear."""
    c, rt = contexts(name)
    prs = jt.with_factors(c.profiles, jt.EDGE_FACTORS[edge])
    refs = jt.case_reference(name, workdir, edge=edge)
    res = jacobian(rt, prs, jt.FACTORS, what=f"{name}, factors {edge}")
    assert all(r.bound(v) == jt.TOL for r in refs for v in jt.FACTORS)
    check_call(res, prs, refs, jt.FACTORS, f"{name}, factors {edge}")
    assert sum(1 for v in jt.FACTORS if max(r.peak(v) for r in refs) > 0) >= 4
