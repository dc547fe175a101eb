"""Jacobian variables besides the molecules on the GPU: ln P and ln WBRODL per layer against per-layer brute
force, the scalar arguments of MODM (continuum factors, SCLCPL, SCLHW, Y0RES) against differences of plain runs, dead variables,
that nothing existing moves, step halving, the three entry families, the resident batch with graph replay, sharding, refusals.

Small inputs throughout: 7 channels; layer counts on both sides of 24, where the adjoint goes from 2 to 8 layer groups.  (Step halving
also on two fixtures above 1340 cm-1, through tests/jvar_truth.py; every variable against the oracle there: tests/test_jacobian_vars_truth.py.)"""
import numpy as np
import pytest

import jvar_truth as jt
import obs_cases as oc
from monortm_amd import api, synth, tape3
from test_jacobian import _replace, code, profiles, rel_err, w_floor

pytestmark = pytest.mark.gpu

NEW = tuple(api.JAC_VARS)                 # every new variable, by name
STEP = 1e-3                               # half-step of the scalar brute force


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


def _ctx(workdir, name, rec, wn, **kw):
    t3 = f"{workdir}/TAPE3_{name}"
    tape3.write_tape3(t3, rec, **kw)
    return t3, wn, api.MonoRTM(t3, wn[0], wn[-1])


@pytest.fixture(scope="module")
def case(workdir, gpu):
    """The line list of tests/test_jacobian.py (coupled O2 lines: SCLCPL and Y0RES are live) through 7 microwave channels."""
    t3, wn, rt = _ctx(workdir, "jvars", synth.synthetic_lines(300, seed=777, lc_frac=0.5, sdep_frac=0.2), np.unique(synth.c2_channels(7, seed=11)))
    yield t3, wn, rt
    rt.close()


@pytest.fixture(scope="module")
def plain_case(workdir, gpu):
    """The same list without coupling records: SCLCPL, Y0RES and SCLHW reach nothing."""
    t3, wn, rt = _ctx(workdir, "jvars_plain", synth.synthetic_lines(300, seed=777, sdep_frac=0.2), np.unique(synth.c2_channels(7, seed=11)))
    yield t3, wn, rt
    rt.close()


@pytest.fixture(scope="module")
def real_case(workdir, gpu):
    """The real_like list (the O2 non-resonant IFLG = 3 / -3 term: SCLHW is live) through 7 sounder channels."""
    rec, kw, _ = synth.real_like_file()
    t3, wn, rt = _ctx(workdir, "jvars_real", rec, synth.sounder_channels()[[4, 6, 10, 16, 21, 27, 35]], **kw)
    yield t3, wn, rt
    rt.close()


def with_scalar(prs, name, delta):
    """The batch with the scalar argument `name` shifted by delta (MODM takes the scalars of profiles[0]: all get it)."""
    if name in ("sclcpl", "sclhw", "y0res"):
        return [_replace(p, **{name: getattr(p, name) + delta}) for p in prs]
    fac = prs[0].cntnm.copy()
    fac[api.JAC_VARS[name] - api.JAC_VARS["xself"]] += delta
    return [_replace(p, cntnm=fac.copy()) for p in prs]


def scalar_difference(rt, prs, name, step):
    tb = [np.array([d.tb for d in rt.run(with_scalar(prs, name, s))]) for s in (step, -step)]
    return (tb[0] - tb[1]) / (2 * step)


def check_scalar(res, ref, names, what):
    """sum over the layers of every named slot against ref[name] [nprof, nwn]: 1e-6 of the peak of the variable's column over the
    profile's channels."""
    errs = {}
    for i, name in enumerate(names):
        got = res["k_w"][:, :, i].sum(axis=1)
        peak = np.abs(ref[name]).max(axis=1, keepdims=True)
        assert np.all(peak > 0), (what, name, "the variable is dead on this input")
        errs[name] = float(np.max(np.abs(got - ref[name]) / peak))
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-6, (what, errs)


# ---- 1. ln P and ln WBRODL against per-layer brute force ------------------------------------------------------------------------
def layer_brute_force(run, prs, eps):
    """Central differences of TB, every perturbed profile changing ONE layer's P or WBRODL: per profile (k_p, k_wbrod) [nlay, nwn]."""
    out = []
    for pr in prs:
        batch = []
        for k in range(pr.nlay):
            for name in ("p", "wbrodl"):
                for sgn in (1, -1):
                    a = getattr(pr, name).copy()
                    a[k] *= 1 + sgn * eps
                    batch.append(_replace(pr, **{name: a}))
        tb = np.array([d.tb for d in run(batch)])
        out.append(tuple(np.array([(tb[4 * k + 2 * v] - tb[4 * k + 2 * v + 1]) / (2 * eps) for k in range(pr.nlay)]) for v in range(2)))
    return out


def test_layer_variables_match_per_layer_brute_force(case):
    """k_w of "p" and "wbrod" at jac_dlnw = 3e-4 against the brute force of plain runs at the same step, rel_err with w_floor as
    tests/test_jacobian.py::test_jacobian_matches_per_layer_brute_force_gpu.  Bound: 1e-6, or 10 x the brute force's own spread between
    eps = 3e-4 and eps = 1e-3 on these inputs where that is larger - the difference of two TBs resolves a weak derivative only to TB's
    rounding over 2 eps (~3e-9 K), so there the reference is the limit, not the kernel.  Both numbers are printed (LABNOTES section 25)."""
    _, wn, rt = case
    prs = profiles(wn, [400, 401], [24, 17], irt=(1, 3))
    try:
        rt.set_option("jac_dlnw", 3e-4)
        res = rt.jacobian(prs, mols=("p", "wbrod"))
    finally:
        rt.set_option("jac_dlnw", "auto")
    assert res["vars"].tolist() == [1001, 1002]
    bf, bf3 = layer_brute_force(rt.run, prs, 3e-4), layer_brute_force(rt.run, prs, 1e-3)
    errs, bounds = {}, {}
    for p, pr in enumerate(prs):
        n = pr.nlay
        for i, name in enumerate(("p", "wbrod")):
            ref = bf[p][i]
            spread = rel_err(bf3[p][i], ref, axis=0, floor=w_floor(ref))
            errs[f"{p} {name}"] = rel_err(res["k_w"][p, :n, i], ref, axis=0, floor=w_floor(ref))
            bounds[f"{p} {name}"] = max(1e-6, 10 * spread)
            print(f"profile {p} {name}: kernel against brute force {errs[f'{p} {name}']:.2e}, brute force 3e-4 against 1e-3 {spread:.2e}")
            assert np.any(res["k_w"][p, :n, i] != 0)
    assert all(errs[k] <= bounds[k] for k in errs), (errs, bounds)


# ---- 2. the scalar variables against differences of plain runs ---------------------------------------------------------------
def test_scalar_variables_match_brute_force(case):
    _, wn, rt = case
    prs = profiles(wn, [410, 411, 412], [24, 17, 6], irt=(1, 3))
    names = ("xself", "xfrgn", "xn2cn", "sclcpl", "y0res")
    ref = {n: scalar_difference(rt, prs, n, STEP) for n in names}
    res = rt.jacobian(prs, mols=names)
    assert res["vars"].tolist() == [api.JAC_VARS[n] for n in names]
    check_scalar(res, ref, names, "default step")
    # O is linear in a continuum factor: the same K from a difference of optical depths over +-0.5
    try:
        rt.set_option("jac_dlnw", 0.5)
        wide = rt.jacobian(prs, mols=("xself",))
    finally:
        rt.set_option("jac_dlnw", "auto")
    check_scalar(wide, ref, ("xself",), "xself, step 0.5")


def test_sclhw_matches_brute_force(real_case):
    _, wn, rt = real_case
    prs = profiles(wn, [420, 421], [24, 17], irt=(1, 3))
    ref = {"sclhw": scalar_difference(rt, prs, "sclhw", STEP)}
    check_scalar(rt.jacobian(prs, mols=("sclhw",)), ref, ("sclhw",), "real_like")


def test_zero_continuum_factor_is_one_sided(case):
    """XSELF = 0: MODM switches the self continuum off at a factor <= 0, so the pair of states is 2 eps / 0, and the slot still holds
    d/dXSELF at 0.  The reference can only come from the positive side: one-sided differences of TB over h = 1e-3 and 2e-3, whose
    first-order truncation (RTM's curvature) cancels in 2 D(h) - D(2h); what remains is O(h^2), below the 1e-6 of check_scalar."""
    _, wn, rt = case
    prs = profiles(wn, [425], [17], irt=(1,))
    fac = prs[0].cntnm.copy()
    fac[0] = 0.0
    off = [_replace(prs[0], cntnm=fac)]
    tb = [np.array([d.tb for d in rt.run(with_scalar(off, "xself", s))]) for s in (0.0, STEP, 2 * STEP)]
    ref = {"xself": 2 * (tb[1] - tb[0]) / STEP - (tb[2] - tb[0]) / (2 * STEP)}
    check_scalar(rt.jacobian(off, mols=("xself",)), ref, ("xself",), "xself = 0")


# ---- 3. dead variables are exactly zero ---------------------------------------------------------------------------------------
def test_dead_variables_are_exactly_zero(case, plain_case):
    _, wn, rt = plain_case
    prs = profiles(wn, [430, 431], [24, 17], irt=(1, 3))
    assert wn[-1] < 820.0
    res = rt.jacobian(prs, mols=("xrayl", "sclcpl", "y0res", "sclhw", 1))
    for i in range(4):
        assert np.all(res["k_w"][:, :, i] == 0), res["vars"][i]
    assert np.any(res["k_w"][:, :, 4] != 0)
    # WBRODL = 0 in some layers, and the padding of the shorter profile
    _, wn, rt = case
    dry = [_replace(p, wbrodl=np.where(np.arange(p.nlay) % 3 == 1, 0.0, p.wbrodl)) for p in prs]
    res = rt.jacobian(dry, mols=("wbrod", "p", "xself", "sclcpl"))
    for p, pr in enumerate(dry):
        n = pr.nlay
        z = pr.wbrodl == 0
        assert z.any() and np.all(res["k_w"][p, :n, 0][z] == 0) and np.all(res["k_w"][p, :n, 0][~z] != 0)
        assert np.all(res["k_w"][p, n:] == 0)
        assert np.all(res["k_w"][p, :n, 1:] != 0)


# ---- 4. nothing existing moves ------------------------------------------------------------------------------------------------
OLD_FIELDS = ("o", "tb", "k_t", "k_tz", "k_clw", "k_o", "k_sfc")


def test_molecule_slots_and_other_fields_are_bit_equal(case):
    """24 profiles x 6 layers: every state is a launch of its own (more than 64 state-profiles), of the shape of a plain MODM call."""
    _, wn, rt = case
    prs = profiles(wn, list(range(440, 464)), 6, irt=(1, 3))
    mixed = rt.jacobian(prs, mols=(1, "p", 3, "xself"))
    mol = rt.jacobian(prs, mols=(1, 3))
    assert mixed["vars"].tolist() == [1, 1001, 3, 1011] and mol["vars"].tolist() == [1, 3]
    assert np.array_equal(mixed["k_w"][:, :, 0], mol["k_w"][:, :, 0]) and np.array_equal(mixed["k_w"][:, :, 2], mol["k_w"][:, :, 1])
    for name in OLD_FIELDS:
        assert np.array_equal(mixed[name], mol[name]), name
    assert np.all(mixed["k_w"][:, :, 1] != 0) and np.all(mixed["k_w"][:, :, 3] != 0)


def test_molecule_slots_in_the_extended_launch(case):
    """2 profiles: all per-layer states of either call ride in ONE extended MODM launch, of 18 and of 14 profiles - MODM's launch shape
    may differ in the last bit.  Bound: 1e-11, the project's bound between its line kernels.
    The line sum's slice count is pinned ("nslice"): left to itself MODM cuts the list into 5 slices for the 18 x 24 states of the one
    launch and into 7 for the 14 x 24 of the other (modm_plan.hpp), O then differs in its last bit (6e-17), and the differences divide
    that by 2 jac_dlnw - measured without the pin: k_t 2.6e-12, H2O's slot 2.1e-12, O3's slot 1.65e-11, a weak absorber's rounding,
    not a moved slot."""
    _, wn, rt = case
    prs = profiles(wn, [470, 471], [24, 17], irt=(1, 3))
    try:
        rt.set_option("nslice", 4)
        mixed = rt.jacobian(prs, mols=(1, "p", 3, "xself"))
        mol = rt.jacobian(prs, mols=(1, 3))
    finally:
        rt.set_option("nslice", "auto")
    errs = {}
    for p in range(2):
        for a, b in ((0, 0), (2, 1)):
            ref = mol["k_w"][p, :, b]
            errs[f"{p} k_w[{b}]"] = rel_err(mixed["k_w"][p, :, a], ref, axis=0, floor=w_floor(ref))
    for name in OLD_FIELDS:
        errs[name] = rel_err(mixed[name], mol[name], axis=1 if mol[name].ndim > 2 else 0)
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-11, errs


# ---- 5. step halving ----------------------------------------------------------------------------------------------------------
def _two_steps(rt, prs, names):
    a = rt.jacobian(prs, mols=names)["k_w"]
    try:
        rt.set_option("jac_dlnw", api.JAC_DLNW / 2)
        b = rt.jacobian(prs, mols=names)["k_w"]
    finally:
        rt.set_option("jac_dlnw", "auto")
    return {n: (a[:, :, i], b[:, :, i]) for i, n in enumerate(names)}


@pytest.fixture(scope="module")
def halved(case, real_case):
    """k_w of every new variable at jac_dlnw and at half of it: on the synthetic list (24 and 17 layers), and SCLHW on real_like (24
    and 6 layers).  Computed once for the cases below."""
    _, wn, rt = case
    out = _two_steps(rt, profiles(wn, [480, 481], [24, 17], irt=(1, 3)), NEW)
    _, wn, rt = real_case
    out["sclhw, real_like"] = _two_steps(rt, profiles(wn, [482, 483], [24, 6], irt=(1, 3)), ("sclhw",))["sclhw"]
    return out


HIGH_INPUTS = ("uv_hartley_huggins", "ir_o2_fundamental")   # fixtures above 1340 cm-1: finish_kernel<HIGH>, XO3CN / XO2CN / XRAYL live
HIGH_VARS = ("p", "wbrod") + jt.FACTORS
HIGH_ALIVE = {"uv_hartley_huggins": ("p", "wbrod", "xo3cn", "xo2cn", "xrayl"),
              "ir_o2_fundamental": ("p", "wbrod", "xself", "xfrgn", "xco2c", "xo2cn", "xrayl")}


@pytest.fixture(scope="module")
def halved_high(workdir, gpu):
    """The same on the three profiles of two cases of tests/jvar_truth.py (factors off 1), where the factors the microwave leaves dead
    halve something non-zero."""
    out = {}
    for name in HIGH_INPUTS:
        c = jt.case(name, workdir)
        rt = api.MonoRTM(c.tape3, c.wn[0], c.wn[-1])
        try:
            for n, ab in _two_steps(rt, c.profiles, HIGH_VARS).items():
                out[f"{n}, {name}"] = ab
        finally:
            rt.close()
    return out


@pytest.mark.parametrize("name", NEW + ("sclhw, real_like",))
def test_step_halving(halved, name):
    """Halving jac_dlnw moves no slot by more than 1e-6 (rel_err and floor of tests/test_jacobian.py::test_step_halving).

    [xco2c]: below 30 cm-1 the CO2 continuum is ~1e-12 of a layer's optical depth; differences of the TOTAL optical depth gave a slot of
    quantisation noise there (1.0 and 0.5 in this measure).  The states of a continuum factor hold its OC slot instead (DESIGN.md
    section 3.11), which resolves the slot on its own scale."""
    _check_halving(halved[name], name, name in ("p", "wbrod", "xself", "xfrgn", "xco2c", "xn2cn", "sclcpl", "y0res", "sclhw, real_like"))


def _check_halving(ab, name, alive):
    a, b = ab
    errs = [rel_err(b[p], a[p], axis=0, floor=w_floor(a[p])) for p in range(a.shape[0])]
    print(f"{name}: peak |k_w| {np.abs(a).max():.3e}, step halving {max(errs):.2e}")
    assert max(errs) <= 1e-6, errs
    if alive:
        assert np.any(a != 0), "the variable is dead on this input"
    else:
        assert not np.any(a != 0) and not np.any(b != 0), "a variable that reaches nothing gives slots that are exactly 0"


@pytest.mark.parametrize("name", [f"{v}, {n}" for n in HIGH_INPUTS for v in HIGH_VARS])
def test_step_halving_above_1340(halved_high, name):
    """test_step_halving where XO3CN, XO2CN and XRAYL are live (uv_hartley_huggins) and where Rayleigh is 4e-11 of a layer's optical
    depth (ir_o2_fundamental): its states hold Rayleigh's own term - differences of the total gave
    quantisation there.  Every variable of the list is either alive or exactly 0 on these inputs."""
    v, n = name.split(", ")
    _check_halving(halved_high[name], name, v in HIGH_ALIVE[n])


# ---- 6. the three entry families ------------------------------------------------------------------------------------------------
MIXED = (1, "p", "sclcpl", 3, "wbrod", "xfrgn")


def test_scan_and_obs_entries_agree(case):
    _, wn, rt = case
    prs = profiles(wn, [490, 491, 492], [24, 17, 6], irt=(1, 3))
    jac = rt.jacobian(prs, mols=MIXED)
    ones = rt.scan_jacobian(prs, np.ones((1, 24)), mols=MIXED)
    assert ones["vars"].tolist() == jac["vars"].tolist()
    for name in api.JAC_FIELDS:
        assert np.array_equal(ones[name] if name == "o" else ones[name][:, 0], jac[name]), name
    assert np.all(jac["k_w"][0] != 0)
    # obs_jacobian against the float64 contraction of scan_jacobian's k_w: the bound tests/test_obs_jacobian.py holds k_w to
    import test_obs_jacobian as toj

    path = oc.factors(9)[:, None] * (1.0 + 0.01 * np.arange(24) / 23.0)[None, :]
    mono = dict(rt.scan_jacobian(prs, path, mols=MIXED))
    mono["y"] = mono["tb"]
    op = oc.operator("A", "comb", len(wn))
    with toj.handle(rt, op) as h:
        got = rt.obs_jacobian(prs, path, h, mols=MIXED)
    assert got["vars"].tolist() == jac["vars"].tolist() and got["k_w"].shape == (3, op.nview, 24, len(MIXED), op.nchan)
    np.testing.assert_array_equal(got["o"], mono["o"])
    toj.check_full(got, mono, op, toj.TOL8, "mixed variables", fields=("y", "k_w"))


# ---- 7. the resident batch and graphs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [(1, "p", "sclcpl"), ("xco2c", 1, "xself")], ids=["layer+scalar", "continuum"])
def test_device_batch_and_graph_replay(case, names):
    """(continuum: the states of a continuum factor are a 2-D device copy of its OC slot behind the MODM launch - captured with it.)"""
    import torch

    _, wn, rt = case
    prs = profiles(wn, [500, 501], [24, 17], irt=(1, 3))
    ref = rt.jacobian(prs, mols=names)
    db = api.DeviceBatch(rt, prs)
    got = db.jacobian(mols=names)
    torch.cuda.synchronize()
    db.check()
    assert got["vars"].tolist() == api.jac_codes(names).tolist()

    def same(ref):
        for name in api.JAC_FIELDS:
            assert rel_err(got[name].cpu().numpy(), ref[name], axis=1 if ref[name].ndim > 2 else 0) <= 1e-12, name

    same(ref)
    assert db.jacobian(mols=[int(v) for v in api.jac_codes(names)]) is got      # the cache is keyed by the codes; overwritten in place
    assert db.jacobian(mols=[n.upper() if isinstance(n, str) else n for n in names]) is got
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            db.jacobian(mols=names)
    torch.cuda.current_stream().wait_stream(s)
    db.P.mul_(1.01)
    for name in api.JAC_FIELDS:
        got[name].zero_()
    g.replay()
    torch.cuda.synchronize()
    db.check()
    ref2 = rt.jacobian([_replace(p, p=p.p * 1.01) for p in prs], mols=names)
    assert not np.array_equal(ref2["tb"], ref["tb"])
    same(ref2)


# ---- 8. sharding ----------------------------------------------------------------------------------------------------------------
def test_multi_device_context_equals_one_device(case, monkeypatch):
    """Two shards (2 + 1 profiles) against one device at 1e-12.  The line sum's slice count is pinned on both contexts: MODM picks it
    from the states of a launch (modm_plan.hpp) - here 4 for the one device's 33 x 17 and 7 for the shards' - and sums in another
    order then; tests/test_jacobian.py's version of this test has 7 on both sides by its shapes.  Measured without the pin: k_t
    4.0e-12, k_w 2.9e-12 (the last bit of O over 2 h), every other field <= 3.5e-16."""
    t3, wn, rt = case
    prs = profiles(wn, [510, 511, 512], 17, irt=(1, 3))
    monkeypatch.setenv("MONORTM_DEVICES", "0,0")
    m = api.MonoRTM(t3, wn[0], wn[-1], ngpu=0)
    assert m.lib.monortm_hip_device_count(m.ctx) == 2
    m.set_option("jac_dt", api.JAC_DT)   # passed on to every shard
    try:
        rt.set_option("nslice", 4)
        m.set_option("nslice", 4)
        one = rt.jacobian(prs, mols=MIXED)
        two = m.jacobian(prs, mols=MIXED)
    finally:
        rt.set_option("nslice", "auto")
        m.close()
    errs = {name: rel_err(two[name], one[name], axis=1 if one[name].ndim > 2 else 0) for name in api.JAC_FIELDS}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-12, errs


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(case):
    import torch

    t3, wn, rt = case
    prs = profiles(wn, [520], 17)
    launches = lambda: sum(rt.counter(k) for k in range(2, 8))   # noqa: E731  (one finish launch per MODM evaluation)
    rt.jacobian(prs, mols=(1, "p"))
    n0 = launches()
    assert n0 > 0
    for bad in ((999,), (1003,), (1018,), (1024,), (1, 1010), ("p", "p"), (1001, "p"), ("xself", 2, 1011), tuple(range(1, 8)) * 6):
        assert code(lambda: rt.jacobian(prs, mols=bad)) == "EARG", bad
    assert len(tuple(range(1, 8)) * 6) > 39
    path = np.ones((1, 17))
    assert code(lambda: rt.scan_jacobian(prs, path, mols=(1024,))) == "EARG"
    assert code(lambda: rt.jacobian(prs, mols=np.arange(1, 41))) == "EARG"                          # njac = 40
    db = api.DeviceBatch(rt, prs)
    for bad in ((1003,), ("wbrod", 1002), tuple(range(1, 41))):
        assert code(lambda: db.jacobian(mols=bad)) == "EARG", bad
    r4 = api.MonoRTM(t3, wn[0], wn[-1], real_kind=4)
    assert code(lambda: r4.jacobian(prs, mols=("p",))) == "EUNSUPPORTED"
    r4.close()
    torch.cuda.synchronize()
    assert launches() == n0
    db.check()
    # the context still works after every refusal
    assert np.all(np.isfinite(rt.jacobian(prs, mols=("wbrod", 1))["k_w"]))
