"""The Jacobians with the cross-section molecules (monortm_hip_jacobian_xs, _scan_jacobian_xs, _obs_jacobian_xs; xsec_jac_kernel.hip;
DESIGN.md section 3.12) against the oracle chained with the closed-form adjoint of the truth.

Context, tables and TAPE3 as tests/test_xsec_kernel.py has them (a line file without lines; the tables of tests/xsec_cases.py through
set_xsec).  The batch is the three ragged profiles of xsec_cases (10 / 4 / 7 layers x 127 channels), call `all`, in three amount sets:
`all` itself, `zeros` (F12's column zero in two layers of every profile) and `big` (all amounts x 1e3: the cross sections dominate O
at the band peaks).

References.  k_o, the Planck k_t: rtm_truth.truth_adjoint at the oracle's O (its MODM without cross sections + its ODXSEC).
  XS slot of molecule m   k_o x the oracle's ODXSEC of molecule m alone (xsec_cases' calls only<m>; linear in the amounts).  Exact.
  "p" slot                k_o x (d O / d ln P of the oracle's MODM without cross sections, by jvar_truth's Richardson recipe, + the
                          frozen-plan derivative of tests/xsec_jac_truth.py)
  k_t                     the Planck k_t + k_o x (the same two terms for T; Richardson over 0.1 / 0.2 K)
Errors as jvar_truth measures them (rel_err over the layer axis with w_floor); bound 1e-6, or 10 x the reference's self-spread where
that is larger.  No cell is left out of any comparison.

Observed on an MI355X (20 tests, 7.4 s, 4.8 s of them the CPU references, computed once): O bit-equal to modm(ixsect = 1); XS slots
<= 1.5e-13 (`all`, `zeros`), 3.4e-12 (`big`), their sum against k_o x ODXSEC <= 3.7e-16; the "p" slot 3.0e-11 .. 4.7e-11 in `all` (the
continuum's: the cross sections' share is small at 1e15 molecules / cm^2) and 7.3e-9 .. 1.1e-8 in `big`, where it is the cross
sections' - the h^2 truncation of eps = 1e-4 that tests/test_xsec_jac_cpu.py shows for the frozen differences; k_t 3.8e-8 .. 6.7e-8;
every self-spread <= 2.8e-11, so the bound is 1e-6 throughout.  Scan: <= 1.7e-13 against 1e-12; obs against the contracted scan
<= 4.3e-16 S.
"""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

import continuum_cases as cc
import jvar_truth as jt
import rtm_truth
import test_obs_jacobian as toj
import xsec_cases as xc
import xsec_jac_truth as xt
from monortm_amd import api

pytestmark = pytest.mark.gpu

XS = tuple(f"xs:{n}" for n in xc.NAMES)
NX = len(xc.NAMES)
SETS = ("all", "zeros", "big")
ZERO_MOL = 2                                   # F12: three regions, two of them overlapping
PATHS = np.array([1.0, 1.7, 0.6])
_replace = dataclasses.replace


def code(f) -> str:
    try:
        f()
    except api.MonoRTMError as e:
        return api.ERRORS.get(e.code, str(e.code))
    return "OK"


def zero_layers(nlay: int):
    return [1, nlay - 1]


def profiles(name: str) -> list:
    base = [_replace(p, irt=irt) for p, irt in zip(xc.oracle(8).profs["all"], (1, 3, 1))]
    if name == "all":
        return base
    out = []
    for p in base:
        xa = p.xamnt.copy()
        if name == "zeros":
            xa[zero_layers(p.nlay), ZERO_MOL] = 0.0
        else:
            xa *= 1e3
        out.append(_replace(p, xamnt=xa))
    return out


@pytest.fixture(scope="module")
def dev(workdir):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    t3 = cc.header_only_tape3(f"{workdir}/TAPE3_xsec_jacobian")
    rt = api.MonoRTM(t3, xc.WN[0], xc.WN[-1])
    assert rt.line_count(0) == 0
    rt.set_xsec(xc.oracle(8).tabs)
    yield types.SimpleNamespace(t3=t3, rt=rt)
    rt.close()


# ---- the references, once per session ------------------------------------------------------------------------------------------------
_REF = {}


def _oracle(dev):
    from oracle.pyoracle import Oracle

    if "orc" not in _REF:
        _REF["orc"] = Oracle(dev.t3, xc.WN[0], xc.WN[-1])
    return _REF["orc"]


def no_xs(pr):
    return _replace(pr, xs_names=None, xamnt=None)


def base_terms(dev, i: int):
    """Of profile i, independent of the amounts: the oracle's O without cross sections and its derivatives in ln P and T (with those
    from the half steps), and per molecule and unit amount the oracle's ODXSEC and the frozen-plan derivatives."""
    key = ("base", i)
    if key in _REF:
        return _REF[key]
    orc, x = _oracle(dev), xc.oracle(8)
    pr = no_xs(profiles("all")[i])
    run = lambda p: orc.run(p).o  # noqa: E731
    dT = {s: (run(_replace(pr, t=pr.t + s * xt.H_T)) - run(_replace(pr, t=pr.t - s * xt.H_T))) / (2 * s * xt.H_T) for s in (0.5, 1.0, 2.0)}
    res = types.SimpleNamespace(o=run(pr), dp=jt.richardson(run, pr, "p"), dt=((4 * dT[1.0] - dT[2.0]) / 3, (4 * dT[0.5] - dT[1.0]) / 3),
                                unit=[], xp=[], xtt=[])
    fz = xt.frozen(i)
    amounts = x.profs["all"][i].xamnt
    res.unit = [x.odx[f"only{m}"][i] / amounts[:, m:m + 1] for m in range(NX)]
    res.xp, res.xtt = ([[np.asarray(d[m], np.float64) for d in fz.richardson_units(var)] for m in range(NX)] for var in ("p", "t"))
    _REF[key] = res
    return res


def reference(dev, name: str, i: int, quantity: str):
    """-> namespace: o, odx [nlay, nwn], ko (longdouble), slots {variable: float64 [nlay, nwn]}, spread {variable: float or None}"""
    key = (name, i, quantity)
    if key in _REF:
        return _REF[key]
    b, pr = base_terms(dev, i), profiles(name)[i]
    xa = pr.xamnt
    term = [xa[:, m:m + 1] * b.unit[m] for m in range(NX)]
    odx = sum(term)
    o = b.o + odx
    adj = rtm_truth.truth_adjoint(pr.wn, [pr.nlay], [pr.irt], pr.t[None], pr.tz[None], o[None], [pr.tmpsfc], pr.emiss[None], pr.reflc[None],
                                  quantities=(quantity,))[quantity]
    ko, kt_planck = adj["k_o"][0], adj["k_t"][0]
    slots = {XS[m]: np.asarray(ko * term[m], np.float64) for m in range(NX)}
    spread = {v: None for v in XS}
    for var, d_modm, d_xs, planck in (("p", b.dp, b.xp, 0.0), ("t", b.dt, b.xtt, kt_planck)):
        both = [np.asarray(planck + ko * (d_modm[h] + sum(xa[:, m:m + 1] * d_xs[m][h] for m in range(NX))), np.float64) for h in (0, 1)]
        slots[var] = both[0]
        spread[var] = jt.rel_err(both[1], both[0], axis=-2, floor=jt.w_floor(both[0]))
    ref = types.SimpleNamespace(o=o, odx=odx, ko=ko, slots=slots, spread=spread)
    _REF[key] = ref
    return ref


def check(got, ref, var, what: str) -> float:
    r = ref.slots[var]
    bound = jt.TOL if ref.spread[var] is None else max(jt.TOL, 10.0 * ref.spread[var])
    e = jt.rel_err(got, r, axis=-2, floor=jt.w_floor(r))
    print(f"{what} {var}: peak {np.abs(r).max():.3e} error {e:.2e} bound {bound:.1e}"
          + ("" if ref.spread[var] is None else f" (self-spread {ref.spread[var]:.1e})"))
    assert e <= bound, f"{what} {var}: {e:.3e} > {bound:.1e}"
    return e


# ---- the GPU's results, once per session -----------------------------------------------------------------------------------------------
_GOT = {}
MOLS = XS + ("p",)


def jac(dev, name: str, quantity: str):
    key = (name, quantity)
    if key not in _GOT:
        _GOT[key] = dev.rt.jacobian(profiles(name), mols=MOLS, quantity=quantity, ixsect=1)
        for v in _GOT[key].values():
            v.setflags(write=False)
    return _GOT[key]


# ---- a. O -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_o_is_modm_with_cross_sections(dev, name):
    prs = profiles(name)
    o, *_, odx = dev.rt.modm(prs, ixsect=1)
    got = jac(dev, name, "tb")["o"]
    assert got.shape == o.shape == (3, max(xc.NLAYS), len(xc.WN))
    for i, p in enumerate(prs):
        e = np.abs(got[i, :p.nlay] - o[i, :p.nlay]) / np.abs(o[i, :p.nlay])
        ref = reference(dev, name, i, "tb")
        eo = np.abs(got[i, :p.nlay] - ref.o) / np.abs(ref.o)
        print(f"{name} profile {i}: O of jacobian(ixsect = 1) against modm(ixsect = 1) {e.max():.2e}, against the oracle {eo.max():.2e}; "
              f"ODXSEC / O up to {np.max(odx[i, :p.nlay] / o[i, :p.nlay]):.3g}")
        assert e.max() <= xc.TOL_SUM
        assert eo.max() <= 1e-9
        assert not got[i, p.nlay:].any()
    if name == "big":
        assert np.max(odx / np.where(o > 0, o, 1.0)) > 0.9, "the cross sections do not dominate O anywhere"


# ---- b. the slots of the cross-section molecules -------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", ["tb", "rad"])
@pytest.mark.parametrize("name", SETS)
def test_xs_slots(dev, name, quantity):
    got = jac(dev, name, quantity)
    assert got["vars"].tolist() == [api.JVAR_XS0 + m for m in range(NX)] + [api.JAC_VARS["p"]]
    odx = dev.rt.modm(profiles(name), ixsect=1)[4]
    for i, p in enumerate(profiles(name)):
        ref = reference(dev, name, i, quantity)
        kw = got["k_w"][i]
        for m in range(NX):
            check(kw[:p.nlay, m], ref, XS[m], f"{name} {quantity} profile {i}")
            assert not kw[:p.nlay, m][p.xamnt[:, m] == 0].any(), "a slot is not exactly 0 where XAMNT = 0"
        assert not kw[p.nlay:].any(), "padding layers"
        total, exp = kw[:p.nlay, :NX].sum(axis=1), got["k_o"][i, :p.nlay] * odx[i, :p.nlay]
        e = jt.rel_err(total, exp, axis=-2, floor=jt.w_floor(exp))
        print(f"{name} {quantity} profile {i}: the five slots against k_o x ODXSEC {e:.2e}")
        assert e <= 1e-12
    if name == "zeros":
        assert all(not got["k_w"][i, zero_layers(n), ZERO_MOL].any() and got["k_w"][i, 0, ZERO_MOL].any() for i, n in enumerate(xc.NLAYS))


# ---- c. k_t and the "p" slot ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quantity", [(n, "tb") for n in SETS] + [("big", "rad")])
def test_k_t_and_ln_p_include_the_cross_sections(dev, name, quantity):
    got = jac(dev, name, quantity)
    off = dev.rt.jacobian(profiles(name), mols=("p",), quantity=quantity)
    for i, p in enumerate(profiles(name)):
        ref = reference(dev, name, i, quantity)
        check(got["k_w"][i, :p.nlay, NX], ref, "p", f"{name} {quantity} profile {i}")
        check(got["k_t"][i, :p.nlay], ref, "t", f"{name} {quantity} profile {i}")
        assert not got["k_t"][i, p.nlay:].any()
    # the cross sections are a visible share of both: without them the same references are missed
    r0 = reference(dev, name, 0, quantity)
    miss = {"t": jt.rel_err(off["k_t"][0, :xc.NLAYS[0]], r0.slots["t"], axis=-2), "p": jt.rel_err(off["k_w"][0, :xc.NLAYS[0], 0], r0.slots["p"], axis=-2)}
    print(f"{name} {quantity} profile 0: the call with ixsect = 0 misses these references by {miss['t']:.2e} (k_t) and {miss['p']:.2e} (p)")
    assert miss["t"] > 1e-3
    if name == "big":
        assert miss["p"] > 1e-3


def test_per_state_launches_equal_the_extended_launch(dev):
    """Six profiles and five per-layer variables are 66 states: one MODM launch per state, ODXSEC of the base, T +- h and P (1 +- eps)
    in slots of their own, the molecules' and WBRODL's states without cross sections.  Against the three-profile call (one extended
    launch of 15 states) and the same references."""
    prs = profiles("big")
    mols = (1, XS[3], "wbrod", "p", 2, XS[0], 3)
    got = dev.rt.jacobian(prs + prs, mols=mols, ixsect=1)
    ext = jac(dev, "big", "tb")
    for i, p in enumerate(prs + prs):
        ref, n = reference(dev, "big", i % 3, "tb"), p.nlay
        check(got["k_w"][i, :n, 3], ref, "p", f"per-state profile {i}")
        check(got["k_t"][i, :n], ref, "t", f"per-state profile {i}")
        for slot, m in ((1, 3), (5, 0)):
            check(got["k_w"][i, :n, slot], ref, XS[m], f"per-state profile {i}")
            assert jt.rel_err(got["k_w"][i, :n, slot], ext["k_w"][i % 3, :n, m], axis=-2) <= 1e-12
        assert np.abs(got["o"][i, :n] / ext["o"][i % 3, :n] - 1).max() <= xc.TOL_SUM
    # a molecule's slot does not see the cross sections beyond k_o
    alone = dev.rt.jacobian(prs, mols=(1, 2, 3), ixsect=1)
    for j, s in enumerate((0, 4, 6)):
        assert jt.rel_err(got["k_w"][:3, :, s], alone["k_w"][:, :, j], axis=1, floor=jt.w_floor(alone["k_w"][:, :, j])) <= 1e-9


# ---- d. scan and obs ---------------------------------------------------------------------------------------------------------------
def scan_path():
    lm = max(xc.NLAYS)
    return PATHS[:, None] * np.ones((1, lm))


def test_scan_and_obs(dev):
    rt, prs = dev.rt, profiles("all")
    path = scan_path()
    sc = rt.scan_jacobian(prs, path, mols=MOLS, ixsect=1)
    one = jac(dev, "all", "tb")
    assert sc["k_w"].shape == (3, 3, max(xc.NLAYS), NX + 1, len(xc.WN))
    np.testing.assert_array_equal(sc["o"], one["o"])
    for k in ("tb", "rad", "k_t", "k_tz", "k_w", "k_clw", "k_o", "k_sfc"):
        np.testing.assert_array_equal(sc[k][:, 0], one[k], err_msg=k)
    x = xc.oracle(8)
    for i, p in enumerate(prs):
        for j in range(len(PATHS)):
            for m in range(NX):
                exp = sc["k_o"][i, j, :p.nlay] * x.odx[f"only{m}"][i]
                e = jt.rel_err(sc["k_w"][i, j, :p.nlay, m], exp, axis=-2, floor=jt.w_floor(exp))
                print(f"scan profile {i} path {j} {XS[m]}: against k_o x the oracle's term {e:.2e}")
                assert e <= 1e-12
    op = api.ObsOperator(np.array([0, 2, 3], np.int32), np.array([0.6, 0.4, 1.0]), (np.arange(len(xc.WN)) % 10).astype(np.int32),
                         np.full(len(xc.WN), 0.1), nchan=10)
    mono = dict(sc, y=sc["tb"])
    with toj.handle(rt, op) as h:
        ob = rt.obs_jacobian(prs, path, h, mols=MOLS, ixsect=1)
    np.testing.assert_array_equal(ob["o"], sc["o"])
    toj.check_full(ob, mono, op, toj.TOL8, "obs_jacobian(ixsect = 1)")


# ---- e. ixsect = 0 ------------------------------------------------------------------------------------------------------------------
def test_ixsect_0_is_the_entry_without_cross_sections(dev):
    rt, prs = dev.rt, profiles("all")
    path, mols = scan_path(), (1, "p", "xself", 2)
    op = api.ObsOperator(np.array([0, 2, 3], np.int32), np.array([0.6, 0.4, 1.0]), (np.arange(len(xc.WN)) % 10).astype(np.int32),
                         np.full(len(xc.WN), 0.1), nchan=10)
    with toj.handle(rt, op) as h:
        pairs = [(rt.jacobian(prs, mols=mols), rt.jacobian(prs, mols=mols, ixsect=0, xs_entry=True)),
                 (rt.scan_jacobian(prs, path, mols=mols), rt.scan_jacobian(prs, path, mols=mols, ixsect=0, xs_entry=True)),
                 (rt.obs_jacobian(prs, path, h, mols=mols), rt.obs_jacobian(prs, path, h, mols=mols, ixsect=0, xs_entry=True))]
    for old, new in pairs:
        assert set(old) == set(new)
        for k in old:
            np.testing.assert_array_equal(old[k], new[k], err_msg=k)
    assert np.any(pairs[0][0]["k_w"] != 0)


# ---- f. reproducibility and allocation -----------------------------------------------------------------------------------------------
def test_twice_the_same_bits(dev):
    a = dev.rt.jacobian(profiles("zeros"), mols=MOLS, ixsect=1)
    for k, v in jac(dev, "zeros", "tb").items():
        np.testing.assert_array_equal(a[k], v, err_msg=k)


def test_second_device_call_allocates_nothing(dev):
    """monortm_hip_jacobian_xs_dev under graph capture (an allocation would end the capture with an error), as
    tests/test_jacobian_vars.py captures the entries of its variables: one warm call, the capture, a replay into cleared outputs."""
    import torch

    rt, prs = dev.rt, profiles("all")
    ref = jac(dev, "all", "tb")
    n, lm, nw, nmol = 3, max(xc.NLAYS), len(xc.WN), prs[0].nmol
    cuda = torch.device("cuda")

    def pack(get, *tail):
        out = np.zeros((n, lm) + tail)
        for i, p in enumerate(prs):
            out[i, : p.nlay] = get(p)
        return torch.from_numpy(out).to(cuda)

    P, T, CLW, WB = (pack(lambda p, k=k: getattr(p, k)) for k in ("p", "t", "clw", "wbrodl"))
    WKL, XA = pack(lambda p: p.wkl, nmol), pack(lambda p: p.xamnt, NX)
    TZ = torch.zeros(n, lm + 1, dtype=torch.float64, device=cuda)
    for i, p in enumerate(prs):
        TZ[i, : p.nlay + 1] = torch.from_numpy(p.tz).to(cuda)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=cuda)  # noqa: E731
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(cuda)  # noqa: E731
    nlay, irt, wn = i32([p.nlay for p in prs]), i32([p.irt for p in prs]), f64(xc.WN)
    ts, em, rf = f64([p.tmpsfc for p in prs]), f64(np.stack([p.emiss for p in prs])), f64(np.stack([p.reflc for p in prs]))
    jm = api.jac_codes(MOLS, xc.NAMES)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=cuda)  # noqa: E731
    out = dict(o=z(n, lm, nw), rad=z(n, nw), tb=z(n, nw), k_t=z(n, lm, nw), k_tz=z(n, lm + 1, nw), k_w=z(n, lm, len(jm), nw),
               k_clw=z(n, lm, nw), k_o=z(n, lm, nw), k_sfc=z(n, 3, nw))
    fac, ends = np.ascontiguousarray(prs[0].cntnm, np.float64), np.array([xc.WN[0], xc.WN[-1]])
    d = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    h = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    p0 = prs[0]

    def call(stream):
        rt._chk(rt.lib.monortm_hip_jacobian_xs_dev(rt.ctx, n, nw, d(wn), p0.dvset, d(nlay), lm, nmol, d(P), d(T), d(CLW), d(WKL), d(WB), h(fac),
                                                   p0.sclcpl, p0.sclhw, p0.y0res, p0.ibrd, 1, d(XA), d(irt), d(TZ), d(ts), d(em), d(rf), 1, len(jm),
                                                   h(jm), *[d(out[k]) for k in api.JAC_FIELDS], h(ends), C.c_void_p(stream.cuda_stream)))

    def same():
        torch.cuda.synchronize()
        for k in api.JAC_FIELDS:
            np.testing.assert_array_equal(out[k].cpu().numpy(), ref[k], err_msg=k)

    call(torch.cuda.current_stream())
    same()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call(s)
    torch.cuda.current_stream().wait_stream(s)
    for k in api.JAC_FIELDS:
        out[k].zero_()
    g.replay()
    same()


# ---- g. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    import torch

    rt, prs = dev.rt, profiles("all")
    path = scan_path()
    op = api.ObsOperator(np.array([0, 2, 3], np.int32), np.array([0.6, 0.4, 1.0]), (np.arange(len(xc.WN)) % 10).astype(np.int32),
                         np.full(len(xc.WN), 0.1), nchan=10)
    launches = lambda r: sum(r.counter(k) for k in range(2, 8))   # noqa: E731  (one finish launch per MODM evaluation)
    xs0 = api.JVAR_XS0
    with toj.handle(rt, op) as h:
        entries = {"jacobian": lambda r, hh, **kw: r.jacobian(prs, **kw), "scan": lambda r, hh, **kw: r.scan_jacobian(prs, path, **kw),
                   "obs": lambda r, hh, **kw: r.obs_jacobian(prs, path, hh, **kw)}
        n0 = launches(rt)
        for name, f in entries.items():
            # a cross-section code with ixsect = 0: through the entry without cross sections, and through the _xs entry
            assert code(lambda: f(rt, h, mols=(xs0,))) == "EARG", name
            assert code(lambda: f(rt, h, mols=(1, xs0 + 2), xs_entry=True)) == "EARG", name
            # x >= nxs; the same variable twice; more than 39
            assert code(lambda: f(rt, h, mols=(xs0 + NX,), ixsect=1)) == "EARG", name
            assert code(lambda: f(rt, h, mols=(xs0 + 37,), ixsect=1)) == "EARG", name
            assert code(lambda: f(rt, h, mols=(xs0 + 38,), ixsect=1)) == "EARG", name
            assert code(lambda: f(rt, h, mols=(XS[1], xs0 + 1), ixsect=1)) == "EARG", name
            assert code(lambda: f(rt, h, mols=tuple(range(1, 8)) + tuple(xs0 + m for m in range(NX)) * 7, ixsect=1)) == "EARG", name
        with pytest.raises(ValueError):
            rt.jacobian(prs, mols=("xs:SF6",), ixsect=1)
        # XAMNT NULL, ixsect outside 0 / 1: the C entry itself
        a = rt.jacobian(prs, mols=XS[:1], ixsect=1)
        assert np.any(a["k_w"] != 0)
        n1 = launches(rt)
        assert n1 > n0
        real_xs = rt._jac_xs
        try:
            rt._jac_xs = lambda *a, **k: ("_xs", (1, None), None)
            assert code(lambda: rt.jacobian(prs, mols=XS[:1], ixsect=1)) == "EARG"
            rt._jac_xs = lambda *a, **k: ("_xs", (2, real_xs(prs, 1, False, max(xc.NLAYS))[1][1]), None)
            assert code(lambda: rt.scan_jacobian(prs, path, mols=(1,), ixsect=1)) == "EARG"
        finally:
            del rt._jac_xs
        # no tables on the context
        bare = api.MonoRTM(dev.t3, xc.WN[0], xc.WN[-1])
        r4 = api.MonoRTM(dev.t3, xc.WN[0], xc.WN[-1], real_kind=4)
        r4.set_xsec(xc.oracle(8).tabs)
        try:
            for name, f in entries.items():
                if name == "obs":
                    continue   # (a handle belongs to its context)
                assert code(lambda: f(bare, None, mols=(1,), ixsect=1)) == "EARG", name
                assert code(lambda: f(r4, None, mols=(1,), ixsect=1)) == "EUNSUPPORTED", name
                assert code(lambda: f(r4, None, mols=(xs0,), ixsect=1)) == "EUNSUPPORTED", name
            with toj.handle(r4, op) as h4:
                assert code(lambda: r4.obs_jacobian(prs, path, h4, mols=(1,), ixsect=1)) == "EUNSUPPORTED"
            with toj.handle(bare, op) as hb:
                assert code(lambda: bare.obs_jacobian(prs, path, hb, mols=(1,), ixsect=1)) == "EARG"
            torch.cuda.synchronize()
            assert launches(bare) == 0 and launches(r4) == 0
        finally:
            bare.close()
            r4.close()
        torch.cuda.synchronize()
        assert launches(rt) == n1, "a refused call launched something"
        # the context still works
        b = rt.jacobian(prs, mols=XS[:1], ixsect=1)
    np.testing.assert_array_equal(a["k_w"], b["k_w"])


# ---- h. multi-device ----------------------------------------------------------------------------------------------------------------
def test_multi_device_context_equals_one_device(dev, monkeypatch):
    """Three shards take the blocks (0, 1), (2, 3), (4, 5) of six profiles - each block holds a 10-layer profile, so every shard runs the
    batch shape of the one-device call on its two profiles alone - and return them bit for bit (tests/test_host_entries.py's rule)."""
    p = profiles("all")
    prs, path = [p[0], p[1], p[2], p[0], p[1], p[0]], scan_path()
    op = api.ObsOperator(np.array([0, 2, 3], np.int32), np.array([0.6, 0.4, 1.0]), (np.arange(len(xc.WN)) % 10).astype(np.int32),
                         np.full(len(xc.WN), 0.1), nchan=10)
    monkeypatch.setenv("MONORTM_DEVICES", "0,0,0")
    m = api.MonoRTM(dev.t3, xc.WN[0], xc.WN[-1], ngpu=0)
    try:
        assert m.lib.monortm_hip_device_count(m.ctx) == 3
        m.set_xsec(xc.oracle(8).tabs)
        with toj.handle(dev.rt, op) as h1, toj.handle(m, op) as h3:
            multi = (m.jacobian(prs, mols=MOLS, ixsect=1), m.scan_jacobian(prs, path, mols=MOLS, ixsect=1),
                     m.obs_jacobian(prs, path, h3, mols=MOLS, ixsect=1))
            for b in range(3):
                blk = prs[2 * b: 2 * b + 2]
                one = (dev.rt.jacobian(blk, mols=MOLS, ixsect=1), dev.rt.scan_jacobian(blk, path, mols=MOLS, ixsect=1),
                       dev.rt.obs_jacobian(blk, path, h1, mols=MOLS, ixsect=1))
                for got, exp, fields in zip(multi, one, (api.JAC_FIELDS, api.SCAN_JAC_FIELDS, api.OBS_JAC_FIELDS)):
                    for k in fields:
                        np.testing.assert_array_equal(got[k][2 * b: 2 * b + 2], exp[k], err_msg=f"{k} block {b}")
        assert np.any(multi[2]["k_w"][..., :NX, :] != 0)
    finally:
        m.close()
