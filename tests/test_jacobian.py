"""Jacobians of RAD / TB (monortm_hip_rtm_jac, monortm_hip_jacobian) on the GPU.

The adjoint of RTM against central differences of the CPU oracle's RTM; the layer-diagonal Jacobian against per-layer brute force
(every perturbed profile changes ONE layer: what shows that layers do not interact in MODM), on the GPU and end to end against the
oracle; a sum rule; step halving; consistency with modm / rtm, padding, sharding, DeviceBatch and graph replay; errors."""
import copy
import ctypes as C

import numpy as np
import pytest

from monortm_amd import api, synth, tape3

pytestmark = pytest.mark.gpu

FIELDS_RTM = ("k_o", "k_t", "k_tz")


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


@pytest.fixture(scope="module")
def case(workdir, gpu):
    """A line list with coupled and speed-dependent lines, the c2 channels plus the sounder channels."""
    rec = synth.synthetic_lines(300, seed=777, lc_frac=0.5, sdep_frac=0.2)
    t3 = f"{workdir}/TAPE3_jac"
    tape3.write_tape3(t3, rec)
    wn = np.unique(np.concatenate([synth.c2_channels(12, seed=11), synth.sounder_channels()]))
    rt = api.MonoRTM(t3, wn[0], wn[-1])
    yield t3, wn, rt
    rt.close()


def profiles(wn, ids, nlay, irt=(1, 3), cloud=True):
    nl = nlay if isinstance(nlay, (list, tuple)) else [nlay] * len(ids)
    return [synth.perturbed_profile(i, wn, nlay=n, cloud=cloud, irt=irt[j % len(irt)]) for j, (i, n) in enumerate(zip(ids, nl))]


def rel_err(k, ref, axis, floor=0.0):
    """max |k - ref| relative to max |ref| over `axis` (the layer / level axis): per (profile, channel).  `floor` (broadcast against
    the scale) bounds the scale from below."""
    scale = np.maximum(np.abs(ref).max(axis=axis, keepdims=True), floor)
    return float(np.max(np.abs(k - ref) / np.where(scale > 0, scale, 1.0)))


def w_floor(kw):
    """Scale floor of a K_W comparison: 1e-3 of the species' peak |K_W| in the profile (all layers and channels).  Differences of TB
    resolve d TB / d ln WKL only to ~10 ulp(TB) / (2 eps) ~ 3e-9 K, i.e. 1e-4 of a weak species' K_W in a channel where it hardly
    absorbs; such channels are checked to 1e-8 of the species' peak instead."""
    return 1e-2 * float(np.abs(kw).max())


def _orc_rtm(pr, o, quantity):
    from oracle.pyoracle import lib

    nwn = pr.nwn
    rup, rdn, trtot, rad, tb = (np.zeros(nwn) for _ in range(5))
    ts = C.c_double(pr.tmpsfc)
    lib().orc_rtm(1, pr.irt, nwn, pr.wn, pr.nlay, np.ascontiguousarray(pr.t), np.ascontiguousarray(pr.tz), np.ascontiguousarray(o),
                  C.byref(ts), rup, trtot, rdn, np.ascontiguousarray(pr.reflc), np.ascontiguousarray(pr.emiss), rad, tb)
    return tb if quantity == "tb" else rad


# ---- 1. the adjoint of RTM against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("irt", [1, 2, 3])
@pytest.mark.parametrize("quantity", ["tb", "rad"])
def test_rtm_adjoint_matches_oracle_differences(case, irt, quantity):
    _, wn, rt = case
    pr = synth.perturbed_profile(300 + irt, wn, nlay=20, cloud=True, irt=irt)
    if irt != 1:
        pr.tmpsfc, pr.emiss, pr.reflc = 280.0, np.full(len(wn), 0.7), np.full(len(wn), 0.3)   # ignored by RTM for irt = 2, 3
    O = rt.modm([pr])[0]
    res = rt.rtm_jacobian([pr], O, quantity)
    o = O[0]
    f = lambda p, oo: _orc_rtm(p, oo, quantity)  # noqa: E731

    def cd(setter, h):   # central differences at h and 2h, Richardson-extrapolated (truncation O(h^4))
        d = []
        for hh in (h, 2 * h):
            a, b = copy.deepcopy(pr), copy.deepcopy(pr)
            oa, ob = o.copy(), o.copy()
            setter(a, oa, hh)
            setter(b, ob, -hh)
            d.append((f(a, oa) - f(b, ob)) / (2 * hh))
        return (4 * d[0] - d[1]) / 3

    n = pr.nlay
    ref = {"k_o": np.zeros((n, len(wn))), "k_t": np.zeros((n, len(wn))), "k_tz": np.zeros((n + 1, len(wn)))}
    for k in range(n):
        hk = 1e-4 * max(float(o[k].max()), 1.0)
        ref["k_o"][k] = cd(lambda p, oo, h, k=k: oo[k].__iadd__(h), hk)
        ref["k_t"][k] = cd(lambda p, oo, h, k=k: p.t.__setitem__(k, p.t[k] + h), 0.1)   # (0.1 K: rounding of TB, not truncation, limits)
    for j in range(n + 1):
        ref["k_tz"][j] = cd(lambda p, oo, h, j=j: p.tz.__setitem__(j, p.tz[j] + h), 0.1)
    for name in FIELDS_RTM:
        got = res[name][0]
        e = rel_err(got, ref[name], axis=0)
        assert e <= 1e-6, f"irt={irt} {quantity} {name}: {e:.2e}"
    assert np.all(res["k_o"][0] != 0)
    if irt == 3:
        assert np.all(res["k_tz"][0, n] == 0)
    sfc = [cd(lambda p, oo, h: setattr(p, "tmpsfc", p.tmpsfc + h), 0.1), cd(lambda p, oo, h: setattr(p, "emiss", p.emiss + h), 1e-3),
           cd(lambda p, oo, h: setattr(p, "reflc", p.reflc + h), 1e-3)]
    for i in range(3):
        got = res["k_sfc"][0, i]
        if irt == 1:
            assert np.max(np.abs(got - sfc[i])) <= 1e-6 * np.abs(sfc[i]).max(), f"k_sfc[{i}]"
        else:
            assert np.all(got == 0) and np.all(np.abs(sfc[i]) <= 1e-9 * np.abs(res["k_o"][0]).max()), f"irt={irt} k_sfc[{i}]"
    ref_rad = rt.rtm([pr], O)
    np.testing.assert_allclose(res["rad"][0], ref_rad[3][0], rtol=1e-12)
    np.testing.assert_allclose(res["tb"][0], ref_rad[4][0], rtol=1e-12)


def test_rtm_adjoint_single_precision(case):
    """real_kind 4: float arrays, double arithmetic - the same K to float rounding."""
    t3, wn, rt = case
    prs = profiles(wn, [310, 311, 312], 20, irt=(1, 2, 3))
    O = rt.modm(prs)[0]
    ref = rt.rtm_jacobian(prs, O)
    r4 = api.MonoRTM(t3, wn[0], wn[-1], real_kind=4)
    got = r4.rtm_jacobian(prs, O.astype(np.float32))
    r4.close()
    for name in FIELDS_RTM:
        assert got[name].dtype == np.float32
        assert rel_err(got[name].astype(np.float64), ref[name], axis=1) <= 1e-4, name


# ---- 2. / 3. the layer-diagonal Jacobian against per-layer brute force --------------------------------------------------------
def brute_force(run, prs, mols, quantity="tb", clw_step=1e-4, dlnw=api.JAC_DLNW):
    """Central differences with the API's steps, every perturbed profile changing ONE layer; all of them in one batch per profile."""
    out = []
    for pr in prs:
        batch, n = [], pr.nlay
        for k in range(n):
            for sgn in (1, -1):
                t = pr.t.copy()
                t[k] += sgn * api.JAC_DT
                batch.append(_replace(pr, t=t))
            for m in mols:
                for sgn in (1, -1):
                    w = pr.wkl.copy()
                    w[k, m - 1] *= 1 + sgn * dlnw
                    batch.append(_replace(pr, wkl=w))
            for sgn in (1, -1):   # (O is linear in CLW: a central difference; a layer without cloud goes to -step, which MODM takes)
                c = pr.clw.copy()
                c[k] += sgn * clw_step
                batch.append(_replace(pr, clw=c))
        got = run(batch)
        q = np.array([getattr(d, quantity) for d in got])
        per = 2 + 2 * len(mols) + 2
        kt = np.array([(q[k * per] - q[k * per + 1]) / (2 * api.JAC_DT) for k in range(n)])
        kw = np.array([[(q[k * per + 2 + 2 * i] - q[k * per + 3 + 2 * i]) / (2 * dlnw) for i in range(len(mols))] for k in range(n)])
        kc = np.array([(q[k * per + per - 2] - q[k * per + per - 1]) / (2 * clw_step) for k in range(n)])
        out.append((kt, kw, kc))
    return out


def _replace(pr, **kw):
    p = copy.deepcopy(pr)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_jacobian_matches_per_layer_brute_force_gpu(case):
    _, wn, rt = case
    prs = profiles(wn, [400, 401], [24, 17], irt=(1, 3))
    # WKL x (1 +- 3e-4) on both sides (set_option).  The brute force differences RTM itself: at the default 1e-4 TB's rounding is 1e-6
    # of O3's K_W where O3 hardly absorbs; at 1e-3 RTM's curvature (~(eps O_k)^2) is 1e-6 of H2O's where H2O is opaque
    try:
        rt.set_option("jac_dlnw", 3e-4)
        res = rt.jacobian(prs, mols=(1, 3))
    finally:
        rt.set_option("jac_dlnw", "auto")
    bf = brute_force(rt.run, prs, (1, 3), dlnw=3e-4)
    errs = {}
    for p, (pr, (kt, kw, kc)) in enumerate(zip(prs, bf)):
        n = pr.nlay
        errs[f"{p} k_t"] = rel_err(res["k_t"][p, :n], kt, axis=0)
        for i in range(2):
            errs[f"{p} k_w[{i}]"] = rel_err(res["k_w"][p, :n, i], kw[:, i], axis=0, floor=w_floor(kw[:, i]))
        errs[f"{p} k_clw"] = rel_err(res["k_clw"][p, :n], kc, axis=0)
        assert np.any(pr.clw == 0) and np.all(res["k_clw"][p, :n][pr.clw == 0] != 0)   # closed form: right where CLW = 0 too
    assert max(errs.values()) <= 1e-6, errs


def test_jacobian_matches_oracle_end_to_end(case):
    from oracle.pyoracle import Oracle

    t3, wn, rt = case
    prs = profiles(wn, [410], 12, irt=(1,))
    res = rt.jacobian(prs, mols=(1,))
    orc = Oracle(t3, wn[0], wn[-1])
    (kt, kw, kc), = brute_force(lambda b: [orc.run(p) for p in b], prs, (1,))
    orc.close()
    assert rel_err(res["k_t"][0, :12], kt, axis=0) <= 1e-5
    assert rel_err(res["k_w"][0, :12, 0], kw[:, 0], axis=0, floor=w_floor(kw[:, 0])) <= 1e-5
    assert rel_err(res["k_clw"][0, :12], kc, axis=0) <= 1e-5


# ---- 4. sum rule, 5. step halving -------------------------------------------------------------------------------------------
def test_sum_rule_uniform_temperature_shift(case):
    _, wn, rt = case
    prs = profiles(wn, [420, 421], 20, irt=(1, 3))
    res = rt.jacobian(prs, mols=())
    # the Jacobian's own step: every layer's O then sees exactly the temperatures of the Jacobian's T +- h states (MODM is layer-
    # diagonal), so a line-shape switch crossed within +-h is crossed on both sides alike; what remains is RTM's curvature
    d = api.JAC_DT
    shifted = []
    for pr in prs:
        for sgn in (1, -1):
            shifted.append(_replace(pr, t=pr.t + sgn * d, tz=pr.tz + sgn * d))
    tb = np.array([x.tb for x in rt.run(shifted)])
    for p in range(len(prs)):
        fd = (tb[2 * p] - tb[2 * p + 1]) / (2 * d)
        s = res["k_t"][p].sum(axis=0) + res["k_tz"][p].sum(axis=0)
        # relative to the profile's largest sum: in some channels the Planck and optical-depth terms of K_T cancel to 1e-5 of either,
        # and the ~1e-8 truncation of the MODM differences is relative to those terms, not to their sum
        assert np.max(np.abs(s - fd)) <= 1e-6 * np.abs(fd).max(), p


def test_step_halving(case):
    _, wn, rt = case
    prs = profiles(wn, [430, 431], 20, irt=(1, 3))
    a = rt.jacobian(prs, mols=(1, 3))
    try:
        rt.set_option("jac_dt", api.JAC_DT / 2)
        rt.set_option("jac_dlnw", api.JAC_DLNW / 2)
        b = rt.jacobian(prs, mols=(1, 3))
    finally:
        rt.set_option("jac_dt", "auto")
        rt.set_option("jac_dlnw", "auto")
    assert rel_err(b["k_t"], a["k_t"], axis=1) <= 1e-6
    for p in range(len(prs)):
        for i in range(2):
            assert rel_err(b["k_w"][p, :, i], a["k_w"][p, :, i], axis=0, floor=w_floor(a["k_w"][p, :, i])) <= 1e-6, (p, i)
    c = rt.jacobian(prs, mols=(1, 3))
    assert np.array_equal(c["k_t"], a["k_t"])   # "auto" restores the defaults


# ---- 6. consistency ------------------------------------------------------------------------------------------------------------
def test_forward_outputs_equal_modm_rtm(case):
    _, wn, rt = case
    prs = profiles(wn, [440, 441, 442], [20, 16, 18], irt=(1, 3, 2))
    res = rt.jacobian(prs, mols=(1,))
    O = rt.modm(prs)[0]
    r = rt.rtm(prs, O)
    np.testing.assert_allclose(res["o"], O, rtol=1e-12, atol=0)
    np.testing.assert_allclose(res["rad"], r[3], rtol=1e-12)
    np.testing.assert_allclose(res["tb"], r[4], rtol=1e-12)


def test_mixed_nlay_equals_single_profiles(case):
    _, wn, rt = case
    prs = profiles(wn, [450, 451, 452], [24, 13, 19], irt=(1, 3))
    res = rt.jacobian(prs, mols=(1, 3))
    for p, pr in enumerate(prs):
        one = rt.jacobian([pr], mols=(1, 3))
        n = pr.nlay
        # (the two calls run MODM on batches of different sizes: O agrees to rounding, which the differences divide by h)
        for name, tol in (("k_t", 1e-9), ("k_clw", 1e-12), ("k_o", 1e-12), ("k_w", 1e-9)):
            fl = w_floor(one[name][0]) if name == "k_w" else 0.0
            assert rel_err(res[name][p, :n], one[name][0], axis=0, floor=fl) <= tol, (p, name)
            assert np.all(res[name][p, n:] == 0), (p, name, "padding")
        assert rel_err(res["k_tz"][p, : n + 1], one["k_tz"][0], axis=0) <= 1e-9
        assert np.all(res["k_tz"][p, n + 1:] == 0)
        np.testing.assert_allclose(res["tb"][p], one["tb"][0], rtol=1e-12)


def test_multi_device_context_equals_one_device(case, monkeypatch):
    t3, wn, rt = case
    prs = profiles(wn, [460, 461, 462], 18, irt=(1, 3))
    one = rt.jacobian(prs, mols=(1,))
    O = rt.modm(prs)[0]
    one_r = rt.rtm_jacobian(prs, O)
    monkeypatch.setenv("MONORTM_DEVICES", "0,0")
    m = api.MonoRTM(t3, wn[0], wn[-1], ngpu=0)
    assert m.lib.monortm_hip_device_count(m.ctx) == 2
    m.set_option("jac_dt", api.JAC_DT)   # passed on to every shard
    two = m.jacobian(prs, mols=(1,))
    two_r = m.rtm_jacobian(prs, O)
    m.close()
    for name in api.JAC_FIELDS:
        assert rel_err(two[name], one[name], axis=1 if one[name].ndim > 2 else 0) <= 1e-12, name
    for name in ("rad", "tb", "k_o", "k_t", "k_tz", "k_sfc"):
        assert np.array_equal(two_r[name], one_r[name]), name


def test_device_batch_and_graph_replay(case):
    import torch

    _, wn, rt = case
    prs = profiles(wn, [470, 471], 20, irt=(1, 3))
    ref = rt.jacobian(prs, mols=(1, 3))
    db = api.DeviceBatch(rt, prs)
    got = db.jacobian(mols=(1, 3))
    torch.cuda.synchronize()
    db.check()
    for name in api.JAC_FIELDS:
        assert rel_err(got[name].cpu().numpy(), ref[name], axis=1 if ref[name].ndim > 2 else 0) <= 1e-12, name
    first = {k: v.cpu().numpy().copy() for k, v in got.items()}
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            db.jacobian(mols=(1, 3))
    torch.cuda.current_stream().wait_stream(s)
    for v in got.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for name in api.JAC_FIELDS:
        assert np.array_equal(got[name].cpu().numpy(), first[name]), name


def test_jacobian_between_modm_and_rtm_changes_nothing(case):
    _, wn, rt = case
    prs = profiles(wn, [480, 481], 20, irt=(1, 3))
    O = rt.modm(prs)[0]
    tb0 = rt.rtm(prs, O)[4]
    O = rt.modm(prs)[0]
    rt.jacobian(prs, mols=(1,))
    rt.rtm_jacobian(prs, O)
    tb1 = rt.rtm(prs, O)[4]
    assert np.array_equal(tb0, tb1)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------
def code(fn):
    with pytest.raises(api.MonoRTMError) as e:
        fn()
    return api.ERRORS[e.value.code]


def test_errors(case):
    t3, wn, rt = case
    prs = profiles(wn, [490], 16)
    r4 = api.MonoRTM(t3, wn[0], wn[-1], real_kind=4)
    assert code(lambda: r4.jacobian(prs)) == "EUNSUPPORTED"
    r4.close()
    for mols in ((0,), (8,), (1, 1)):
        assert code(lambda: rt.jacobian(prs, mols=mols)) == "EARG", mols
    assert code(lambda: rt.jacobian(prs, quantity=2)) == "EARG"
    O = rt.modm(prs)[0]
    assert code(lambda: rt.rtm_jacobian(prs, O, quantity=-1)) == "EARG"
    for v in ("0", "-1", "abc", "nan", "inf", "1e-2x"):
        assert code(lambda: rt.set_option("jac_dt", v)) == "EARG", v
    assert code(lambda: rt.set_option("jac_dlnw", "1")) == "EARG"
    cold = _replace(prs[0], t=prs[0].t.copy())
    cold.t[3] = 70.0 + 0.5 * api.JAC_DT
    assert code(lambda: rt.jacobian([cold])) == "ETEMP"
    # NULL outputs
    pr = prs[0]
    n, nw = pr.nlay, pr.nwn
    z = lambda *s: np.zeros(s)  # noqa: E731
    nl, irt = np.array([n], np.int32), np.array([pr.irt], np.int32)
    ts, em, rf = np.array([pr.tmpsfc]), pr.emiss[None], pr.reflc[None]
    P = api._ptr
    outs = [z(1, nw), z(1, nw), z(1, n, nw), z(1, n, nw), z(1, n + 1, nw), z(1, 3, nw)]
    for drop in range(len(outs)):
        ptrs = [None if i == drop else P(o) for i, o in enumerate(outs)]
        rc = rt.lib.monortm_hip_rtm_jac(rt.ctx, 1, nw, P(pr.wn), P(nl), n, P(irt), 1, P(pr.t[None].copy()), P(pr.tz[None].copy()),
                                        P(np.ascontiguousarray(O)), P(ts), P(np.ascontiguousarray(em)), P(np.ascontiguousarray(rf)), *ptrs)
        assert api.ERRORS[rc] == "EARG", drop
    wkl, jm = np.ascontiguousarray(pr.wkl[None]), np.array([1], np.int32)
    jouts = [z(1, n, nw), z(1, nw), z(1, nw), z(1, n, nw), z(1, n + 1, nw), z(1, n, 1, nw), z(1, n, nw), z(1, n, nw), z(1, 3, nw)]
    for drop in (0, 1, 2, 3, 4, 5, 6, 8):   # (K_O, index 7, may be NULL)
        ptrs = [None if i == drop else P(o) for i, o in enumerate(jouts)]
        rc = rt.lib.monortm_hip_jacobian(rt.ctx, 1, nw, P(pr.wn), pr.dvset, P(nl), n, pr.nmol, P(pr.p[None].copy()), P(pr.t[None].copy()),
                                         P(pr.clw[None].copy()), P(wkl), P(pr.wbrodl[None].copy()), P(pr.cntnm), pr.sclcpl, pr.sclhw,
                                         pr.y0res, pr.ibrd, P(irt), P(pr.tz[None].copy()), P(ts), P(np.ascontiguousarray(em)),
                                         P(np.ascontiguousarray(rf)), 1, 1, P(jm), *ptrs)
        assert api.ERRORS[rc] == "EARG", drop
    # the context still works after every refusal
    assert np.all(np.isfinite(rt.jacobian(prs, mols=(1,))["k_t"]))
