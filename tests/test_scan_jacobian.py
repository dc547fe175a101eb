"""Jacobians of path scans on the GPU (monortm_hip_rtm_scan_jac, monortm_hip_scan_jacobian and their _dev forms,
rtm_scan_jac_kernel.hip): K along npath paths per profile from ONE set of optical depths and ONE set of
perturbed MODM states - against monortm_hip_rtm_jac per path on optical depths the test scaled itself, against differences of the
CPU oracle, against MonoRTM.jacobian on profiles with scaled amounts, and the plumbing around it.

Synthetic inputs are seeded as in tests/test_scan.py; 70 wavenumbers = one full block of 64 lanes and one with 6 live lanes.  The
kernel holds NP = 4 paths per thread: npath = 1 is a short tile, 5 = 4 + 1, 9 = 4 + 4 + 1."""
import copy
import ctypes as C

import numpy as np
import pytest

from monortm_amd import api, synth, tape3

pytestmark = pytest.mark.gpu

NWN = 70
NP = 4                                   # SCAN_JAC_NP of rtm_scan_jac_kernel.hip
NPATHS = (1, NP + 1, 2 * NP + 1)
EARG = 6
FACTORS9 = [1.0, 1.3, 2.0, 5.76, 19.1, 1.05, 3.3, 0.7, 11.0]   # FACTORS9 of tests/test_scan.py
BATCHES = {
    "R30": [1, 2, 7, 30],   # nlay_max >= 24 -> G = 8, with empty layer groups and one-layer profiles
    "B30": [5, 24, 30],     # G = 8
    "C12": [3, 12],         # nlay_max < 24 -> G = 2
}
RTM_OUT = api.SCAN_JAC_RTM_FIELDS        # rad, tb, k_o, k_path, k_t, k_tz, k_sfc: the output order of monortm_hip_rtm_scan_jac
FULL_OUT = api.SCAN_JAC_FIELDS           # o, rad, tb, k_t, k_tz, k_w, k_clw, k_o, k_path, k_sfc: of monortm_hip_scan_jacobian
FILL = -7.0


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


@pytest.fixture(scope="module")
def rt(gpu):
    """The adjoint needs no line table: a context without TAPE3."""
    r = api.MonoRTM("", 0.0, 0.0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rt4(gpu):
    r = api.MonoRTM("", 0.0, 0.0, real_kind=4)
    yield r
    r.close()


@pytest.fixture(scope="module")
def case(workdir, gpu):
    """The line list and channels of tests/test_jacobian.py::case."""
    t3 = f"{workdir}/TAPE3_scan_jac"
    tape3.write_tape3(t3, synth.synthetic_lines(300, seed=777, lc_frac=0.5, sdep_frac=0.2))
    wn = np.unique(np.concatenate([synth.c2_channels(12, seed=11), synth.sounder_channels()]))
    r = api.MonoRTM(t3, wn[0], wn[-1])
    yield t3, wn, r
    r.close()


class Batch:
    """Seeded RTM inputs of a ragged batch (tests/test_scan.py::Batch); pad(x, v) fills what lies beyond nlay[p] (levels beyond
    nlay[p] + 1) with v."""

    def __init__(self, nlay, seed, nwn=NWN, irt=(1, 2, 3)):
        rng = np.random.default_rng(seed)
        self.nlay = np.array(nlay, np.int32)
        self.nprof, self.lm, self.nwn = len(nlay), int(max(nlay)), nwn
        n, lm = self.nprof, self.lm
        self.irt = np.array([irt[i % len(irt)] for i in range(n)], np.int32)
        self.wn = np.linspace(15.0, 250.0, nwn)
        self.O = np.clip(np.exp(rng.normal(np.log(7e-3), 1.6, (n, lm, nwn))), 1e-5, 5.0)
        self.T = rng.uniform(200.0, 300.0, (n, lm))
        self.TZ = rng.uniform(200.0, 300.0, (n, lm + 1))
        self.ts = rng.uniform(270.0, 310.0, n)
        self.em = rng.uniform(0.6, 1.0, (n, nwn))
        self.rf = 1.0 - self.em
        self.lay = np.arange(lm)[None, :] < self.nlay[:, None]          # [nprof, lm] active layers
        self.lev = np.arange(lm + 1)[None, :] <= self.nlay[:, None]     # [nprof, lm + 1] active levels

    def pad(self, x, v):
        x = np.array(x, np.float64)
        if x.ndim == 2:                                                # T [nprof, lm] or TZ [nprof, lm + 1]
            x[~(self.lay if x.shape[1] == self.lm else self.lev)] = v
        elif x.shape[1:] == (self.lm, self.nwn):                       # O [nprof, lm, nwn]
            x[~self.lay] = v
        else:                                                          # path [nprof, npath, lm]
            x[np.broadcast_to(~self.lay[:, None, :], x.shape)] = v
        return x

    def path(self, factors, slope=0.01):
        """[nprof, npath, lm]: factors[j] times a mild per-layer slope."""
        l = np.arange(self.lm) / max(self.lm - 1, 1)
        f = np.asarray(factors, np.float64)[:, None] * (1.0 + slope * l)[None, :]
        return np.ascontiguousarray(np.broadcast_to(f[None], (self.nprof,) + f.shape))


def rel_err(k, ref, axis, floor=0.0):
    """rel_err of tests/test_jacobian.py: max |k - ref| relative to max |ref| over `axis` (the layer / level axis)."""
    scale = np.maximum(np.abs(ref).max(axis=axis, keepdims=True), floor)
    return float(np.max(np.abs(k - ref) / np.where(scale > 0, scale, 1.0)))


def w_floor(kw):
    """Scale floor of a K_W comparison (tests/test_jacobian.py): 1e-2 of the species' peak |K_W| in the profile."""
    return 1e-2 * float(np.abs(kw).max())


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def err(r):
    return r.lib.monortm_hip_last_error(r.ctx)


def shapes(b, npath):
    n, lm, nw = b.nprof, b.lm, b.nwn
    return dict(rad=(n, npath, nw), tb=(n, npath, nw), k_o=(n, npath, lm, nw), k_path=(n, npath, lm, nw), k_t=(n, npath, lm, nw),
                k_tz=(n, npath, lm + 1, nw), k_sfc=(n, npath, 3, nw))


def raw_rtm_jac(r, b, O, quantity, em=None, rf=None):
    """monortm_hip_rtm_jac on the batch with optical depths O, zero padding -> dict of its six outputs."""
    dt = r.dtype
    c = lambda x: np.ascontiguousarray(x, dt)  # noqa: E731
    n, lm, nw = b.nprof, b.lm, b.nwn
    out = dict(rad=np.zeros((n, nw), dt), tb=np.zeros((n, nw), dt), k_o=np.zeros((n, lm, nw), dt), k_t=np.zeros((n, lm, nw), dt),
               k_tz=np.zeros((n, lm + 1, nw), dt), k_sfc=np.zeros((n, 3, nw), dt))
    T, TZ, O, ts = c(b.pad(b.T, 0.0)), c(b.pad(b.TZ, 0.0)), c(O), c(b.ts)
    em, rf = c(b.em if em is None else em), c(b.rf if rf is None else rf)
    rc = r.lib.monortm_hip_rtm_jac(r.ctx, n, nw, _p(b.wn), _p(b.nlay), lm, _p(b.irt), quantity, _p(T), _p(TZ), _p(O), _p(ts), _p(em), _p(rf),
                                   *[_p(out[k]) for k in ("rad", "tb", "k_o", "k_t", "k_tz", "k_sfc")])
    assert rc == 0, err(r)
    return out


def raw_scan_jac(r, b, path, quantity, O=None, em=None, rf=None, T=None, TZ=None, sfc=None, drop=(), **over):
    """monortm_hip_rtm_scan_jac -> (rc, dict of outputs pre-filled with FILL).  drop: names of arrays passed as NULL; over: nprof /
    npath / nwn / nlay_max / sfc_per_path handed to the call instead of the arrays' own."""
    dt = r.dtype
    c = lambda x: np.ascontiguousarray(x, dt)  # noqa: E731
    path = c(path)
    npath = path.shape[1]
    a = dict(wn=b.wn, nlay=b.nlay, irt=b.irt, T=c(b.pad(b.T, 0.0) if T is None else T), TZ=c(b.pad(b.TZ, 0.0) if TZ is None else TZ),
             O=c(b.pad(b.O, 0.0) if O is None else O), path=path, ts=c(b.ts), em=c(b.em if em is None else em),
             rf=c(b.rf if rf is None else rf))
    outs = {k: np.full(s, FILL, dt) for k, s in shapes(b, npath).items()}
    if sfc is None:
        sfc = int(a["em"].ndim == 3)
    g = lambda k: None if k in drop else _p(a[k] if k in a else outs[k])  # noqa: E731
    rc = r.lib.monortm_hip_rtm_scan_jac(r.ctx, over.get("nprof", b.nprof), over.get("npath", npath), over.get("nwn", b.nwn), g("wn"),
                                        g("nlay"), over.get("nlay_max", b.lm), g("irt"), quantity, g("T"), g("TZ"), g("O"), g("path"), g("ts"),
                                        over.get("sfc_per_path", sfc), g("em"), g("rf"), *[g(k) for k in RTM_OUT])
    return rc, outs


def ref_by_rtm_jac(r, b, path, quantity, O=None, em=None, rf=None):
    """The reference of the adjoint: one monortm_hip_rtm_jac call per path on optical depths scaled here (one rounding per element,
    in the context's REAL kind), zero padding; k_o = factor x its k_o, k_path = O x its k_o."""
    O = np.asarray(b.pad(b.O, 0.0) if O is None else O, r.dtype)
    f0 = np.asarray(b.pad(path, 0.0), r.dtype)
    res = {k: [] for k in RTM_OUT}
    for j in range(path.shape[1]):
        ej = None if em is None else (em[:, j] if np.ndim(em) == 3 else em)
        rj = None if rf is None else (rf[:, j] if np.ndim(rf) == 3 else rf)
        o = raw_rtm_jac(r, b, O * f0[:, j, :, None], quantity, ej, rj)
        ko = o["k_o"].astype(np.float64)
        for k in ("rad", "tb", "k_t", "k_tz", "k_sfc"):
            res[k].append(o[k].astype(np.float64))
        res["k_o"].append(f0[:, j, :, None].astype(np.float64) * ko)
        res["k_path"].append(O.astype(np.float64) * ko)
    return {k: np.stack(v, axis=1) for k, v in res.items()}


_REF = {}


def shared_ref(r, name, quantity):
    """Batch, the 9 paths and their reference: computed once per (batch, quantity), shared, never modified; fewer paths are a slice."""
    key = (name, quantity, r.real_kind)
    if key not in _REF:
        b = Batch(BATCHES[name], 11 + list(BATCHES).index(name))
        path = b.path(FACTORS9)
        want = ref_by_rtm_jac(r, b, path, quantity)
        for v in want.values():
            v.setflags(write=False)
        _REF[key] = (b, path, want)
    return _REF[key]


def check_adjoint(got, want, b, tol, what=""):
    """rad, tb at rtol `tol`; the K fields at `tol` by rel_err over the layer / level axis (k_sfc: over its three components);
    padded layers and levels exactly 0."""
    worst = {}
    for k in ("rad", "tb"):
        assert np.all(np.isfinite(got[k])), f"{what}: {k}"
        np.testing.assert_allclose(got[k], want[k], rtol=tol, atol=0, err_msg=f"{what}: {k}")
    for k in ("k_o", "k_path", "k_t", "k_tz", "k_sfc"):
        assert np.all(np.isfinite(got[k])), f"{what}: {k}"
        worst[k] = rel_err(np.asarray(got[k], np.float64), want[k], axis=2)
        print(f"{what}: {k} rel_err {worst[k]:.2e}")
    assert max(worst.values()) <= tol, (what, worst)
    npath = got["rad"].shape[1]
    lay = np.broadcast_to(b.lay[:, None, :], (b.nprof, npath, b.lm))
    lev = np.broadcast_to(b.lev[:, None, :], (b.nprof, npath, b.lm + 1))
    for k in ("k_o", "k_path", "k_t"):
        assert np.all(got[k][~lay] == 0), f"{what}: {k} padding"
    assert np.all(got["k_tz"][~lev] == 0), f"{what}: k_tz padding"
    return worst


# ---- 1. the adjoint equals rtm_jacobian per path on optical depths the test scaled ------------------------------------------------
@pytest.mark.parametrize("quantity", [1, 0])
@pytest.mark.parametrize("npath", NPATHS)
@pytest.mark.parametrize("name", list(BATCHES))
def test_adjoint_equals_rtm_jacobian_on_scaled_optical_depths(rt, name, npath, quantity):
    """rad, tb at rtol 1e-12, atol 0; k_o against f x (reference k_o), k_path against O x (reference k_o), k_t, k_tz, k_sfc against
    the reference's, each <= 1e-12 by rel_err (the project's bound between two HIP formulations of the recurrence: tau is rounded
    once and the terms come in rtm_jac_kernel's order, so only contraction differences remain).  The scan call gets NaN in every
    padded entry of O, T, TZ and path, the reference zeros; the outputs are pre-filled, so the zeros of padded layers and levels
    are the kernel's.  irt cycles 1, 2, 3.  Instantiations: R30, B30 -> <double, 8, 4, false>, C12 -> <double, 2, 4, false>.
    Measured worst (MI355X): k_o 3.8e-14, k_path 3.8e-14, k_t 3.7e-15, k_tz 3.9e-15, k_sfc 7.0e-15 (R30, npath = 9); rad, tb pass at
    rtol 1e-12."""
    b, path, want = shared_ref(rt, name, quantity)
    path = np.ascontiguousarray(path[:, :npath])
    want = {k: v[:, :npath] for k, v in want.items()}
    nan = np.nan
    rc, got = raw_scan_jac(rt, b, b.pad(path, nan), quantity, O=b.pad(b.O, nan), T=b.pad(b.T, nan), TZ=b.pad(b.TZ, nan))
    assert rc == 0, err(rt)
    check_adjoint(got, want, b, 1e-12, what=f"{name} npath={npath} q={quantity}")


# ---- 2. the adjoint against differences of the CPU oracle --------------------------------------------------------------------------
def _orc_rtm(pr, o, quantity):
    from oracle.pyoracle import lib

    nwn = pr.nwn
    rup, rdn, trtot, rad, tb = (np.zeros(nwn) for _ in range(5))
    ts = C.c_double(pr.tmpsfc)
    lib().orc_rtm(1, pr.irt, nwn, pr.wn, pr.nlay, np.ascontiguousarray(pr.t), np.ascontiguousarray(pr.tz), np.ascontiguousarray(o),
                  C.byref(ts), rup, trtot, rdn, np.ascontiguousarray(pr.reflc), np.ascontiguousarray(pr.emiss), rad, tb)
    return tb if quantity == "tb" else rad


@pytest.mark.parametrize("irt", [1, 2, 3])
@pytest.mark.parametrize("quantity", ["tb", "rad"])
def test_adjoint_matches_oracle_differences(case, irt, quantity):
    """Independent of any HIP adjoint: Richardson-extrapolated central differences of the oracle's RTM on f x O (the scheme of
    tests/test_jacobian.py::test_rtm_adjoint_matches_oracle_differences), one path with non-uniform factors in [1, 6].  k_o, k_path,
    k_t, k_tz, k_sfc at <= 1e-6 by rel_err.
    The profiles: 301, 302 as that test; 306 for irt = 3.  Downwelling radiance saturates in the opaque channels, where the largest
    |k_o| of a column is 1e-4 of RAD and less, and the difference quotient resolves it only to ~10 ulp(RAD) / h: with profile 303
    and these factors the quotient's OWN error against the exact derivative (complex step, on the CPU, tests/test_scan_jacobian_cpu.py)
    is 9e-8 .. 1.1e-6 depending on the last bits of O - at the bound whatever the adjoint does (first GPU run: 1.06e-6 for k_o, q = RAD,
    while the kernel agreed with rtm_jac_kernel to 4e-14).  Profile 306 saturates least of 303 .. 308 (largest |k_o| >= 3.8e-4 of
    RAD); there the quotient's own error is 1.3e-7."""
    _, wn, rt = case
    pr = synth.perturbed_profile({1: 301, 2: 302, 3: 306}[irt], wn, nlay=20, cloud=True, irt=irt)
    if irt != 1:
        pr.tmpsfc, pr.emiss, pr.reflc = 280.0, np.full(len(wn), 0.7), np.full(len(wn), 0.3)   # ignored by RTM for irt = 2, 3
    n = pr.nlay
    fac = np.random.default_rng(60 + irt).uniform(1.0, 6.0, n)
    O = rt.modm([pr])[0]
    res = rt.rtm_scan_jacobian([pr], O, fac[None, :], quantity)
    o = O[0]

    def cd(setter, h):   # central differences at h and 2h, Richardson-extrapolated (truncation O(h^4))
        d = []
        for hh in (h, 2 * h):
            q = []
            for sgn in (1, -1):
                p, oo, ff = copy.deepcopy(pr), o.copy(), fac.copy()
                setter(p, oo, ff, sgn * hh)
                q.append(_orc_rtm(p, ff[:, None] * oo, quantity))
            d.append((q[0] - q[1]) / (2 * hh))
        return (4 * d[0] - d[1]) / 3

    ref = {k: np.zeros((n, len(wn))) for k in ("k_o", "k_path", "k_t")}
    ref["k_tz"] = np.zeros((n + 1, len(wn)))
    for k in range(n):
        ref["k_o"][k] = cd(lambda p, oo, ff, h, k=k: oo[k].__iadd__(h), 1e-4 * max(float(o[k].max()), 1.0))
        ref["k_path"][k] = cd(lambda p, oo, ff, h, k=k: ff.__setitem__(k, ff[k] + h), 1e-4 * max(float(fac[k]), 1.0))
        ref["k_t"][k] = cd(lambda p, oo, ff, h, k=k: p.t.__setitem__(k, p.t[k] + h), 0.1)
    for j in range(n + 1):
        ref["k_tz"][j] = cd(lambda p, oo, ff, h, j=j: p.tz.__setitem__(j, p.tz[j] + h), 0.1)
    for name in ("k_o", "k_path", "k_t", "k_tz"):
        e = rel_err(res[name][0, 0], ref[name], axis=0)
        print(f"irt={irt} {quantity} {name}: {e:.2e}")
        assert e <= 1e-6, f"irt={irt} {quantity} {name}: {e:.2e}"
    assert np.all(res["k_o"][0, 0] != 0) and np.all(res["k_path"][0, 0] != 0)
    sfc = [cd(lambda p, oo, ff, h: setattr(p, "tmpsfc", p.tmpsfc + h), 0.1), cd(lambda p, oo, ff, h: setattr(p, "emiss", p.emiss + h), 1e-3),
           cd(lambda p, oo, ff, h: setattr(p, "reflc", p.reflc + h), 1e-3)]
    for i in range(3):
        got = res["k_sfc"][0, 0, i]
        if irt == 1:
            assert np.max(np.abs(got - sfc[i])) <= 1e-6 * np.abs(sfc[i]).max(), f"k_sfc[{i}]"
        else:
            assert np.all(got == 0), f"irt={irt} k_sfc[{i}]"


# ---- 3. the full entry against MonoRTM.jacobian on profiles with scaled amounts ---------------------------------------------------
def scaled(pr, s):
    """The profile with every amount of layer l multiplied by s[l]; P, T, TZ as they were."""
    q = copy.deepcopy(pr)
    s = np.asarray(s, np.float64)[: pr.nlay]
    q.wkl, q.wbrodl, q.clw = pr.wkl * s[:, None], pr.wbrodl * s, pr.clw * s
    return q


@pytest.fixture(scope="module")
def full_case(case):
    """Profiles, paths and the result of the full entry, shared by the tests below (never modified)."""
    _, wn, rt = case
    nl = [20, 16, 18]
    prs = [synth.perturbed_profile(450 + i, wn, nlay=n, cloud=True, irt=irt) for i, (n, irt) in enumerate(zip(nl, (1, 3, 2)))]
    l = np.arange(20) / 19.0
    path = np.asarray(FACTORS9[: NP + 1])[:, None] * (1.0 + 0.01 * l)[None, :]   # [5, 20]
    res = rt.scan_jacobian(prs, path, mols=(1, 3))
    for v in res.values():
        v.setflags(write=False)
    return prs, path, res


def test_full_entry_equals_jacobian_on_scaled_amounts(case, full_case):
    """monortm_hip_scan_jacobian (ONE set of MODM passes for all paths) against MonoRTM.jacobian - existing, separately tested code -
    on profiles whose wkl, wbrodl and clw are scaled by f_j per layer: k_t, k_tz, k_sfc, k_w directly, k_clw against f x (reference
    k_clw), each <= 1e-6 by rel_err (the project's Jacobian tolerance; expected ~1e-11 from DESIGN 3.6's rounding budget).  o equals
    modm, rad / tb equal scan at rtol 1e-12.  Instantiation <double, 2, 4, true> (nlay_max = 20), tiles of 4 + 1 paths."""
    _, wn, rt = case
    prs, path, res = full_case
    assert res["k_w"].shape == (3, NP + 1, 20, 2, len(wn))
    errs = {}
    for j in range(path.shape[0]):
        ref = rt.jacobian([scaled(p, path[j]) for p in prs], mols=(1, 3))
        for p, pr in enumerate(prs):
            n = pr.nlay
            errs[f"{j} {p} k_t"] = rel_err(res["k_t"][p, j, :n], ref["k_t"][p, :n], axis=0)
            errs[f"{j} {p} k_tz"] = rel_err(res["k_tz"][p, j, : n + 1], ref["k_tz"][p, : n + 1], axis=0)
            errs[f"{j} {p} k_sfc"] = rel_err(res["k_sfc"][p, j], ref["k_sfc"][p], axis=0)
            for i in range(2):
                kw = ref["k_w"][p, :n, i]
                errs[f"{j} {p} k_w[{i}]"] = rel_err(res["k_w"][p, j, :n, i], kw, axis=0, floor=w_floor(kw))
            errs[f"{j} {p} k_clw"] = rel_err(res["k_clw"][p, j, :n], path[j, :n, None] * ref["k_clw"][p, :n], axis=0)
            assert np.all(res["k_t"][p, j, n:] == 0) and np.all(res["k_w"][p, j, n:] == 0) and np.all(res["k_clw"][p, j, n:] == 0)
            assert np.all(res["k_tz"][p, j, n + 1:] == 0)
    worst = max(errs, key=errs.get)
    print(f"full entry vs jacobian on scaled amounts: worst {worst} = {errs[worst]:.2e}")
    assert errs[worst] <= 1e-6, {k: v for k, v in errs.items() if v > 1e-6}
    O = rt.modm(prs)[0]
    np.testing.assert_allclose(res["o"], O, rtol=1e-12, atol=0)
    sc = rt.rtm_scan(prs, O, path)
    np.testing.assert_allclose(res["rad"], sc["rad"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(res["tb"], sc["tb"], rtol=1e-12, atol=0)
    # the adjoint-only entry on the same O: the fields that do not involve the perturbed states
    adj = rt.rtm_scan_jacobian(prs, O, path)
    for k in ("k_o", "k_path", "k_tz", "k_sfc"):
        assert rel_err(res[k], adj[k], axis=2) <= 1e-12, k


# ---- 4. end to end against the oracle ----------------------------------------------------------------------------------------------
def _replace(pr, **kw):
    p = copy.deepcopy(pr)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def brute_force(run, prs, mols, quantity="tb", clw_step=1e-4, dlnw=api.JAC_DLNW):
    """brute_force of tests/test_jacobian.py: central differences with the API's steps, every perturbed profile changing ONE layer."""
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
            for sgn in (1, -1):
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


def test_full_entry_matches_oracle_end_to_end(case):
    """One 12-layer irt 1 profile, one plane-parallel path at 60 degrees: brute force through Oracle.run on the profile with scaled
    amounts; k_t, k_w and k_clw / f at <= 1e-5, as tests/test_jacobian.py::test_jacobian_matches_oracle_end_to_end."""
    from oracle.pyoracle import Oracle

    t3, wn, rt = case
    pr = synth.perturbed_profile(410, wn, nlay=12, cloud=True, irt=1)
    path = api.plane_parallel_path([60.0], 12)
    res = rt.scan_jacobian([pr], path, mols=(1,))
    orc = Oracle(t3, wn[0], wn[-1])
    (kt, kw, kc), = brute_force(lambda b: [orc.run(p) for p in b], [scaled(pr, path[0])], (1,))
    orc.close()
    e = dict(k_t=rel_err(res["k_t"][0, 0], kt, axis=0), k_w=rel_err(res["k_w"][0, 0, :, 0], kw[:, 0], axis=0, floor=w_floor(kw[:, 0])),
             k_clw=rel_err(res["k_clw"][0, 0] / path[0, :, None], kc, axis=0))
    print("end to end against the oracle:", {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= 1e-5, e


# ---- 5. a unit path ------------------------------------------------------------------------------------------------------------------
def test_unit_path_equals_rtm_jacobian_and_k_o_k_path_may_be_null(rt):
    b = Batch(BATCHES["B30"], 21)
    one = np.ones((b.nprof, 1, b.lm))
    for quantity in (1, 0):
        want = ref_by_rtm_jac(rt, b, one, quantity)
        rc, got = raw_scan_jac(rt, b, one, quantity)
        assert rc == 0, err(rt)
        check_adjoint(got, want, b, 1e-12, what=f"unit path q={quantity}")
    rc, sub = raw_scan_jac(rt, b, one, 0, drop=("k_o", "k_path"))
    assert rc == 0, err(rt)
    for k in RTM_OUT:
        if k in ("k_o", "k_path"):
            assert np.all(sub[k] == FILL)   # untouched
        else:
            np.testing.assert_array_equal(sub[k], got[k])


def raw_full(rt, prs, path, mols=(1,), quantity=1, drop=(), T=None, **over):
    """monortm_hip_scan_jacobian straight through ctypes -> (rc, outputs); drop: arrays passed as NULL; over: npath."""
    p0 = prs[0]
    nprof, nwn, nlay, lm, irt, T0, TZ, ts, em, rf = rt._pack_rtm(prs)
    T = T0 if T is None else T

    def pack(get, width=None):
        out = np.zeros((nprof, lm) if width is None else (nprof, lm, width))
        for i, p in enumerate(prs):
            out[i, : p.nlay] = get(p)
        return out

    P, CLW, WB, WKL = pack(lambda p: p.p), pack(lambda p: p.clw), pack(lambda p: p.wbrodl), pack(lambda p: p.wkl, p0.nmol)
    f = rt._path(path, nprof, lm)
    npath = f.shape[1]
    jm = np.ascontiguousarray(np.asarray(mols, np.int32).reshape(-1))
    z = lambda *s: np.full((nprof, npath) + s, FILL)  # noqa: E731
    out = dict(o=np.full((nprof, lm, nwn), FILL), rad=z(nwn), tb=z(nwn), k_t=z(lm, nwn), k_tz=z(lm + 1, nwn), k_w=z(lm, len(jm), nwn),
               k_clw=z(lm, nwn), k_o=z(lm, nwn), k_path=z(lm, nwn), k_sfc=z(3, nwn))
    a = dict(wn=np.ascontiguousarray(p0.wn), nlay=nlay, P=P, T=T, CLW=CLW, WKL=WKL, WB=WB, fac=np.ascontiguousarray(p0.cntnm), irt=irt, TZ=TZ,
             ts=ts, em=em, rf=rf, jm=jm, path=f)
    g = lambda k: None if k in drop else _p(a[k] if k in a else out[k])  # noqa: E731
    rc = rt.lib.monortm_hip_scan_jacobian(rt.ctx, nprof, nwn, g("wn"), p0.dvset, g("nlay"), lm, p0.nmol, g("P"), g("T"), g("CLW"), g("WKL"),
                                          g("WB"), g("fac"), p0.sclcpl, p0.sclhw, p0.y0res, p0.ibrd, g("irt"), g("TZ"), g("ts"), g("em"),
                                          g("rf"), quantity, len(jm), g("jm") if len(jm) else None, over.get("npath", npath), g("path"), 0,
                                          *[g(k) for k in FULL_OUT])
    return rc, out


def test_unit_path_equals_jacobian(case):
    """The full entry with factors 1 against monortm_hip_jacobian, every field at <= 1e-12 by rel_err; K_O and K_PATH may be NULL."""
    _, wn, rt = case
    prs = [synth.perturbed_profile(440 + i, wn, nlay=n, cloud=True, irt=irt) for i, (n, irt) in enumerate(((20, 1), (16, 3), (18, 2)))]
    ref = rt.jacobian(prs, mols=(1, 3))
    got = rt.scan_jacobian(prs, np.ones((1, 20)), mols=(1, 3))
    for k in api.JAC_FIELDS:
        g = got[k] if k == "o" else got[k][:, 0]
        assert rel_err(g, ref[k], axis=1 if ref[k].ndim > 2 else 0) <= 1e-12, k
    assert rel_err(got["k_path"][:, 0], ref["o"] * ref["k_o"], axis=1) <= 1e-12
    rc, sub = raw_full(rt, prs, np.ones((1, 20)), mols=(1, 3), drop=("k_o", "k_path"))
    assert rc == 0, err(rt)
    assert np.all(sub["k_o"] == FILL) and np.all(sub["k_path"] == FILL)   # untouched
    same_full(dict(sub, k_o=got["k_o"], k_path=got["k_path"]), got, 1e-12)


# ---- 6. a zero factor in one layer -------------------------------------------------------------------------------------------------
def test_zero_factor_layer(rt):
    """The layer does not absorb along that path: k_o (= factor x dq/dtau) of the layer is 0, k_path (= O x dq/dtau: what a larger
    factor would do) is finite and not 0; everything still equals the per-path reference."""
    b = Batch(BATCHES["C12"], 22)
    path = b.path([1.0, 2.5])
    path[:, 1, 2] = 0.0
    path[1, 0, 11] = 0.0
    want = ref_by_rtm_jac(rt, b, path, 1)
    rc, got = raw_scan_jac(rt, b, path, 1)
    assert rc == 0, err(rt)
    check_adjoint(got, want, b, 1e-12, what="zero factor")
    for sel in ((slice(None), 1, 2), (1, 0, 11)):
        assert np.all(got["k_o"][sel] == 0)
        assert np.all(np.isfinite(got["k_path"][sel])) and np.all(got["k_path"][sel] != 0)


# ---- 7. surface arrays per path ----------------------------------------------------------------------------------------------------
def test_surface_arrays_per_path(rt):
    b = Batch(BATCHES["B30"], 23, irt=(1,))
    path = b.path(FACTORS9[: NP + 1])
    rng = np.random.default_rng(5)
    em = rng.uniform(0.5, 1.0, (b.nprof, NP + 1, b.nwn))
    rf = 1.0 - em
    want = ref_by_rtm_jac(rt, b, path, 1, em=em, rf=rf)
    rc, got = raw_scan_jac(rt, b, path, 1, em=em, rf=rf)
    assert rc == 0, err(rt)
    check_adjoint(got, want, b, 1e-12, what="surface per path")
    np.testing.assert_allclose(got["k_sfc"], want["k_sfc"], rtol=1e-12, atol=0)
    rc, shared = raw_scan_jac(rt, b, path, 1)
    assert rc == 0
    assert not np.array_equal(got["k_sfc"], shared["k_sfc"])
    rep = lambda x: np.ascontiguousarray(np.broadcast_to(x[:, None, :], (b.nprof, NP + 1, b.nwn)))  # noqa: E731
    rc, replicated = raw_scan_jac(rt, b, path, 1, em=rep(b.em), rf=rep(b.rf))
    assert rc == 0
    for k in RTM_OUT:
        np.testing.assert_array_equal(replicated[k], shared[k])


# ---- 8. real_kind = 4 ----------------------------------------------------------------------------------------------------------------
def test_real_kind_4(rt, rt4, case):
    """float32 arrays, double arithmetic: the K of the double context to float rounding, <= 1e-4 by rel_err (the bound of
    tests/test_jacobian.py::test_rtm_adjoint_single_precision).  Reaches <float, 8, 4, false> and <float, 2, 4, false>.  The full
    entry needs double arrays: EUNSUPPORTED."""
    for name in ("B30", "C12"):
        b = Batch(BATCHES[name], 30)
        path = b.path(FACTORS9[: NP + 1])
        rc, ref = raw_scan_jac(rt, b, path, 1)
        assert rc == 0
        rc, got = raw_scan_jac(rt4, b, path, 1)
        assert rc == 0, err(rt4)
        for k in ("k_o", "k_path", "k_t", "k_tz", "k_sfc"):
            assert got[k].dtype == np.float32
            assert rel_err(got[k].astype(np.float64), ref[k], axis=2) <= 1e-4, (name, k)
        np.testing.assert_allclose(got["tb"], ref["tb"], rtol=1e-5)
    _, wn, _ = case
    pr = synth.perturbed_profile(490, wn, nlay=8)
    with pytest.raises(api.MonoRTMError) as e:
        rt4.scan_jacobian([pr], np.ones((1, 8)))
    assert api.ERRORS[e.value.code] == "EUNSUPPORTED"


# ---- 9. plumbing ---------------------------------------------------------------------------------------------------------------------
def test_multi_device_context(rt, monkeypatch):
    """A two-shard context (both on device 0) equals one device; a bad factor in the LAST shard is refused before any launch: every
    output keeps the caller's fill.  The context still works afterwards."""
    b = Batch(BATCHES["B30"], 40)
    path = b.path(FACTORS9)
    monkeypatch.setenv("MONORTM_DEVICES", "0,0")
    m = api.MonoRTM("", 0.0, 0.0, ngpu=0)
    assert m.lib.monortm_hip_device_count(m.ctx) == 2
    rc, one = raw_scan_jac(rt, b, path, 1)
    assert rc == 0
    rc, two = raw_scan_jac(m, b, path, 1)
    assert rc == 0, err(m)
    for k in RTM_OUT:
        np.testing.assert_array_equal(two[k], one[k])
    for v in (-1.0, np.nan, np.inf):
        f = path.copy()
        f[2, 3, 29] = v                              # the last active layer of the last profile
        rc, got = raw_scan_jac(m, b, f, 1)
        assert rc == EARG and b"profile 2 path 3 layer 29" in err(m)
        assert all(np.all(got[k] == FILL) for k in RTM_OUT)
    bad_nlay = copy.copy(b)
    bad_nlay.nlay = np.array([5, 24, 31], np.int32)
    rc, got = raw_scan_jac(m, bad_nlay, path, 1)
    assert rc == EARG and all(np.all(got[k] == FILL) for k in RTM_OUT)
    rc, again = raw_scan_jac(m, b, path, 1)
    assert rc == 0, err(m)
    for k in RTM_OUT:
        np.testing.assert_array_equal(again[k], one[k])
    m.close()


def same_full(got, ref, tol, other=None):
    """The outputs of the full entry: o, rad, tb at rtol `tol`, the K fields at `tol` by rel_err over the layer / level axis (k_sfc:
    its three components); `other`: fields with a bound of their own."""
    for k in FULL_OUT:
        g = got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy()
        t = (other or {}).get(k, tol)
        if k in ("o", "rad", "tb"):
            np.testing.assert_allclose(g, ref[k], rtol=t, atol=0, err_msg=k)
        else:
            assert rel_err(g, ref[k], axis=2) <= t, k


def test_full_entry_multi_device(case, full_case, monkeypatch):
    t3, wn, _ = case
    prs, path, res = full_case
    monkeypatch.setenv("MONORTM_DEVICES", "0,0")
    m = api.MonoRTM(t3, wn[0], wn[-1], ngpu=0)
    assert m.lib.monortm_hip_device_count(m.ctx) == 2
    two = m.scan_jacobian(prs, path, mols=(1, 3))
    f = np.broadcast_to(path[None], (3,) + path.shape).copy()
    f[2, 4, 17] = -0.5                               # the last active layer of the last profile, in the last shard
    with pytest.raises(api.MonoRTMError) as e:
        m.scan_jacobian(prs, f, mols=(1, 3))
    assert e.value.code == EARG and "profile 2 path 4 layer 17" in str(e.value)
    m.close()
    # (the shards run MODM on batches of other sizes: O agrees to rounding, which the differences in k_t and k_w divide by the step -
    # the 1e-9 of tests/test_jacobian.py::test_mixed_nlay_equals_single_profiles, k_w with its floor per profile)
    same_full(dict(two, k_w=res["k_w"]), res, 1e-12, {"k_t": 1e-9})
    for p in range(len(prs)):
        assert rel_err(two["k_w"][p], res["k_w"][p], axis=1, floor=w_floor(res["k_w"][p])) <= 1e-9, p


def test_device_batch_scan_jacobian_and_graph_replay(case, full_case):
    import torch

    _, wn, rt = case
    prs, path, ref = full_case
    db = api.DeviceBatch(rt, prs)
    fdev = torch.as_tensor(path).to(db.dev)
    got = db.scan_jacobian(fdev, mols=(1, 3))
    torch.cuda.synchronize()
    db.check()
    same_full(got, ref, 1e-12)
    assert db.scan_jacobian(fdev, mols=(1, 3)) is got    # overwritten in place
    torch.cuda.synchronize()
    # one capture after the warm calls; the factors change in their device tensor, the replay follows them into the same tensors
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            db.scan_jacobian(fdev, mols=(1, 3))
    torch.cuda.current_stream().wait_stream(s)
    path2 = path[::-1] * 1.25
    fdev.copy_(torch.as_tensor(np.ascontiguousarray(path2)))
    for v in got.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    db.check()
    ref2 = rt.scan_jacobian(prs, path2, mols=(1, 3))
    assert not np.array_equal(ref2["tb"], ref["tb"])
    same_full(got, ref2, 1e-12)


def test_scan_jacobian_between_modm_and_rtm_changes_nothing(case, full_case):
    _, wn, rt = case
    prs, path, _ = full_case
    O = rt.modm(prs)[0]
    tb0 = rt.rtm(prs, O)[4]
    sc0 = rt.rtm_scan(prs, O, path)["tb"]
    O = rt.modm(prs)[0]
    rt.scan_jacobian(prs, path, mols=(1,))
    rt.rtm_scan_jacobian(prs, O, path)
    tb1 = rt.rtm(prs, O)[4]
    sc1 = rt.rtm_scan(prs, O, path)["tb"]
    assert np.array_equal(tb0, tb1) and np.array_equal(sc0, sc1)


def test_refusals_leave_the_context_working(rt, case):
    b = Batch(BATCHES["C12"], 50)
    path = b.path([1.0, 2.0, 3.0])
    rc, want = raw_scan_jac(rt, b, path, 1)
    assert rc == 0
    for over in (dict(npath=0), dict(npath=-3), dict(npath=1 << 20), dict(sfc_per_path=2), dict(nprof=0), dict(nwn=0), dict(nlay_max=0),
                 dict(nlay_max=604)):
        assert raw_scan_jac(rt, b, path, 1, **over)[0] == EARG, over
        assert err(rt)
    for q in (2, -1):
        assert raw_scan_jac(rt, b, path, q)[0] == EARG, q
    for name in ("wn", "nlay", "irt", "T", "TZ", "O", "path", "ts", "em", "rf", "rad", "tb", "k_t", "k_tz", "k_sfc"):
        assert raw_scan_jac(rt, b, path, 1, drop=(name,))[0] == EARG, name
    bad_nlay = copy.copy(b)
    bad_nlay.nlay = np.array([3, 13], np.int32)     # beyond nlay_max = 12
    assert raw_scan_jac(rt, bad_nlay, path, 1)[0] == EARG
    for v in (-1e-3, np.nan, np.inf):
        f = path.copy()
        f[0, 2, 2] = v                               # an active layer of profile 0 (3 layers)
        rc, got = raw_scan_jac(rt, b, f, 1)
        assert rc == EARG, v
        assert all(np.all(got[k] == FILL) for k in RTM_OUT)
    f = path.copy()
    f[0, 1, 3:] = -1.0                               # padded layers of profile 0: ignored
    f[0, 2, 7] = np.nan
    rc, got = raw_scan_jac(rt, b, f, 1)
    assert rc == 0, err(rt)
    for k in RTM_OUT:
        np.testing.assert_array_equal(got[k], want[k])
    # the full entry
    _, wn, r = case
    prs = [synth.perturbed_profile(490, wn, nlay=16)]
    one = np.ones((1, 16))
    code = lambda rc: api.ERRORS.get(rc, "OK")  # noqa: E731
    assert raw_full(r, prs, one)[0] == 0
    for mols in ((0,), (8,), (1, 1)):
        assert code(raw_full(r, prs, one, mols=mols)[0]) == "EARG", mols
    assert code(raw_full(r, prs, one, quantity=2)[0]) == "EARG"
    assert code(raw_full(r, prs, one, npath=0)[0]) == "EARG"
    for name in ("wn", "nlay", "P", "T", "CLW", "WKL", "WB", "fac", "irt", "TZ", "ts", "em", "rf", "path", "o", "rad", "tb", "k_t", "k_tz", "k_w",
                 "k_clw", "k_sfc"):
        assert code(raw_full(r, prs, one, drop=(name,))[0]) == "EARG", name
    for v in (-2.0, np.nan, np.inf):
        f = one.copy()
        f[0, 15] = v
        rc, got = raw_full(r, prs, f)
        assert code(rc) == "EARG", v
        assert all(np.all(got[k] == FILL) for k in FULL_OUT)
    cold = prs[0].t[None].copy()
    cold[0, 3] = 70.0 + 0.5 * api.JAC_DT
    assert code(raw_full(r, prs, one, T=cold)[0]) == "ETEMP"
    cold[0, 3] = 3000.0 - 0.5 * api.JAC_DT
    assert code(raw_full(r, prs, one, T=cold)[0]) == "ETEMP"
    res = r.scan_jacobian(prs, one)
    assert all(np.all(np.isfinite(v)) for v in res.values())


def test_device_entry_flags_bad_factors(rt):
    import torch

    b = Batch(BATCHES["C12"], 51)
    path = b.path([1.0, 2.0, 3.0])
    rc, want = raw_scan_jac(rt, b, path, 1)
    assert rc == 0
    dev = torch.device("cuda:0")
    up = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
    wn, nlay, irt = up(b.wn), up(b.nlay, torch.int32), up(b.irt, torch.int32)
    T, TZ, O, em, rf, ts = up(b.pad(b.T, 0.0)), up(b.pad(b.TZ, 0.0)), up(b.pad(b.O, 0.0)), up(b.em), up(b.rf), up(b.ts)
    outs = {k: torch.zeros(s, dtype=torch.float64, device=dev) for k, s in shapes(b, 3).items()}
    d = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(f, npath=3):
        fd = up(f)
        rc = rt.lib.monortm_hip_rtm_scan_jac_dev(rt.ctx, b.nprof, npath, b.nwn, d(wn), d(nlay), b.lm, d(irt), 1, d(T), d(TZ), d(O), d(fd), d(ts),
                                                 0, d(em), d(rf), *[d(outs[k]) for k in RTM_OUT], s)
        return rc, rt.lib.monortm_hip_check(rt.ctx, s)

    assert call(path) == (0, 0)
    for k in RTM_OUT:
        np.testing.assert_array_equal(outs[k].cpu().numpy(), want[k])
    for v in (-2.0, np.nan, np.inf):
        f = path.copy()
        f[1, 0, 11] = v                              # the last active layer of profile 1
        assert call(f) == (0, EARG), v               # the launch succeeds, the flag tells
        assert rt.lib.monortm_hip_check(rt.ctx, s) == 0   # ... once
    f = path.copy()
    f[0, 0, 6] = -5.0                                # a padded layer
    assert call(f) == (0, 0)
    for k in RTM_OUT:
        np.testing.assert_array_equal(outs[k].cpu().numpy(), want[k])
    assert call(path, npath=0)[0] == EARG
    assert call(path) == (0, 0)
