"""Path scans on the GPU (monortm_hip_rtm_scan / _dev, rtm_scan_kernel.hip): radiances along npath paths per
profile from ONE set of optical depths, against monortm_hip_rtm on optical depths that the test scaled itself, against the CPU oracle
end to end, and the plumbing around it (surface arrays, real_kind 4, sharding, the resident O, DeviceBatch and graph replay, errors).

Synthetic inputs are seeded; O is lognormal, clipped to 1e-5 .. 5; 70 wavenumbers = one full block of 64 lanes and one with 6 live
lanes."""
import copy
import ctypes as C

import numpy as np
import pytest

from monortm_amd import api, synth, tape3

pytestmark = pytest.mark.gpu

NWN = 70
OUT = api.SCAN_FIELDS            # rup, rdn, trtot, rad, tb, tmr: the output order of both entry points
EARG = 6
FACTORS5 = [1.0, 1.3, 2.0, 5.76, 19.1]
FACTORS9 = FACTORS5 + [1.05, 3.3, 0.7, 11.0]
# the ragged batches of the issue; with SCAN_NP = 4 paths per thread npath = 5 is 2 tiles (4 + 1), npath = 9 is 3 (4 + 4 + 1)
BATCHES = {
    "A64": [1, 2, 7, 23, 24, 48, 64],   # 2 x 7 x 2|3 workgroups < 256, nlay_max >= 48 -> rtm_scan_kernel<R, 16, 4>
    "B30": [5, 24, 30],                 # 24 <= nlay_max < 48                          -> rtm_scan_kernel<R, 8, 4>
    "C12": [3, 12],                     # nlay_max < 24                                -> rtm_scan_kernel<R, 2, 4>
    "D48": [48] * 140,                  # 2 x 140 x 2|3 workgroups >= 256              -> rtm_scan_kernel<R, 8, 4>, many workgroups
}


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


@pytest.fixture(scope="module")
def rt(gpu):
    """RTM needs no line table: a context without TAPE3."""
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
    t3 = f"{workdir}/TAPE3_scan"
    tape3.write_tape3(t3, synth.synthetic_lines(300, seed=777, lc_frac=0.5, sdep_frac=0.2))
    wn = np.unique(np.concatenate([synth.c2_channels(12, seed=11), synth.sounder_channels()]))
    r = api.MonoRTM(t3, wn[0], wn[-1])
    yield t3, wn, r
    r.close()


class Batch:
    """Seeded RTM inputs of a ragged batch; pad(x, v) fills what lies beyond nlay[p] (levels beyond nlay[p] + 1) with v."""

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


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw_rtm(r, b, O, em=None, rf=None, T=None, TZ=None, tmr=True):
    """monortm_hip_rtm on the batch with optical depths O [nprof, lm, nwn] -> (rc, dict of [nprof, nwn], tmpsfc)."""
    dt = r.dtype
    c = lambda x: np.ascontiguousarray(x, dt)  # noqa: E731
    T, TZ, O = c(b.pad(b.T, 0.0) if T is None else T), c(b.pad(b.TZ, 0.0) if TZ is None else TZ), c(O)
    em, rf, ts = c(b.em if em is None else em), c(b.rf if rf is None else rf), c(b.ts).copy()
    outs = {k: np.full((b.nprof, b.nwn), -7.0, dt) for k in OUT}
    rc = r.lib.monortm_hip_rtm(r.ctx, b.nprof, b.nwn, _p(b.wn), _p(b.nlay), b.lm, _p(b.irt), 1, _p(T), _p(TZ), _p(O), _p(ts), _p(em),
                               _p(rf), *[_p(outs[k]) if (tmr or k != "tmr") else None for k in OUT])
    return rc, outs, ts


def raw_scan(r, b, path, O=None, em=None, rf=None, T=None, TZ=None, tmr=True, sfc=None, drop=(), **over):
    """monortm_hip_rtm_scan -> (rc, dict of [nprof, npath, nwn], tmpsfc).  drop: names of arrays passed as NULL; over: nprof /
    npath / nwn / nlay_max / sfc_per_path handed to the call instead of the arrays' own."""
    dt = r.dtype
    c = lambda x: np.ascontiguousarray(x, dt)  # noqa: E731
    path = c(path)
    npath = path.shape[1]
    a = dict(wn=b.wn, nlay=b.nlay, irt=b.irt, T=c(b.pad(b.T, 0.0) if T is None else T), TZ=c(b.pad(b.TZ, 0.0) if TZ is None else TZ),
             O=c(b.pad(b.O, 0.0) if O is None else O), path=path, ts=c(b.ts).copy(), em=c(b.em if em is None else em),
             rf=c(b.rf if rf is None else rf))
    outs = {k: np.full((b.nprof, npath, b.nwn), -7.0, dt) for k in OUT}
    if sfc is None:
        sfc = int(a["em"].ndim == 3)
    g = lambda k: None if k in drop else _p(a[k] if k in a else outs[k])  # noqa: E731
    rc = r.lib.monortm_hip_rtm_scan(r.ctx, over.get("nprof", b.nprof), over.get("npath", npath), over.get("nwn", b.nwn), g("wn"),
                                    g("nlay"), over.get("nlay_max", b.lm), g("irt"), 1, g("T"), g("TZ"), g("O"), g("path"), g("ts"),
                                    over.get("sfc_per_path", sfc), g("em"), g("rf"),
                                    *[g(k) if (tmr or k != "tmr") else None for k in OUT])
    return rc, outs, a["ts"]


def ref_by_rtm(r, b, path, O=None, em=None, rf=None):
    """The reference of the scan: one monortm_hip_rtm call per path on optical depths scaled here (one rounding per element, in
    the context's REAL kind), zero padding.  em / rf may be [nprof, npath, nwn]."""
    O = b.pad(b.O, 0.0) if O is None else O
    f0 = b.pad(path, 0.0)
    res = {k: [] for k in OUT}
    ts = None
    for j in range(path.shape[1]):
        Oj = np.asarray(O, r.dtype) * np.asarray(f0[:, j, :, None], r.dtype)
        ej = None if em is None else (em[:, j] if np.ndim(em) == 3 else em)
        rj = None if rf is None else (rf[:, j] if np.ndim(rf) == 3 else rf)
        rc, o, ts = raw_rtm(r, b, Oj, ej, rj)
        assert rc == 0, r.lib.monortm_hip_last_error(r.ctx)
        for k in OUT:
            res[k].append(o[k])
    return {k: np.stack(v, axis=1) for k, v in res.items()}, ts


_REF = {}


def shared_ref(r, name, seed, factors):
    """Batch, path and reference of (batch, factors): computed once, shared by the tests that need them, never modified."""
    key = (name, len(factors), r.real_kind)
    if key not in _REF:
        b = Batch(BATCHES[name], seed)
        path = b.path(factors)
        want, ts = ref_by_rtm(r, b, path)
        for v in want.values():
            v.setflags(write=False)
        _REF[key] = (b, path, want, ts)
    return _REF[key]


def assert_same(got, want, rtol, fields=OUT, what=""):
    for k in fields:
        assert np.all(np.isfinite(got[k])), f"{what}: {k} is not finite"
        np.testing.assert_allclose(got[k], want[k], rtol=rtol, atol=0, err_msg=f"{what}: {k}")


# ---- 1. equals rtm on pre-scaled optical depths --------------------------------------------------------------------------------
@pytest.mark.parametrize("npath", [5, 9])
@pytest.mark.parametrize("name", list(BATCHES))
def test_scan_equals_rtm_on_scaled_optical_depths(rt, name, npath):
    """All six outputs and tmpsfc at rtol 1e-12, atol 0 (the tolerance between two HIP formulations of the recurrence), irt cycling
    1, 2, 3.  The scan call gets NaN in every padded entry of O, T, TZ and path, the reference zeros: padding is never read.
    Launch instantiations reached (double): A64 -> <double, 16, 4> (few workgroups, >= 48 layers), B30 -> <double, 8, 4>,
    C12 -> <double, 2, 4>, D48 -> <double, 8, 4> past the few-workgroups rule (560 / 840 workgroups).  npath = 5: tiles of 4 + 1
    paths; npath = 9: 4 + 4 + 1 (more than one full tile and a short last one)."""
    b, path, want, ts_want = shared_ref(rt, name, 11 + list(BATCHES).index(name), FACTORS5 if npath == 5 else FACTORS9)
    nan = np.nan
    rc, got, ts = raw_scan(rt, b, b.pad(path, nan), O=b.pad(b.O, nan), T=b.pad(b.T, nan), TZ=b.pad(b.TZ, nan))
    assert rc == 0, rt.lib.monortm_hip_last_error(rt.ctx)
    assert_same(got, want, 1e-12, what=f"{name} npath={npath}")
    np.testing.assert_allclose(ts, ts_want, rtol=1e-12, atol=0)
    assert np.all(ts[b.irt != 1] == 2.75) and np.all(ts[b.irt == 1] == b.ts[b.irt == 1])


# ---- 2. one path, factors 1 ------------------------------------------------------------------------------------------------------
def test_one_unit_path_equals_rtm_and_tmr_may_be_null(rt):
    b = Batch([9, 31, 40], 21)
    rc, want, ts_want = raw_rtm(rt, b, b.pad(b.O, 0.0))
    assert rc == 0
    one = np.ones((b.nprof, 1, b.lm))
    rc, got, ts = raw_scan(rt, b, one)
    assert rc == 0, rt.lib.monortm_hip_last_error(rt.ctx)
    assert_same({k: v[:, 0] for k, v in got.items()}, want, 1e-12)
    np.testing.assert_array_equal(ts, ts_want)
    rc, no_tmr, _ = raw_scan(rt, b, one, tmr=False)
    assert rc == 0, rt.lib.monortm_hip_last_error(rt.ctx)
    for k in OUT[:-1]:
        np.testing.assert_array_equal(no_tmr[k], got[k])
    assert np.all(no_tmr["tmr"] == -7.0)   # untouched


# ---- 3. a layer with factor 0 ----------------------------------------------------------------------------------------------------
def test_zero_factor_layer_equals_zeroed_optical_depth(rt):
    b = Batch([6, 26], 22)
    path = b.path([1.0, 2.5])
    path[:, 1, 3] = 0.0
    path[1, 0, 25] = 0.0
    path[0, 0, 0] = 0.0
    want, _ = ref_by_rtm(rt, b, path)
    O2 = b.pad(b.O, 0.0)
    O2[:, 3] = 0.0
    rc, lay3, _ = raw_rtm(rt, b, O2 * b.pad(path, 0.0)[:, 1, :, None])
    assert rc == 0
    rc, got, _ = raw_scan(rt, b, path)
    assert rc == 0, rt.lib.monortm_hip_last_error(rt.ctx)
    assert_same(got, want, 1e-12)
    assert_same({k: v[:, 1] for k, v in got.items()}, lay3, 1e-12)


# ---- 4. surface arrays -----------------------------------------------------------------------------------------------------------
def test_surface_arrays_per_path(rt):
    b = Batch([8, 25, 17], 23, irt=(1,))
    path = b.path(FACTORS5)
    rc, shared, _ = raw_scan(rt, b, path)
    assert rc == 0
    rep = lambda x: np.ascontiguousarray(np.broadcast_to(x[:, None, :], (b.nprof, 5, b.nwn)))  # noqa: E731
    rc, replicated, _ = raw_scan(rt, b, path, em=rep(b.em), rf=rep(b.rf))
    assert rc == 0, rt.lib.monortm_hip_last_error(rt.ctx)
    for k in OUT:
        np.testing.assert_array_equal(replicated[k], shared[k])
    rng = np.random.default_rng(5)
    em = rng.uniform(0.5, 1.0, (b.nprof, 5, b.nwn))
    rf = 1.0 - em
    want, _ = ref_by_rtm(rt, b, path, em=em, rf=rf)
    rc, got, _ = raw_scan(rt, b, path, em=em, rf=rf)
    assert rc == 0
    assert_same(got, want, 1e-12)
    assert not np.array_equal(got["rad"], shared["rad"])


# ---- 5. end to end against the oracle --------------------------------------------------------------------------------------------
def test_scan_end_to_end_matches_oracle(case):
    """MonoRTM.scan against Oracle.run on profiles whose wkl, wbrodl and clw are scaled by the path: TB, RAD, TMR at 1e-6."""
    from oracle.pyoracle import Oracle

    t3, wn, r = case
    prs = [synth.perturbed_profile(520 + i, wn, nlay=12, cloud=True, irt=irt) for i, irt in enumerate((1, 3))]
    path = api.plane_parallel_path([0.0, 48.0, 70.0], 12) * (1.0 + 0.02 * np.arange(12))[None, :]
    got = r.scan(prs, path)
    assert got["tb"].shape == (2, 3, len(wn)) and got["tmpsfc"].shape == (2,)
    orc = Oracle(t3, wn[0], wn[-1])
    for i, pr in enumerate(prs):
        for j in range(3):
            q = copy.deepcopy(pr)
            s = path[j]
            q.wkl, q.wbrodl, q.clw = pr.wkl * s[:, None], pr.wbrodl * s, pr.clw * s
            want = orc.run(q)
            for k in ("tb", "rad", "tmr"):
                np.testing.assert_allclose(got[k][i, j], getattr(want, k), rtol=1e-6, atol=0, err_msg=f"profile {i} path {j} {k}")
    orc.close()


# ---- 6. real_kind = 4 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A64", "B30", "C12"])
def test_real_kind_4(rt4, name):
    """Factors from {0.5, 1, 2, 4} are exact in float, so the float O the reference gets is the product the kernel forms in double;
    both sides compute in double and round once: 2 float ulps, rtol 2.4e-7.  Reaches <float, 16, 4>, <float, 8, 4>, <float, 2, 4>."""
    b = Batch(BATCHES[name], 30 + list(BATCHES).index(name))
    rng = np.random.default_rng(6)
    path = rng.choice([0.5, 1.0, 2.0, 4.0], (b.nprof, 5, b.lm))
    O32 = b.pad(b.O, 0.0).astype(np.float32)
    want, ts_want = ref_by_rtm(rt4, b, path, O=O32)
    assert want["rad"].dtype == np.float32
    rc, got, ts = raw_scan(rt4, b, path, O=O32)
    assert rc == 0, rt4.lib.monortm_hip_last_error(rt4.ctx)
    assert_same(got, want, 2.4e-7, what=name)
    np.testing.assert_array_equal(ts, ts_want)


# ---- 7. multi-device -----------------------------------------------------------------------------------------------------------------
def test_multi_device_context_equals_one_device(rt, monkeypatch):
    b = Batch([4, 30, 11, 26, 19], 40)
    path = b.path(FACTORS9)
    rng = np.random.default_rng(7)
    em = rng.uniform(0.5, 1.0, (b.nprof, 9, b.nwn))
    monkeypatch.setenv("MONORTM_DEVICES", "0,0")
    m = api.MonoRTM("", 0.0, 0.0, ngpu=0)
    assert m.lib.monortm_hip_device_count(m.ctx) == 2
    for kw in ({}, dict(em=em, rf=1.0 - em)):
        rc, one, ts1 = raw_scan(rt, b, path, **kw)
        assert rc == 0
        rc, two, ts2 = raw_scan(m, b, path, **kw)
        assert rc == 0, m.lib.monortm_hip_last_error(m.ctx)
        for k in OUT:
            np.testing.assert_array_equal(two[k], one[k])
        np.testing.assert_array_equal(ts2, ts1)
    m.close()


def test_multi_device_context_refuses_before_any_launch(monkeypatch):
    """A bad factor in a profile of the LAST shard: EARG, and no earlier shard has run - every output keeps the caller's fill and
    tmpsfc (irt 2 / 3 would set 2.75) is as given.  The same for an nlay beyond nlay_max.  The context still works afterwards."""
    b = Batch([4, 30, 11, 26, 19], 41)
    path = b.path(FACTORS5)
    monkeypatch.setenv("MONORTM_DEVICES", "0,0")
    m = api.MonoRTM("", 0.0, 0.0, ngpu=0)
    assert m.lib.monortm_hip_device_count(m.ctx) == 2
    rc, want, ts_want = raw_scan(m, b, path)
    assert rc == 0, m.lib.monortm_hip_last_error(m.ctx)
    for v in (-1.0, np.nan):
        f = path.copy()
        f[4, 3, 18] = v                              # the last active layer of the last profile
        rc, got, ts = raw_scan(m, b, f)
        assert rc == EARG and b"profile 4 path 3 layer 18" in m.lib.monortm_hip_last_error(m.ctx)
        assert all(np.all(got[k] == -7.0) for k in OUT)
        np.testing.assert_array_equal(ts, b.ts)
    bad_nlay = copy.copy(b)
    bad_nlay.nlay = np.array([4, 30, 11, 26, 31], np.int32)
    rc, got, ts = raw_scan(m, bad_nlay, path)
    assert rc == EARG
    assert all(np.all(got[k] == -7.0) for k in OUT)
    np.testing.assert_array_equal(ts, b.ts)
    rc, got, ts = raw_scan(m, b, path)
    assert rc == 0, m.lib.monortm_hip_last_error(m.ctx)
    for k in OUT:
        np.testing.assert_array_equal(got[k], want[k])
    np.testing.assert_array_equal(ts, ts_want)
    m.close()


# ---- 8. the resident optical depths ----------------------------------------------------------------------------------------------------
def test_resident_optical_depths_are_reused(case):
    _, wn, r = case
    prs = [synth.perturbed_profile(530 + i, wn, nlay=n, cloud=True, irt=1 + 2 * i) for i, n in enumerate((12, 9))]
    path = api.plane_parallel_path([0.0, 30.0, 60.0], 12)
    c0, c1 = r.counter(0), r.counter(1)
    O = r.modm(prs)[0]
    res = r.rtm_scan(prs, O, path)
    assert r.counter(1) == c1 + 1
    O2 = O.copy()
    assert O2[1, 10, 0] == 0.0      # a padded layer of the second profile
    O2[1, 10, 0] = 1.0
    up = r.rtm_scan(prs, O2, path)
    assert r.counter(1) == c1 + 1   # compared unequal: uploaded
    assert r.counter(0) == c0
    for k in OUT + ("tmpsfc",):
        np.testing.assert_array_equal(up[k], res[k])
    assert r.counter(8) == -1 and r.counter(-1) == -1      # (2 .. 7 count the finish launches by variant)


# ---- 9. DeviceBatch.scan ---------------------------------------------------------------------------------------------------------------
def test_device_batch_scan(case):
    import torch

    _, wn, r = case
    prs = [synth.perturbed_profile(540 + i, wn, nlay=n, cloud=True, irt=irt) for i, (n, irt) in enumerate(((14, 1), (10, 3), (14, 2)))]
    path = api.plane_parallel_path([0.0, 20.0, 40.0, 55.0, 65.0, 75.0], 14)
    want = r.scan(prs, path)
    db = api.DeviceBatch(r, prs)
    db.step()
    torch.cuda.synchronize()
    before = db.spectral_block().clone()
    blk = db.scan(path)
    db.check()
    assert tuple(blk.shape) == (6, 3, 6, len(wn))
    got = blk.cpu().numpy()
    for i, k in enumerate(("rad", "tb", "trtot", "tmr", "rup", "rdn")):   # the order of spectral_block()
        np.testing.assert_allclose(got[i], want[k], rtol=1e-12, atol=0, err_msg=k)
    assert db.scan(path) is blk   # overwritten in place
    db.step()
    torch.cuda.synchronize()
    assert torch.equal(db.spectral_block(), before)
    # a captured scan replays into the same tensors (the factors are on the device: nothing but kernels and a device copy inside)
    fdev = torch.as_tensor(path).to(db.dev)
    db.scan(fdev)
    torch.cuda.synchronize()
    ref = blk.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        db.scan(fdev)
    blk.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(blk, ref)
    db.check()


# ---- 10. errors ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(rt):
    b = Batch([5, 9], 50)
    path = b.path([1.0, 2.0, 3.0])
    rc, want, _ = raw_scan(rt, b, path)
    assert rc == 0
    for over in (dict(npath=0), dict(npath=-3), dict(npath=1 << 20), dict(sfc_per_path=2), dict(sfc_per_path=-1), dict(nprof=0), dict(nwn=0),
                 dict(nlay_max=0), dict(nlay_max=604)):
        assert raw_scan(rt, b, path, **over)[0] == EARG, over
        assert rt.lib.monortm_hip_last_error(rt.ctx)
    for name in ("wn", "nlay", "irt", "T", "TZ", "O", "path", "ts", "em", "rf", "rup", "rdn", "trtot", "rad", "tb"):
        assert raw_scan(rt, b, path, drop=(name,))[0] == EARG, name
    bad_nlay = copy.copy(b)
    bad_nlay.nlay = np.array([5, 10], np.int32)     # beyond nlay_max = 9
    assert raw_scan(rt, bad_nlay, path)[0] == EARG
    for v in (-1e-3, np.nan, np.inf):
        f = path.copy()
        f[0, 2, 4] = v                               # an active layer of profile 0 (5 layers)
        assert raw_scan(rt, b, f)[0] == EARG, v
    f = path.copy()
    f[0, 1, 5:] = -1.0                               # padded layers of profile 0: ignored
    f[0, 2, 7] = np.nan
    rc, got, _ = raw_scan(rt, b, f)
    assert rc == 0, rt.lib.monortm_hip_last_error(rt.ctx)
    for k in OUT:
        np.testing.assert_array_equal(got[k], want[k])


def test_device_entry_flags_bad_factors(rt):
    import torch

    b = Batch([5, 9], 51)
    path = b.path([1.0, 2.0, 3.0])
    rc, want, _ = raw_scan(rt, b, path)
    assert rc == 0
    dev = torch.device("cuda:0")
    up = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
    wn, nlay, irt = up(b.wn), up(b.nlay, torch.int32), up(b.irt, torch.int32)
    T, TZ, O, em, rf = up(b.pad(b.T, 0.0)), up(b.pad(b.TZ, 0.0)), up(b.pad(b.O, 0.0)), up(b.em), up(b.rf)
    outs = torch.zeros(6, b.nprof, 3, b.nwn, dtype=torch.float64, device=dev)
    d = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(f, npath=3):
        fd, ts = up(f), up(b.ts)
        rc = rt.lib.monortm_hip_rtm_scan_dev(rt.ctx, b.nprof, npath, b.nwn, d(wn), d(nlay), b.lm, d(irt), 1, d(T), d(TZ), d(O), d(fd), d(ts),
                                             0, d(em), d(rf), *[d(outs[k]) for k in range(6)], s)
        return rc, rt.lib.monortm_hip_check(rt.ctx, s)

    assert call(path) == (0, 0)
    for k, name in enumerate(OUT):
        np.testing.assert_array_equal(outs[k].cpu().numpy(), want[name])
    for v in (-2.0, np.nan):
        f = path.copy()
        f[1, 0, 8] = v                               # the last active layer of profile 1
        assert call(f) == (0, EARG), v               # the launch succeeds, the flag tells
        assert rt.lib.monortm_hip_check(rt.ctx, s) == 0   # ... once
    f = path.copy()
    f[0, 0, 6] = -5.0                                # a padded layer
    outs.zero_()
    assert call(f) == (0, 0)
    for k, name in enumerate(OUT):
        np.testing.assert_array_equal(outs[k].cpu().numpy(), want[name])
    assert call(path, npath=0)[0] == EARG
    assert call(path) == (0, 0)
