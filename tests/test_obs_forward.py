"""The forward measurement operator on the GPU (monortm_hip_rtm_obs, monortm_hip_obs and their _dev forms, rtm_obs_kernel.hip;
DESIGN.md section 3.10): Y per measurement (view, channel), contracted inside the kernel, with the band brightness temperature as a
third quantity.

The reference of every comparison is the existing monochromatic entry (monortm_hip_rtm_scan) run in the same test and contracted in
float64 with ObsOperator.dense(); the error of an element is measured against S = sum |wpath_j wchan_i q_ji| of that element
(obs_cases.reference).  Shapes and seeds are those of tests/test_obs_jacobian.py: BATCHES R30 / B30 / C12, 70 wavenumbers (one full
block of 64 lanes and one of 6 live lanes), irt cycling 1, 2, 3; the operators are in tests/obs_cases.py."""
import ctypes as C

import numpy as np
import pytest

import obs_cases as oc
import test_obs_jacobian as oj
import test_scan as ts
import test_scan_jacobian as sj
from monortm_amd import api, synth
from test_obs_forward_cpu import MIXED_CASE, formula_bound

pytestmark = pytest.mark.gpu

NWN = sj.NWN
BATCHES = sj.BATCHES
EARG = 6
FILL = oj.FILL
TOL8 = oj.TOL8                           # two radiance kernels that differ by contraction and summation order only
TOL4 = oj.TOL4                           # one float rounding per monochromatic term of the reference, one in the result
_p, err, handle = sj._p, sj.err, oj.handle
gpu, rt, rt4, case = oj.gpu, oj.rt, oj.rt4, oj.case   # the module-scoped fixtures of tests/test_obs_jacobian.py, one set for this module


def raw_fwd(r, b, path, quantity, h, op, vcen=None, O=None, em=None, rf=None, T=None, TZ=None, only=None, drop=(), **over):
    """monortm_hip_rtm_obs -> (rc, Y pre-filled with FILL).  only = i: profile i alone, its arrays cut to its own nlay (nprof = 1,
    nlay_max = nlay[i]).  drop: names of arrays passed as NULL; over: nprof / npath / nwn / nlay_max / sfc_per_path handed to the call
    instead of the arrays' own."""
    dt = r.dtype
    c = lambda x: np.ascontiguousarray(x, dt)  # noqa: E731
    a = dict(nlay=b.nlay, irt=b.irt, T=b.pad(b.T, 0.0) if T is None else T, TZ=b.pad(b.TZ, 0.0) if TZ is None else TZ,
             O=b.pad(b.O, 0.0) if O is None else O, path=path, ts=b.ts, em=b.em if em is None else em, rf=b.rf if rf is None else rf)
    nprof, lm = b.nprof, b.lm
    if only is not None:
        i, lm, nprof = only, int(b.nlay[only]), 1
        a = dict(nlay=a["nlay"][i:i + 1], irt=a["irt"][i:i + 1], T=a["T"][i:i + 1, :lm], TZ=a["TZ"][i:i + 1, :lm + 1], O=a["O"][i:i + 1, :lm],
                 path=a["path"][i:i + 1, :, :lm], ts=a["ts"][i:i + 1], em=a["em"][i:i + 1], rf=a["rf"][i:i + 1])
    a = {k: (np.ascontiguousarray(v, np.int32) if k in ("nlay", "irt") else c(v)) for k, v in a.items()}
    a["wn"] = b.wn
    a["vcen"] = None if vcen is None else np.ascontiguousarray(vcen, np.float64)
    a["y"] = np.full((nprof, op.nview, op.nchan), FILL, dt)
    g = lambda k: None if k in drop else _p(a[k])  # noqa: E731
    rc = r.lib.monortm_hip_rtm_obs(r.ctx, over.get("nprof", nprof), over.get("npath", a["path"].shape[1]), over.get("nwn", b.nwn), g("wn"),
                                   g("nlay"), over.get("nlay_max", lm), g("irt"), quantity, g("T"), g("TZ"), g("O"), g("path"), g("ts"),
                                   over.get("sfc_per_path", int(a["em"].ndim == 3)), g("em"), g("rf"), h, g("vcen"), g("y"))
    return rc, a["y"]


_MONO = {}


def shared_scan(r, name, views):
    """Batch, paths and monortm_hip_rtm_scan's fields as float64: computed once per (context, batch, number of paths), never modified."""
    npath = sum(oc.VIEWS[views])
    key = (r.real_kind, name, npath)
    if key not in _MONO:
        b = sj.Batch(BATCHES[name], 11 + list(BATCHES).index(name))
        path = b.path(oc.factors(npath))
        rc, m, _ = ts.raw_scan(r, b, path)
        assert rc == 0, err(r)
        m = {k: v.astype(np.float64) for k, v in m.items()}
        for v in m.values():
            v.setflags(write=False)
        _MONO[key] = (b, path, m)
    return _MONO[key]


def check_y(got, mono_q, op, tol, what):
    """|got - ref| <= tol x S per element; where S = 0 (empty views and channels) that asks for an exact 0.  Prints the worst ratio."""
    ref, S = oc.reference(op, mono_q)
    g = np.asarray(got, np.float64)
    assert g.shape == ref.shape and np.all(np.isfinite(g)), what
    e = np.abs(g - ref)
    worst = float(np.max(e / np.where(S > 0, S, 1.0)))
    print(f"{what}: max |got - ref| / S = {worst:.2e}")
    assert np.all(e <= tol * S), f"{what}: {worst:.2e} > {tol:.2e}"
    assert np.all(g[S == 0] == 0)
    return ref, S


# ---- 1. against the monochromatic scan, contracted -------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", [1, 0])
@pytest.mark.parametrize("views,chmap", oc.PAIRS)
@pytest.mark.parametrize("name", list(BATCHES))
def test_forward_equals_contracted_scan(rt, name, views, chmap, quantity):
    """real_kind 8: |got - ref| <= 1e-12 S.  The call gets NaN in every padded entry of O, T, TZ and path, the reference zeros; Y is
    pre-filled, so the zeros of the empty view and of the empty channel are the kernel's.  Instantiations <double, double, 8, 4>
    (R30, B30) and <double, double, 2, 4> (C12); R30 holds profiles of 1, 2 and 7 layers, which work with two of the eight groups."""
    b, path, mono = shared_scan(rt, name, views)
    op = oc.operator(views, chmap, NWN)
    nan = np.nan
    with handle(rt, op) as h:
        rc, got = raw_fwd(rt, b, b.pad(path, nan), quantity, h, op, O=b.pad(b.O, nan), T=b.pad(b.T, nan), TZ=b.pad(b.TZ, nan))
    assert rc == 0, err(rt)
    check_y(got, mono["tb" if quantity else "rad"], op, TOL8, f"{name} {views}/{chmap} q={quantity}")
    assert np.any(got != 0)


# ---- 2. against the adjoint's Y ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", [1, 0])
@pytest.mark.parametrize("views,chmap", oc.PAIRS)
@pytest.mark.parametrize("name", list(BATCHES))
def test_forward_equals_the_adjoints_y(rt, name, views, chmap, quantity):
    """Y of monortm_hip_rtm_obs_jac on the same inputs: 1e-12 S.  The design's aim is bit-equality (the same owner, the same order);
    it rests on two separately compiled kernels contracting alike, so the number of elements that differ is printed, not asserted."""
    b, path, mono = shared_scan(rt, name, views)
    op = oc.operator(views, chmap, NWN)
    with handle(rt, op) as h:
        rc, got = raw_fwd(rt, b, path, quantity, h, op)
        assert rc == 0, err(rt)
        rc, adj = oj.raw_obs(rt, b, path, quantity, h, op)
        assert rc == 0, err(rt)
    _, S = oc.reference(op, mono["tb" if quantity else "rad"])
    print(f"{name} {views}/{chmap} q={quantity}: {int(np.sum(got != adj['y']))} of {got.size} elements differ from the adjoint's Y in some bit")
    assert np.all(np.abs(got - adj["y"]) <= TOL8 * S)


# ---- 3. the band brightness temperature -------------------------------------------------------------------------------------------------
def centres(op, wn, weighted=True):
    """Per channel the mean wavenumber of its members, weighted with wchan (positive weights) or plain (weights of mixed sign, whose
    weighted mean may lie anywhere); 1 for a channel without members: any valid value."""
    v = np.ones(op.nchan)
    for c in range(op.nchan):
        m = op.chan == c
        if m.any():
            v[c] = np.sum(op.wchan[m] * wn[m]) / np.sum(op.wchan[m]) if weighted else np.mean(wn[m])
    return v


@pytest.mark.parametrize("views", ["A", "B", "C"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_band_tb(rt, name, views):
    """Normalised positive weights (mixed=False) on the comb map, vcen = the weighted mean wavenumber of each channel.  Reference:
    api.band_tb of the float64 contraction of monortm_hip_rtm_scan's RAD.  Bound: the radiance's 1e-12 S carried through the
    conversion, band_tb_slope x 1e-12 S, plus the conversion's own rounding, formula_bound x TB (tests/test_obs_forward_cpu.py)."""
    b, path, mono = shared_scan(rt, name, views)
    op = oc.operator(views, "comb", NWN, mixed=False)
    vcen = centres(op, b.wn)
    with handle(rt, op) as h:
        rc, got = raw_fwd(rt, b, path, 2, h, op, vcen=vcen)
    assert rc == 0, err(rt)
    yr, S = oc.reference(op, mono["rad"])
    ref = api.band_tb(vcen, yr)
    live = S > 0
    assert np.all(yr[live] > 0) and np.all(got[~live] == 0) and np.all(np.isfinite(got))
    bound = api.band_tb_slope(vcen, np.where(live, yr, 1.0)) * TOL8 * S + np.broadcast_to(formula_bound(vcen, np.where(live, yr, 1.0)), yr.shape) * ref
    e = np.abs(got - ref)
    print(f"band TB {name} {views}: max error / bound = {float(np.max(e[live] / bound[live])):.3f}, TB {ref[live].min():.1f} .. {ref[live].max():.1f} K")
    assert np.all(e[live] <= bound[live])
    assert np.all(got[live] > 0)


def test_band_tb_mixed_sign_weights(rt):
    """Mixed-sign weights on the nested map: an element is NaN exactly where the float64 reference radiance is <= 0, 0 exactly where
    it has no sample, and the band temperature elsewhere.  Elements with |Y_rad| < 1e-12 S have no determined sign and are left out;
    they may be at most 5 % of the non-empty elements (tests/test_obs_forward_cpu.py checks that share on the oracle's radiances)."""
    name, views, chmap = MIXED_CASE
    b, path, mono = shared_scan(rt, name, views)
    op = oc.operator(views, chmap, NWN)
    vcen = centres(op, b.wn, weighted=False)
    with handle(rt, op) as h:
        rc, got = raw_fwd(rt, b, path, 2, h, op, vcen=vcen)
    assert rc == 0, err(rt)
    yr, S = oc.reference(op, mono["rad"])
    live = S > 0
    decided = live & (np.abs(yr) >= TOL8 * S)
    assert np.sum(live & ~decided) <= 0.05 * np.sum(live)
    assert np.all(got[~live] == 0) and np.any(~live)
    neg = decided & (yr <= 0)
    pos = decided & (yr > 0)
    assert neg.any() and pos.any()
    assert np.all(np.isnan(got[neg])) and np.all(np.isfinite(got[pos]))
    ref = api.band_tb(vcen, np.where(pos, yr, 1.0))
    bound = api.band_tb_slope(vcen, np.where(pos, yr, 1.0)) * TOL8 * S + np.broadcast_to(formula_bound(vcen, np.where(pos, yr, 1.0)), yr.shape) * ref
    assert np.all(np.abs(got - ref)[pos] <= bound[pos])


# ---- 4. the identity operator -----------------------------------------------------------------------------------------------------------
def test_identity_operator_gives_the_monochromatic_fields(rt):
    """nview = npath = 5, nchan = nwn = 70 (more channels than lanes: owner lanes serve two), unit weights: Y is RAD / TB of
    monortm_hip_rtm_scan at 1e-12 of its magnitude, and the band TB with vcen = wn is its TB."""
    b = sj.Batch(BATCHES["B30"], 21)
    path = b.path(oc.factors(5))
    op = oc.identity(5, NWN)
    rc, mono, _ = ts.raw_scan(rt, b, path)
    assert rc == 0
    with handle(rt, op) as h:
        for quantity, k in ((1, "tb"), (0, "rad"), (2, "tb")):
            rc, got = raw_fwd(rt, b, path, quantity, h, op, vcen=b.wn if quantity == 2 else None)
            assert rc == 0, err(rt)
            print(f"identity q={quantity}: {int(np.sum(got != mono[k]))} of {got.size} elements differ in some bit")
            np.testing.assert_allclose(got, mono[k], rtol=1e-12, atol=0, err_msg=k)


# ---- 5. real_kind 4 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", [1, 0])
@pytest.mark.parametrize("views,chmap", oc.PAIRS)
@pytest.mark.parametrize("name", list(BATCHES))
def test_forward_real_kind_4(rt4, name, views, chmap, quantity):
    """float32 arrays, double arithmetic: |got - ref| <= 2.5 x 2^-24 S against the float64 contraction of the real_kind 4 scan - one
    float rounding per monochromatic term in the reference, one in the result: the host entry holds the sums in double and rounds
    once.  Instantiations <float, double, 8, 4> and <float, double, 2, 4>."""
    b, path, mono = shared_scan(rt4, name, views)
    op = oc.operator(views, chmap, NWN)
    with handle(rt4, op) as h:
        rc, got = raw_fwd(rt4, b, path, quantity, h, op)
    assert rc == 0, err(rt4)
    assert got.dtype == np.float32
    check_y(got, mono["tb" if quantity else "rad"], op, TOL4, f"real_kind 4 {name} {views}/{chmap} q={quantity}")


def device_arrays(r, b, path):
    import torch

    dev = torch.device("cuda:0")
    real = torch.float32 if r.real_kind == 4 else torch.float64
    up = lambda x, dt=real: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
    a = dict(wn=up(b.wn, torch.float64), nlay=up(b.nlay, torch.int32), irt=up(b.irt, torch.int32))
    a.update({k: up(x) for k, x in dict(T=b.pad(b.T, 0.0), TZ=b.pad(b.TZ, 0.0), O=b.pad(b.O, 0.0), em=b.em, rf=b.rf, ts=b.ts, path=path).items()})
    return a, up, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def dev_call(r, b, a, h, quantity, y, s, path=None, vcen=None, npath=None):
    d = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    f = a["path"] if path is None else path
    return r.lib.monortm_hip_rtm_obs_dev(r.ctx, b.nprof, f.shape[1] if npath is None else npath, b.nwn, d(a["wn"]), d(a["nlay"]), b.lm, d(a["irt"]),
                                         quantity, d(a["T"]), d(a["TZ"]), d(a["O"]), d(f), d(a["ts"]), 0, d(a["em"]), d(a["rf"]), h, d(vcen), d(y), s)


@pytest.mark.parametrize("name,views,chmap", [("B30", "C", "nested"), ("C12", "B", "comb")])
def test_device_entry_real_kind_4(rt4, name, views, chmap):
    """monortm_hip_rtm_obs_dev on a real_kind 4 context: instantiations <float, float, 8, 4> and <float, float, 2, 4>, whose float Y
    holds the running sum itself.  An element of (view v, channel c) receives one contribution per tile of 4 paths of v and block of
    64 wavenumbers that holds a member of c, each added with one float rounding of a partial sum that is at most S:
    |got - ref| <= (1 + tiles(v) x blocks(c)) x 2^-24 S, the 1 for the roundings of the reference's monochromatic terms."""
    import torch

    b, path, mono = shared_scan(rt4, name, views)
    op = oc.operator(views, chmap, NWN)
    tiles = -(-np.diff(op.view_start) // 4)
    blocks = np.array([len(set(np.nonzero(op.chan == c)[0] // 64)) for c in range(op.nchan)])
    ncontrib = (tiles[:, None] * blocks[None, :])[None]              # [1, nview, nchan]
    assert ncontrib.max() >= 4
    a, up, s = device_arrays(rt4, b, path)
    y = torch.full((b.nprof, op.nview, op.nchan), FILL, dtype=torch.float32, device=a["wn"].device)
    with handle(rt4, op) as h:
        assert dev_call(rt4, b, a, h, 1, y, s) == 0, err(rt4)
        assert rt4.lib.monortm_hip_check(rt4.ctx, s) == 0
        got = y.cpu().numpy()
    ref, S = oc.reference(op, mono["tb"])
    e = np.abs(got.astype(np.float64) - ref)
    bound = (1 + ncontrib) * 2.0 ** -24 * S
    print(f"real_kind 4 device entry {name}: max |got - ref| / bound = {float(np.max(e / np.where(bound > 0, bound, 1.0))):.2f}")
    assert np.all(e <= bound)


# ---- 6. the full entry --------------------------------------------------------------------------------------------------------------------
def full_profiles(wn, nlays):
    return [synth.perturbed_profile(450 + i, wn, nlay=n, cloud=True, irt=irt) for i, (n, irt) in enumerate(zip(nlays, (1, 3, 2)))]


@pytest.mark.parametrize("nlays", [(20, 16, 18), (30, 7, 16)])
@pytest.mark.parametrize("real_kind", [8, 4])
def test_full_entry_is_modm_then_the_forward_kernel(case, nlays, real_kind):
    """monortm_hip_obs: O bit-equal to monortm_hip_modm's on the same inputs, Y bit-equal to monortm_hip_rtm_obs on that O (the same
    kernel on the same O) - for all three quantities, and on a real_kind 4 context, which no Jacobian entry serves."""
    t3, wn, rt8 = case
    r = rt8 if real_kind == 8 else api.MonoRTM(t3, wn[0], wn[-1], real_kind=4)
    prs = full_profiles(wn, nlays)
    path = oc.factors(9)[:, None] * (1.0 + 0.01 * np.arange(max(nlays)) / (max(nlays) - 1.0))[None, :]
    op = oc.operator("A", "comb", len(wn), mixed=False)
    vcen = centres(op, wn)
    O = r.modm(prs)[0]
    with handle(r, op) as h:
        for q in ("tb", "rad", "band_tb"):
            full = r.obs(prs, path, h, quantity=q, vcen=vcen)
            part = r.rtm_obs(prs, O, path, h, quantity=q, vcen=vcen)
            assert full["y"].dtype == r.dtype and full["y"].shape == (3, op.nview, op.nchan)
            np.testing.assert_array_equal(full["o"], O)
            np.testing.assert_array_equal(full["y"], part["y"])
            assert np.all(np.isfinite(full["y"])) and np.all(full["y"] > 0)
    if real_kind == 4:
        r.close()


def test_full_entry_matches_oracle_end_to_end(case):
    """Y of the full entry against the oracle's TB along every path - Oracle.run on the profile with amounts scaled by the path's
    factors - contracted in float64; 1e-6 relative, the project's parity bound (tests/test_obs_jacobian.py's case and operator)."""
    from oracle.pyoracle import Oracle

    t3, wn, rt = case
    pr = synth.perturbed_profile(410, wn, nlay=12, cloud=True, irt=1)
    path = api.plane_parallel_path([0.0, 20.0, 30.0, 40.0, 50.0, 55.0, 60.0, 65.0, 70.0], 12)
    ch, _, nchan = oc.nested_map(len(wn))
    op, perm = api.ObsOperator.from_sets(views=[[8, 0, 3, 5], [1], [2, 4, 6, 7]], channels=[list(np.nonzero(ch == c)[0]) for c in range(nchan)],
                                         npath=9, nwn=len(wn))
    with handle(rt, op) as h:
        got = rt.obs([pr], path[perm], h)
    orc = Oracle(t3, wn[0], wn[-1])
    tb = np.array([orc.run(sj.scaled(pr, path[j])).tb for j in perm])[None]      # [1, npath, nwn], the operator's path order
    orc.close()
    ref, S = oc.reference(op, tb)
    live = S > 0
    e = float(np.max(np.abs(got["y"] - ref)[live] / np.abs(ref)[live]))
    print(f"Y against the oracle: {e:.2e}")
    assert e <= 1e-6 and np.all(got["y"][~live] == 0) and np.sum(live) == 3 * 6


# ---- 7. determinism and batch independence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R30", "C12"])
def test_bit_identical_twice_and_alone(rt, name):
    """Two calls give the same bits; profile i of the ragged batch gives the bits of the same profile alone (nprof = 1, its own nlay as
    nlay_max - for R30's profiles of 1, 2 and 7 layers that is the G = 2 instantiation against the batch's G = 8)."""
    b, path, _ = shared_scan(rt, name, "B")
    op = oc.operator("B", "nested", NWN)
    vcen = centres(op, b.wn, weighted=False)
    with handle(rt, op) as h:
        for q in (1, 0, 2):
            rc, one = raw_fwd(rt, b, path, q, h, op, vcen=vcen)
            assert rc == 0, err(rt)
            rc, two = raw_fwd(rt, b, path, q, h, op, vcen=vcen)
            assert rc == 0
            np.testing.assert_array_equal(one, two)
            for i in range(b.nprof):
                rc, alone = raw_fwd(rt, b, path, q, h, op, vcen=vcen, only=i)
                assert rc == 0, err(rt)
                np.testing.assert_array_equal(alone[0], one[i])


# ---- 8. multi-device contexts -------------------------------------------------------------------------------------------------------------
def test_multi_device_context(rt, monkeypatch):
    """Three shards on device 0: R30's four profiles go 2 / 2 / 0 (an empty shard), a batch of five 2 / 2 / 1 (a ragged one).  Bits of
    the one-device call; a bad factor in the last shard is refused before any launch."""
    monkeypatch.setenv("MONORTM_DEVICES", "0,0,0")
    m = api.MonoRTM("", 0.0, 0.0, ngpu=0)
    assert m.lib.monortm_hip_device_count(m.ctx) == 3
    op = oc.operator("A", "nested", NWN)
    vcen = centres(op, np.linspace(15.0, 250.0, NWN), weighted=False)
    with handle(rt, op) as h1, handle(m, op) as h2:
        for b in (shared_scan(rt, "R30", "A")[0], sj.Batch([4, 30, 11, 26, 19], 40)):
            path = b.path(oc.factors(9))
            for q in (1, 2):
                rc, one = raw_fwd(rt, b, path, q, h1, op, vcen=vcen)
                assert rc == 0
                rc, two = raw_fwd(m, b, path, q, h2, op, vcen=vcen)
                assert rc == 0, err(m)
                np.testing.assert_array_equal(two, one)
        f = path.copy()
        f[4, 3, 18] = -1.0                              # the last active layer of the last profile
        rc, got = raw_fwd(m, b, f, 1, h2, op)
        assert rc == EARG and b"profile 4 path 3 layer 18" in err(m) and np.all(got == FILL)
        rc, again = raw_fwd(m, b, path, 2, h2, op, vcen=vcen)
        assert rc == 0, err(m)
        np.testing.assert_array_equal(again, one)
    m.close()


def test_full_entry_multi_device(tmp_path, monkeypatch):
    """monortm_hip_obs over three shards (seven profiles go 3 / 3 / 1, four 2 / 2 / 0): O and Y are the one-device call's bits.
    On the workload of tests/test_multi_device.py, for which the suite holds monortm_hip_modm itself to the one-device bits: MODM
    shapes its line-sum launch by the number of states in the call, so on other line lists a shard's O may differ from the whole
    batch's in the last bit (tests/test_obs_jacobian.py::test_full_entry_multi_device; with the line list of `case` here: 25 % of
    the elements, 8.8e-16 relative): the entry runs per shard the MODM call monortm_hip_modm runs for it.  The premise - MODM sharding
    to the same bits on this workload - is asserted first."""
    import test_multi_device as md
    from monortm_amd import tape3

    t3 = str(tmp_path / "TAPE3")
    tape3.write_tape3(t3, synth.synthetic_lines(150, seed=12, lc_frac=0.5, sdep_frac=0.1))
    all7 = md._profiles(7)
    wn = all7[0].wn
    rt = api.MonoRTM(t3, wn[0], wn[-1])
    monkeypatch.setenv("MONORTM_DEVICES", "0,0,0")
    m = api.MonoRTM(t3, wn[0], wn[-1], ngpu=0)
    assert m.lib.monortm_hip_device_count(m.ctx) == 3
    op = oc.operator("A", "comb", len(wn), mixed=False)
    vcen = centres(op, wn)
    path = oc.factors(9)[:, None] * np.ones(20)[None, :]
    with handle(rt, op) as h1, handle(m, op) as h2:
        for n in (7, 4):
            prs = all7[:n]
            np.testing.assert_array_equal(m.modm(prs)[0], rt.modm(prs)[0])     # the premise: MODM shards to the same bits here
            for q in ("tb", "band_tb"):
                one = rt.obs(prs, path, h1, quantity=q, vcen=vcen)
                two = m.obs(prs, path, h2, quantity=q, vcen=vcen)
                np.testing.assert_array_equal(two["o"], one["o"])
                np.testing.assert_array_equal(two["y"], one["y"])
        f = np.broadcast_to(path[None], (4,) + path.shape).copy()
        f[3, 8, 12] = -0.5                               # the last active layer of the last profile (13 layers), in the last shard in use
        with pytest.raises(api.MonoRTMError) as e:
            m.obs(prs, f, h2)
        assert e.value.code == EARG and "profile 3 path 8 layer 12" in str(e.value)
    m.close()
    rt.close()


# ---- 9. DeviceBatch.obs -------------------------------------------------------------------------------------------------------------------
def test_device_batch_obs_and_graph_replay(case):
    """DeviceBatch.obs against MonoRTM.obs, bit for bit (the same kernels on the same inputs); one capture, new factors in the device
    tensor, a replay into the same (overwritten) tensor, against the host entry on the new factors; after obs_destroy the cached
    tensors go and the stale handle is refused."""
    import torch

    _, wn, rt = case
    prs = full_profiles(wn, (20, 16, 18))
    path = oc.factors(9)[:, None] * (1.0 + 0.01 * np.arange(20) / 19.0)[None, :]
    op = oc.operator("A", "comb", len(wn), mixed=False)
    vcen = centres(op, wn)
    db = api.DeviceBatch(rt, prs)
    fdev = torch.as_tensor(path).to(db.dev)
    vdev = torch.as_tensor(vcen).to(db.dev)
    with handle(rt, op) as h:
        for q in ("tb", "band_tb"):
            ref = rt.obs(prs, path, h, quantity=q, vcen=vcen)
            got = db.obs(fdev, h, quantity=q, vcen=vdev)
            torch.cuda.synchronize()
            db.check()
            np.testing.assert_array_equal(got.cpu().numpy(), ref["y"])
            np.testing.assert_array_equal(db.O.cpu().numpy(), ref["o"])
            assert db.obs(fdev, h, quantity=q, vcen=vdev) is got    # overwritten in place
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                db.obs(fdev, h, quantity="band_tb", vcen=vdev)
        torch.cuda.current_stream().wait_stream(s)
        path2 = path[::-1] * 1.25
        fdev.copy_(torch.as_tensor(np.ascontiguousarray(path2)))
        got.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        db.check()
        ref2 = rt.obs(prs, path2, h, quantity="band_tb", vcen=vcen)
        assert not np.array_equal(ref2["y"], ref["y"])
        np.testing.assert_array_equal(got.cpu().numpy(), ref2["y"])
        assert sorted(k[0] for k in db._obs_fwd) == [h, h]
    with pytest.raises(api.MonoRTMError):
        db.obs(fdev, h)                                  # the stale handle
    assert db._obs_fwd == {}
    with pytest.raises(api.MonoRTMError):
        rt.obs(prs, path, h)


# ---- 10. nothing else moves ---------------------------------------------------------------------------------------------------------------
def test_forward_calls_between_modm_and_rtm_change_nothing(case):
    _, wn, rt = case
    prs = full_profiles(wn, (20, 16, 18))
    path = oc.factors(9)[:, None] * np.ones(20)[None, :]
    op = oc.operator("A", "comb", len(wn))
    cnt = lambda: (rt.counter(0), rt.counter(1))  # noqa: E731
    c0 = cnt()
    O = rt.modm(prs)[0]
    tb0 = rt.rtm(prs, O)[4]
    sc0 = rt.rtm_scan(prs, O, path)["tb"]
    c1 = cnt()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 1)
    O = rt.modm(prs)[0]
    with handle(rt, op) as h:
        rt.rtm_obs(prs, O, path, h)
        rt.obs(prs, path, h)
        assert cnt() == c1                               # neither call counts as, or is, a reader of the resident O
    tb1 = rt.rtm(prs, O)[4]
    sc1 = rt.rtm_scan(prs, O, path)["tb"]
    c2 = cnt()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (1, 1)      # the pair after the calls still finds its O resident
    assert np.array_equal(tb0, tb1) and np.array_equal(sc0, sc1)


# ---- 11. surface arrays per path, a layer that does not absorb ----------------------------------------------------------------------------
def test_surface_arrays_per_path(rt):
    b = sj.Batch(BATCHES["B30"], 23, irt=(1,))
    op = oc.operator("A", "nested", NWN)
    path = b.path(oc.factors(9))
    rng = np.random.default_rng(5)
    em = rng.uniform(0.5, 1.0, (b.nprof, 9, b.nwn))
    rf = 1.0 - em
    rc, mono, _ = ts.raw_scan(rt, b, path, em=em, rf=rf)
    assert rc == 0
    with handle(rt, op) as h:
        rc, got = raw_fwd(rt, b, path, 1, h, op, em=em, rf=rf)
        assert rc == 0, err(rt)
        check_y(got, mono["tb"], op, TOL8, "surface per path")
        rc, shared = raw_fwd(rt, b, path, 1, h, op)
        assert rc == 0
        assert not np.array_equal(got, shared)
        rep = lambda x: np.ascontiguousarray(np.broadcast_to(x[:, None, :], (b.nprof, 9, b.nwn)))  # noqa: E731
        rc, replicated = raw_fwd(rt, b, path, 1, h, op, em=rep(b.em), rf=rep(b.rf))
        assert rc == 0
    np.testing.assert_array_equal(replicated, shared)


def test_zero_factor_layer(rt):
    """A layer that does not absorb along some paths of a view: Y still equals the contracted per-path reference."""
    b = sj.Batch(BATCHES["C12"], 22)
    op = oc.operator("A", "comb", NWN)
    path = b.path(oc.factors(9))
    path[:, 1, 2] = 0.0
    path[1, 4, 11] = 0.0
    path[:, 5:, 0] = 0.0
    rc, mono, _ = ts.raw_scan(rt, b, path)
    assert rc == 0
    with handle(rt, op) as h:
        rc, got = raw_fwd(rt, b, path, 1, h, op)
    assert rc == 0, err(rt)
    check_y(got, mono["tb"], op, TOL8, "zero factor")


# ---- 12. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(rt, rt4):
    b, path, _ = shared_scan(rt, "C12", "A")
    op = oc.operator("A", "nested", NWN)
    vcen = np.linspace(20.0, 200.0, op.nchan)
    with handle(rt, op) as h:
        rc, want = raw_fwd(rt, b, path, 2, h, op, vcen=vcen)
        assert rc == 0

        def refused(*a, **kw):
            rc, got = raw_fwd(rt, b, *a, **kw)
            return rc == EARG and bool(err(rt)) and np.all(got == FILL)

        assert refused(path, 1, h, op, drop=("y",))
        for name in ("wn", "nlay", "irt", "T", "TZ", "O", "path", "ts", "em", "rf"):
            assert refused(path, 1, h, op, drop=(name,)), name
        # a call whose npath or nwn is not the handle's; destroyed, never created, foreign handles
        op13 = oc.operator("B", "nested", NWN)
        with handle(rt, op13) as h13:
            assert refused(path, 1, h13, op) and b"npath = 13" in err(rt)
        with handle(rt, oc.operator("A", "nested", 60)) as h60:
            assert refused(path, 1, h60, op) and b"nwn = 60" in err(rt)
        assert refused(path, 1, h13, op) and b"handle" in err(rt)
        for hb in (0, -1, h + 16, 1 << 30):
            assert refused(path, 1, hb, op), hb
        with handle(rt4, op) as h4:
            assert h4 != h and refused(path, 1, h4, op)
        for over in (dict(npath=0), dict(npath=8), dict(nprof=0), dict(nwn=0), dict(nwn=69), dict(nlay_max=0), dict(nlay_max=604), dict(sfc_per_path=2)):
            assert refused(path, 1, h, op, **over), over
        for q in (3, -1):
            assert refused(path, q, h, op, vcen=vcen), q
        # quantity 2: vcen missing, zero, negative, NaN, infinite - anywhere in the array
        assert refused(path, 2, h, op)
        for i, v in ((0, 0.0), (3, -5.0), (op.nchan - 1, np.nan), (5, np.inf)):
            bad = vcen.copy()
            bad[i] = v
            assert refused(path, 2, h, op, vcen=bad) and b"vcen[%d]" % i in err(rt), (i, v)
            rc, got = raw_fwd(rt, b, path, 1, h, op, vcen=bad)       # ignored by the other quantities
            assert rc == 0
        for v in (-1e-3, np.nan, np.inf):
            f = path.copy()
            f[0, 2, 2] = v                               # an active layer of profile 0 (3 layers)
            assert refused(f, 2, h, op, vcen=vcen), v
        f = path.copy()
        f[0, 1, 3:] = -1.0                               # padded layers of profile 0: ignored
        rc, got = raw_fwd(rt, b, f, 2, h, op, vcen=vcen)
        assert rc == 0, err(rt)
        np.testing.assert_array_equal(got, want)


def test_full_entry_refusals(case):
    _, wn, rt = case
    prs = [synth.perturbed_profile(490, wn, nlay=16)]
    op = oc.operator("A", "nested", len(wn))
    one = np.ones((9, 16))
    vcen = np.linspace(1.0, 20.0, op.nchan)
    with handle(rt, op) as h:
        for kw in (dict(quantity=3), dict(quantity=-1)):
            with pytest.raises(api.MonoRTMError) as e:
                rt.obs(prs, one, h, **kw)
            assert e.value.code == EARG, kw
        f = one.copy()
        f[8, 15] = np.nan
        with pytest.raises(api.MonoRTMError) as e:
            rt.obs(prs, f, h)
        assert e.value.code == EARG and "path 8 layer 15" in str(e.value)
        with pytest.raises(api.MonoRTMError):
            rt.obs(prs, np.ones((5, 16)), h)             # npath is not the handle's
        res = rt.obs(prs, one, h, quantity="band_tb", vcen=vcen)
        # (weights of mixed sign: an element is a temperature or NaN; the channel without a member is 0)
        assert np.all(np.isfinite(res["o"])) and np.all(res["y"][:, :, [0, 1, 2, 3, 4, 6]] != 0) and np.all(res["y"][:, :, 5] == 0)
        assert np.any(np.isfinite(res["y"][:, :, [0, 1, 2, 3, 4, 6]]))


def test_device_entry_flags_bad_factors_and_bad_vcen(rt):
    import torch

    b, path, _ = shared_scan(rt, "C12", "A")
    op = oc.operator("A", "nested", NWN)
    vcen = np.linspace(20.0, 200.0, op.nchan)
    a, up, s = device_arrays(rt, b, path)
    y = torch.full((b.nprof, op.nview, op.nchan), FILL, dtype=torch.float64, device=a["wn"].device)
    with handle(rt, op) as h:
        rc, want = raw_fwd(rt, b, path, 2, h, op, vcen=vcen)
        assert rc == 0

        def call(f=path, v=vcen, q=2, **kw):
            rc = dev_call(rt, b, a, kw.pop("hh", h), q, y, s, path=up(f), vcen=None if v is None else up(v, torch.float64), **kw)
            return rc, rt.lib.monortm_hip_check(rt.ctx, s)

        assert call() == (0, 0)
        np.testing.assert_array_equal(y.cpu().numpy(), want)          # the device entry's bits are the host entry's
        for v in (-2.0, np.nan, np.inf):
            f = path.copy()
            f[1, 8, 11] = v                              # the last active layer of profile 1, last path of the last view
            assert call(f) == (0, EARG), v               # the launch succeeds, the flag tells
            assert rt.lib.monortm_hip_check(rt.ctx, s) == 0   # ... once
        for i, v in ((0, 0.0), (op.nchan - 1, np.nan), (3, -1.0), (5, np.inf)):   # (channel 5 has no member: its vcen is checked all the same)
            bad = vcen.copy()
            bad[i] = v
            assert call(v=bad) == (0, EARG), (i, v)
            assert rt.lib.monortm_hip_check(rt.ctx, s) == 0
            assert call(v=bad, q=1) == (0, 0)            # not read by the other quantities
        f = path.copy()
        f[0, 0, 6] = -5.0                                # a padded layer
        assert call(f) == (0, 0)
        np.testing.assert_array_equal(y.cpu().numpy(), want)
        assert call(v=None)[0] == EARG                   # quantity 2 without vcen
        assert call(npath=8)[0] == EARG
        assert call(hh=h + 16)[0] == EARG
        assert call() == (0, 0)
        np.testing.assert_array_equal(y.cpu().numpy(), want)
