"""Channel- and beam-averaged Jacobians on the GPU (monortm_hip_obs_create, monortm_hip_rtm_obs_jac, monortm_hip_obs_jacobian and their
_dev forms, rtm_obs_jac_kernel.hip): K per measurement (view, channel), contracted inside the kernel.

The reference of every comparison is the existing monochromatic entry (monortm_hip_rtm_scan_jac / monortm_hip_scan_jacobian) run in the
same test and contracted in float64 with ObsOperator.dense(); the error of an element is measured against S = sum |wpath_j wchan_i
term_ji| of that element (obs_cases.reference).  Shapes and seeds are those of tests/test_scan_jacobian.py: BATCHES R30 / B30 / C12,
70 wavenumbers (one full block of 64 lanes and one of 6 live lanes), irt cycling 1, 2, 3, both quantities; the operators are in
tests/obs_cases.py."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest

import obs_cases as oc
import test_scan_jacobian as sj
from monortm_amd import api, synth, tape3

pytestmark = pytest.mark.gpu

NWN = sj.NWN
BATCHES = sj.BATCHES
EARG = 6
FILL = -7.0
RTM_OUT = api.OBS_JAC_RTM_FIELDS         # y, k_t, k_tz, k_sfc: the output order of monortm_hip_rtm_obs_jac
FULL_OUT = api.OBS_JAC_FIELDS            # o, y, k_t, k_tz, k_w, k_clw, k_sfc: of monortm_hip_obs_jacobian
TOL8 = 1e-12                             # two radiance-adjoint kernels that differ by contraction and summation order only
TOL4 = 2.5 * 2.0 ** -24                  # one float rounding per monochromatic term of the reference, one in the result
_p, err = sj._p, sj.err


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
    t3 = f"{workdir}/TAPE3_obs_jac"
    tape3.write_tape3(t3, synth.synthetic_lines(300, seed=777, lc_frac=0.5, sdep_frac=0.2))
    wn = np.unique(np.concatenate([synth.c2_channels(12, seed=11), synth.sounder_channels()]))
    r = api.MonoRTM(t3, wn[0], wn[-1])
    yield t3, wn, r
    r.close()


@contextlib.contextmanager
def handle(r, op):
    h = r.obs_create(op)
    try:
        yield h
    finally:
        r.obs_destroy(h)


def out_shapes(b, op):
    n, lm, nv, nc = b.nprof, b.lm, op.nview, op.nchan
    return dict(y=(n, nv, nc), k_t=(n, nv, lm, nc), k_tz=(n, nv, lm + 1, nc), k_sfc=(n, nv, 3, nc))


def raw_obs(r, b, path, quantity, h, op, O=None, em=None, rf=None, T=None, TZ=None, only=None, drop=(), **over):
    """monortm_hip_rtm_obs_jac -> (rc, dict of outputs pre-filled with FILL).  only = i: profile i alone, its arrays cut to its own nlay
    (nprof = 1, nlay_max = nlay[i]).  drop: names of arrays passed as NULL; over: nprof / npath / nwn / nlay_max / sfc_per_path handed to
    the call instead of the arrays' own."""
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
    npath = a["path"].shape[1]
    sh = dict(y=(nprof, op.nview, op.nchan), k_t=(nprof, op.nview, lm, op.nchan), k_tz=(nprof, op.nview, lm + 1, op.nchan),
              k_sfc=(nprof, op.nview, 3, op.nchan))
    outs = {k: np.full(s, FILL, dt) for k, s in sh.items()}
    g = lambda k: None if k in drop else _p(a[k] if k in a else outs[k])  # noqa: E731
    rc = r.lib.monortm_hip_rtm_obs_jac(r.ctx, over.get("nprof", nprof), over.get("npath", npath), over.get("nwn", b.nwn), g("wn"), g("nlay"),
                                       over.get("nlay_max", lm), g("irt"), quantity, g("T"), g("TZ"), g("O"), g("path"), g("ts"),
                                       over.get("sfc_per_path", int(a["em"].ndim == 3)), g("em"), g("rf"), h, *[g(k) for k in RTM_OUT])
    return rc, outs


def mono_ref(r, b, path, quantity, **kw):
    """The monochromatic per-path fields of monortm_hip_rtm_scan_jac as float64; y = tb or rad by quantity."""
    rc, m = sj.raw_scan_jac(r, b, path, quantity, **kw)
    assert rc == 0, err(r)
    m = {k: v.astype(np.float64) for k, v in m.items()}
    m["y"] = m["tb"] if quantity == 1 else m["rad"]
    return m


def check_fields(got, mono, op, tol, fields, what=""):
    """|got - ref| <= tol x S for every element of every field; where S = 0 (empty views and channels, padded layers and levels) that
    asks for an exact 0.  Prints the worst ratio of each field."""
    worst = {}
    for k in fields:
        ref, S = oc.reference(op, mono[k])
        g = np.asarray(got[k], np.float64)
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        assert np.all(np.isfinite(g)), f"{what}: {k}"
        e = np.abs(g - ref)
        worst[k] = float(np.max(e / np.where(S > 0, S, 1.0)))
        print(f"{what}: {k} max |got - ref| / S = {worst[k]:.2e}")
        assert np.all(e <= tol * S), f"{what}: {k} {worst[k]:.2e} > {tol:.2e}"
    return worst


_MONO = {}


def shared_mono(r, name, views, quantity):
    """Batch, paths and the monochromatic reference: computed once per (context, batch, number of paths, quantity), never modified."""
    npath = sum(oc.VIEWS[views])
    key = (r.real_kind, name, npath, quantity)
    if key not in _MONO:
        b = sj.Batch(BATCHES[name], 11 + list(BATCHES).index(name))
        path = b.path(oc.factors(npath))
        m = mono_ref(r, b, path, quantity)
        for v in m.values():
            v.setflags(write=False)
        _MONO[key] = (b, path, m)
    return _MONO[key]


# ---- 1. the adjoint against rtm_scan_jacobian, contracted --------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", [1, 0])
@pytest.mark.parametrize("views,chmap", oc.PAIRS)
@pytest.mark.parametrize("name", list(BATCHES))
def test_adjoint_equals_contracted_scan_jacobian(rt, name, views, chmap, quantity):
    """real_kind 8: |got - ref| <= 1e-12 S - the bound the project asserts for two radiance-adjoint kernels that differ by contraction
    only (LABNOTES section 15 measured 3.8e-14 against it); reordering at most 21 x 70 terms adds under 2e-13 S.  The call gets NaN in every
    padded entry of O, T, TZ and path, the reference zeros; the outputs are pre-filled, so the zeros of padded layers and levels, of the
    empty view and of the empty channel are the kernel's.  Instantiations <double, double, 8, 4, false> (R30, B30) and
    <double, double, 2, 4, false> (C12); R30 holds profiles of 1, 2 and 7 layers, which work with two of the eight layer groups."""
    b, path, mono = shared_mono(rt, name, views, quantity)
    op = oc.operator(views, chmap, NWN)
    nan = np.nan
    with handle(rt, op) as h:
        rc, got = raw_obs(rt, b, b.pad(path, nan), quantity, h, op, O=b.pad(b.O, nan), T=b.pad(b.T, nan), TZ=b.pad(b.TZ, nan))
    assert rc == 0, err(rt)
    check_fields(got, mono, op, TOL8, RTM_OUT, what=f"{name} {views}/{chmap} q={quantity}")
    assert all(np.any(got[k] != 0) for k in RTM_OUT)


@pytest.mark.parametrize("quantity", [1, 0])
@pytest.mark.parametrize("views,chmap", oc.PAIRS)
@pytest.mark.parametrize("name", list(BATCHES))
def test_adjoint_real_kind_4(rt4, name, views, chmap, quantity):
    """float32 arrays, double arithmetic: |got - ref| <= 2.5 x 2^-24 S - one float rounding per monochromatic term in the reference
    (the float outputs of monortm_hip_rtm_scan_jac), plus one in the result: the host entry holds the sums in double and rounds once.
    Instantiations <float, double, 8, 4, false> and <float, double, 2, 4, false>."""
    b, path, mono = shared_mono(rt4, name, views, quantity)
    op = oc.operator(views, chmap, NWN)
    with handle(rt4, op) as h:
        rc, got = raw_obs(rt4, b, path, quantity, h, op)
    assert rc == 0, err(rt4)
    assert all(got[k].dtype == np.float32 for k in RTM_OUT)
    check_fields(got, mono, op, TOL4, RTM_OUT, what=f"real_kind 4 {name} {views}/{chmap} q={quantity}")


@pytest.mark.parametrize("name,views,chmap", [("B30", "C", "nested"), ("C12", "B", "comb")])
def test_device_entry_real_kind_4(rt4, name, views, chmap):
    """monortm_hip_rtm_obs_jac_dev on a real_kind 4 context: instantiations <float, float, 8, 4, false> and <float, float, 2, 4, false>,
    whose float outputs hold the running sums themselves.  An element of (view v, channel c) receives one contribution per tile of 4
    paths of v and block of 64 wavenumbers that holds a member of c, each added with one float rounding of a partial sum that is at
    most S: |got - ref| <= (1 + tiles(v) x blocks(c)) x 2^-24 S, the 1 for the roundings of the reference's monochromatic terms.
    C / nested: 6 tiles, channel 3 in both blocks; B / comb: views of 2, 0 and 2 tiles, channels 4 .. 9 in both blocks."""
    import torch

    b, path, mono = shared_mono(rt4, name, views, 1)
    op = oc.operator(views, chmap, NWN)
    tiles = -(-np.diff(op.view_start) // 4)
    blocks = np.array([len(set(np.nonzero(op.chan == c)[0] // 64)) for c in range(op.nchan)])
    ncontrib = tiles[:, None] * blocks[None, :]                      # [nview, nchan]
    assert ncontrib.max() >= 4
    dev = torch.device("cuda:0")
    up = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
    wn, nlay, irt = up(b.wn, torch.float64), up(b.nlay, torch.int32), up(b.irt, torch.int32)
    T, TZ, O, em, rf, ts, fd = (up(x) for x in (b.pad(b.T, 0.0), b.pad(b.TZ, 0.0), b.pad(b.O, 0.0), b.em, b.rf, b.ts, path))
    outs = {k: torch.full(s, FILL, dtype=torch.float32, device=dev) for k, s in out_shapes(b, op).items()}
    d = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with handle(rt4, op) as h:
        rc = rt4.lib.monortm_hip_rtm_obs_jac_dev(rt4.ctx, b.nprof, path.shape[1], b.nwn, d(wn), d(nlay), b.lm, d(irt), 1, d(T), d(TZ), d(O), d(fd),
                                                 d(ts), 0, d(em), d(rf), h, *[d(outs[k]) for k in RTM_OUT], s)
        assert rc == 0, err(rt4)
        assert rt4.lib.monortm_hip_check(rt4.ctx, s) == 0
        got = {k: v.cpu().numpy() for k, v in outs.items()}
    for k in RTM_OUT:
        ref, S = oc.reference(op, mono[k])
        n = ncontrib.reshape((1, op.nview) + (1,) * (ref.ndim - 3) + (op.nchan,))
        e = np.abs(got[k].astype(np.float64) - ref)
        bound = (1 + n) * 2.0 ** -24 * S
        print(f"real_kind 4 device entry {name}: {k} max |got - ref| / bound = {float(np.max(e / np.where(bound > 0, bound, 1.0))):.2f}")
        assert np.all(e <= bound), k


# ---- 2. the full entry against scan_jacobian, contracted ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_case(case):
    """Profiles (cloud, irt 1 / 3 / 2, 20 / 16 / 18 layers), 9 paths and the monochromatic result of MonoRTM.scan_jacobian with
    njac = 2, shared by the tests below (never modified)."""
    _, wn, rt = case
    prs = [synth.perturbed_profile(450 + i, wn, nlay=n, cloud=True, irt=irt) for i, (n, irt) in enumerate(zip([20, 16, 18], (1, 3, 2)))]
    l = np.arange(20) / 19.0
    path = oc.factors(9)[:, None] * (1.0 + 0.01 * l)[None, :]   # [9, 20]
    mono = dict(rt.scan_jacobian(prs, path, mols=(1, 3)))
    mono["y"] = mono["tb"]
    for v in mono.values():
        v.setflags(write=False)
    return prs, path, mono


FULL_K = ("y", "k_t", "k_tz", "k_w", "k_clw", "k_sfc")


def check_full(got, mono, op, tol, what, fields=FULL_K):
    g = {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in got.items()}
    m = dict(mono, k_w=np.moveaxis(mono["k_w"], 3, 2))   # [nprof, npath, njac, lm, nwn]: the contraction keeps the middle axes
    gg = dict(g, k_w=np.moveaxis(g["k_w"], 3, 2))        # [nprof, nview, njac, lm, nchan]
    return check_fields(gg, m, op, tol, fields, what=what)


@pytest.fixture(scope="module")
def full_obs(case, full_case):
    """The full entry on full_case with views A and the nested map: instantiation <double, double, 2, 4, true> (nlay_max = 20)."""
    _, wn, rt = case
    prs, path, _ = full_case
    op = oc.operator("A", "nested", len(wn))
    with handle(rt, op) as h:
        got = rt.obs_jacobian(prs, path, h, mols=(1, 3))
    for v in got.values():
        v.setflags(write=False)
    return op, got


def test_full_entry_equals_contracted_scan_jacobian(full_case, full_obs):
    """Y, K_T, K_TZ, K_W, K_CLW, K_SFC at 1e-12 S against MonoRTM.scan_jacobian (the `case` line list, njac = 2, cloud), element by
    element, O bit-equal; padded layers and levels 0.  K_T, K_W and K_CLW carry dq/dtau_k, which in the lowest layers of an opaque
    channel is the rounding residue of a cancellation (1e-14 of the column's largest entry) in rtm_scan_jac_kernel as much as here:
    there S is the size of that residue, and the bound holds because the two kernels round every monochromatic term alike (measured:
    every element bit-equal with the identity operator; 4.7e-7 S while this kernel let the compiler contract tau into the running
    optical depth)."""
    prs, path, mono = full_case
    op, got = full_obs
    assert got["k_w"].shape == (3, 3, 20, 2, 7)
    check_full(got, mono, op, TOL8, "full entry")
    np.testing.assert_array_equal(got["o"], mono["o"])
    for p, pr in enumerate(prs):
        n = pr.nlay
        assert np.all(got["k_t"][p, :, n:] == 0) and np.all(got["k_w"][p, :, n:] == 0) and np.all(got["k_clw"][p, :, n:] == 0)
        assert np.all(got["k_tz"][p, :, n + 1:] == 0)
    assert all(np.any(got[k] != 0) for k in FULL_K)


def test_full_entry_eight_layer_groups(case):
    """The same comparison for instantiation <double, double, 8, 4, true>: profiles of 30, 26 and 24 layers (from 24 layers on a profile
    works with eight layer groups here and in rtm_scan_jac_kernel), views B (a short tile, an empty view), the comb map."""
    _, wn, rt = case
    prs = [synth.perturbed_profile(460 + i, wn, nlay=n, cloud=True, irt=irt) for i, (n, irt) in enumerate(zip([30, 26, 24], (2, 1, 3)))]
    path = oc.factors(13)[:, None] * (1.0 + 0.01 * np.arange(30) / 29.0)[None, :]
    mono = dict(rt.scan_jacobian(prs, path, mols=(1, 3)))
    mono["y"] = mono["tb"]
    op = oc.operator("B", "comb", len(wn))
    with handle(rt, op) as h:
        got = rt.obs_jacobian(prs, path, h, mols=(1, 3))
    check_full(got, mono, op, TOL8, "full entry, G = 8")
    np.testing.assert_array_equal(got["o"], mono["o"])


def test_full_entry_mixed_layer_groups(case):
    """A batch of 30, 7 and 16 layers: nlay_max >= 24, so rtm_scan_jac_kernel walks EVERY profile with eight layer groups, while here a
    profile below 24 layers keeps its two (its bits must not depend on the batch it is in).  The group sums of the two short profiles
    are then formed in another order, and their monochromatic terms agree with the reference's to rounding, not to the bit.  Where a
    term is itself the rounding residue of a cancellation (dq/dtau in the lowest layers of an opaque channel: ~nlay x 2^-53 of the
    column's largest entry) no bound against the element's own S can hold between two summation orders.  For those two profiles the
    optical-depth terms are therefore held to 1e-12 of the LARGEST S over the layers of the (profile, view, channel) column - the
    normalisation (rel_err over the layer axis) and the bound by which tests/test_scan_jacobian.py compares two HIP formulations of the
    recurrence - and Y, K_TZ, K_SFC, which hold no such residue, to 1e-12 S element by element; the 30-layer profile to 1e-12 S in
    every field."""
    _, wn, rt = case
    prs = [synth.perturbed_profile(470 + i, wn, nlay=n, cloud=True, irt=irt) for i, (n, irt) in enumerate(zip([30, 7, 16], (1, 2, 1)))]
    path = oc.factors(9)[:, None] * (1.0 + 0.01 * np.arange(30) / 29.0)[None, :]
    mono = dict(rt.scan_jacobian(prs, path, mols=(1, 3)))
    mono["y"] = mono["tb"]
    op = oc.operator("A", "nested", len(wn))
    with handle(rt, op) as h:
        got = rt.obs_jacobian(prs, path, h, mols=(1, 3))
    np.testing.assert_array_equal(got["o"], mono["o"])
    cut = lambda d, p: {k: v[p:p + 1] for k, v in d.items()}  # noqa: E731
    check_full(cut(got, 0), cut(mono, 0), op, TOL8, "mixed batch, 30 layers")
    for p in (1, 2):
        check_full(cut(got, p), cut(mono, p), op, TOL8, f"mixed batch, profile {p}", fields=("y", "k_tz", "k_sfc"))
        for k in ("k_t", "k_w", "k_clw"):
            ref, S = oc.reference(op, mono[k][p:p + 1])
            scale = S.max(axis=2, keepdims=True)                     # over the layer axis of [1, nview, nlay_max, (njac,) nchan]
            e = float(np.max(np.abs(got[k][p:p + 1] - ref) / np.where(scale > 0, scale, 1.0)))
            print(f"mixed batch, profile {p}: {k} max |got - ref| / max_layers S = {e:.2e}")
            assert e <= TOL8, (p, k, e)


# What the element-wise bound on K_T, K_W and K_CLW rests on: every monochromatic term being rounded as rtm_scan_jac_kernel rounds it.
# The two kernels are compiled separately from the same expressions, and which products the compiler contracts into which sums is its
# choice at every site that is not spelled out (here only add_rounded is; __dmul_rn is a plain multiply to it).  A compiler that
# chooses differently in one of the two kernels makes test_full_entry_equals_contracted_scan_jacobian and
# test_full_entry_eight_layer_groups fail in the residue elements with neither kernel wrong: compare bit for bit with the identity
# operator (LABNOTES section 17) to find the site, and pin it.


# ---- 3. the identity operator --------------------------------------------------------------------------------------------------------
def test_identity_operator_gives_the_monochromatic_fields(rt):
    """nview = npath = 5, nchan = nwn = 70 (more channels than lanes: owner lanes serve two), unit weights: every field equals the
    monochromatic one at 1e-12 of its magnitude (S = |term|)."""
    b = sj.Batch(BATCHES["B30"], 21)
    path = b.path(oc.factors(5))
    op = oc.identity(5, NWN)
    for quantity in (1, 0):
        mono = mono_ref(rt, b, path, quantity)
        with handle(rt, op) as h:
            rc, got = raw_obs(rt, b, path, quantity, h, op)
        assert rc == 0, err(rt)
        check_fields(got, mono, op, TOL8, RTM_OUT, what=f"identity q={quantity}")
        for k in RTM_OUT:
            np.testing.assert_allclose(got[k], mono[k], rtol=1e-12, atol=0, err_msg=k)


# ---- 4. end to end against the oracle --------------------------------------------------------------------------------------------------
def test_full_entry_matches_oracle_end_to_end(case):
    """Y of the full entry against the oracle's TB along every path - Oracle.run on the profile with amounts scaled by the path's
    factors, as tests/test_scan_jacobian.py::test_full_entry_matches_oracle_end_to_end obtains them - contracted in float64; 1e-6
    relative, the project's parity bound (uniform normalised weights: Y is a mean of brightness temperatures).  K follows from the
    tests above and the pin of scan_jacobian."""
    from oracle.pyoracle import Oracle

    t3, wn, rt = case
    pr = synth.perturbed_profile(410, wn, nlay=12, cloud=True, irt=1)
    path = api.plane_parallel_path([0.0, 20.0, 30.0, 40.0, 50.0, 55.0, 60.0, 65.0, 70.0], 12)
    ch, _, nchan = oc.nested_map(len(wn))
    op, perm = api.ObsOperator.from_sets(views=[[8, 0, 3, 5], [1], [2, 4, 6, 7]], channels=[list(np.nonzero(ch == c)[0]) for c in range(nchan)],
                                         npath=9, nwn=len(wn))
    with handle(rt, op) as h:
        got = rt.obs_jacobian([pr], path[perm], h, mols=(1,))
    orc = Oracle(t3, wn[0], wn[-1])
    tb = np.array([orc.run(sj.scaled(pr, path[j])).tb for j in perm])[None]      # [1, npath, nwn], the operator's path order
    orc.close()
    ref, S = oc.reference(op, tb)
    live = S > 0
    e = float(np.max(np.abs(got["y"] - ref)[live] / np.abs(ref)[live]))
    print(f"Y against the oracle: {e:.2e}")
    assert e <= 1e-6 and np.all(got["y"][~live] == 0) and np.sum(live) == 3 * 6


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R30", "C12"])
def test_bit_identical_twice_and_alone(rt, name):
    """Two calls give the same bits; profile i of the ragged batch gives the bits of the same profile alone (nprof = 1, its own nlay as
    nlay_max - for R30's profiles of 1, 2 and 7 layers that is the G = 2 instantiation against the batch's G = 8)."""
    b, path, _ = shared_mono(rt, name, "B", 1)
    op = oc.operator("B", "nested", NWN)
    with handle(rt, op) as h:
        rc, one = raw_obs(rt, b, path, 1, h, op)
        assert rc == 0, err(rt)
        rc, two = raw_obs(rt, b, path, 1, h, op)
        assert rc == 0
        for k in RTM_OUT:
            np.testing.assert_array_equal(one[k], two[k])
        for i in range(b.nprof):
            rc, alone = raw_obs(rt, b, path, 1, h, op, only=i)
            assert rc == 0, err(rt)
            n = int(b.nlay[i])
            np.testing.assert_array_equal(alone["y"][0], one["y"][i])
            np.testing.assert_array_equal(alone["k_sfc"][0], one["k_sfc"][i])
            np.testing.assert_array_equal(alone["k_t"][0], one["k_t"][i, :, :n])
            np.testing.assert_array_equal(alone["k_tz"][0], one["k_tz"][i, :, :n + 1])


def test_full_entry_twice(case, full_case):
    _, wn, rt = case
    prs, path, _ = full_case
    op = oc.operator("A", "comb", len(wn))
    with handle(rt, op) as h:
        one = rt.obs_jacobian(prs, path, h, mols=(1, 3))
        two = rt.obs_jacobian(prs, path, h, mols=(1, 3))
    for k in FULL_OUT:
        np.testing.assert_array_equal(one[k], two[k])


# ---- 6. plumbing -------------------------------------------------------------------------------------------------------------------------
def test_multi_device_context(rt, monkeypatch):
    """A two-shard context (both on device 0) gives the bits of one device; a bad factor in the LAST shard is refused before any
    launch: every output keeps the caller's fill.  The context still works afterwards."""
    b, path, _ = shared_mono(rt, "B30", "A", 1)
    op = oc.operator("A", "nested", NWN)
    monkeypatch.setenv("MONORTM_DEVICES", "0,0")
    m = api.MonoRTM("", 0.0, 0.0, ngpu=0)
    assert m.lib.monortm_hip_device_count(m.ctx) == 2
    with handle(rt, op) as h1, handle(m, op) as h2:
        rc, one = raw_obs(rt, b, path, 1, h1, op)
        assert rc == 0
        rc, two = raw_obs(m, b, path, 1, h2, op)
        assert rc == 0, err(m)
        for k in RTM_OUT:
            np.testing.assert_array_equal(two[k], one[k])
        f = path.copy()
        f[2, 3, 29] = -1.0                              # the last active layer of the last profile
        rc, got = raw_obs(m, b, f, 1, h2, op)
        assert rc == EARG and b"profile 2 path 3 layer 29" in err(m)
        assert all(np.all(got[k] == FILL) for k in RTM_OUT)
        rc, again = raw_obs(m, b, path, 1, h2, op)
        assert rc == 0, err(m)
        for k in RTM_OUT:
            np.testing.assert_array_equal(again[k], one[k])
    m.close()


def same_obs(got, ref, tol, other=None):
    """Two results of the full entry: o, y at rtol `tol`, the K fields at `tol` by rel_err over the layer / level axis (k_sfc: its three
    components; k_w with its floor), as same_full of tests/test_scan_jacobian.py; `other`: fields with a bound of their own."""
    for k in FULL_OUT:
        g = got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy()
        t = (other or {}).get(k, tol)
        if k in ("o", "y"):
            np.testing.assert_allclose(g, ref[k], rtol=t, atol=0, err_msg=k)
        else:
            assert sj.rel_err(g, ref[k], axis=2, floor=sj.w_floor(ref[k]) if k == "k_w" else 0.0) <= t, k


def test_full_entry_multi_device(case, full_case, full_obs, monkeypatch):
    """Two shards against one device, the same entry.  The shards run MODM on batches of other sizes: O agrees to rounding, which the
    differences in k_t and k_w divide by the step - the bounds of tests/test_scan_jacobian.py::test_full_entry_multi_device, by column:
    1e-12, k_t and k_w 1e-9."""
    t3, wn, _ = case
    prs, path, _ = full_case
    op, one = full_obs
    monkeypatch.setenv("MONORTM_DEVICES", "0,0")
    m = api.MonoRTM(t3, wn[0], wn[-1], ngpu=0)
    with handle(m, op) as h:
        two = m.obs_jacobian(prs, path, h, mols=(1, 3))
        f = np.broadcast_to(path[None], (3,) + path.shape).copy()
        f[2, 8, 17] = -0.5                               # the last active layer of the last profile, in the last shard
        with pytest.raises(api.MonoRTMError) as e:
            m.obs_jacobian(prs, f, h, mols=(1, 3))
        assert e.value.code == EARG and "profile 2 path 8 layer 17" in str(e.value)
    m.close()
    same_obs(two, one, 1e-12, {"k_t": 1e-9, "k_w": 1e-9})


def test_device_batch_obs_jacobian_and_graph_replay(case, full_case, full_obs):
    """DeviceBatch.obs_jacobian against MonoRTM.obs_jacobian (the same kernels on the same inputs: the bounds of same_full in
    tests/test_scan_jacobian.py::test_device_batch_scan_jacobian_and_graph_replay); then one capture, new factors in the device tensor,
    a replay into the same (overwritten) tensors, against the host entry on the new factors."""
    import torch

    _, wn, rt = case
    prs, path, _ = full_case
    op, ref = full_obs
    db = api.DeviceBatch(rt, prs)
    fdev = torch.as_tensor(path).to(db.dev)
    with handle(rt, op) as h:
        got = db.obs_jacobian(fdev, h, mols=(1, 3))
        torch.cuda.synchronize()
        db.check()
        same_obs(got, ref, 1e-12)
        assert db.obs_jacobian(fdev, h, mols=(1, 3)) is got    # overwritten in place
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                db.obs_jacobian(fdev, h, mols=(1, 3))
        torch.cuda.current_stream().wait_stream(s)
        path2 = path[::-1] * 1.25
        fdev.copy_(torch.as_tensor(np.ascontiguousarray(path2)))
        for v in got.values():
            v.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        db.check()
        ref2 = rt.obs_jacobian(prs, path2, h, mols=(1, 3))
    assert not np.array_equal(ref2["y"], ref["y"])
    same_obs(got, ref2, 1e-12)
    # the operator is destroyed: the next call drops its tensors from the batch's cache (handles are never given out again)
    assert [k[0] for k in db._obs_jac] == [h]
    with handle(rt, op) as h2:
        again = db.obs_jacobian(fdev, h2, mols=(1, 3))
        torch.cuda.synchronize()
        assert h2 != h and [k[0] for k in db._obs_jac] == [h2] and again is not got
        same_obs(again, ref2, 1e-12)


def test_obs_jacobian_between_modm_and_rtm_changes_nothing(case, full_case):
    _, wn, rt = case
    prs, path, _ = full_case
    op = oc.operator("A", "comb", len(wn))
    O = rt.modm(prs)[0]
    tb0 = rt.rtm(prs, O)[4]
    sc0 = rt.rtm_scan(prs, O, path)["tb"]
    O = rt.modm(prs)[0]
    with handle(rt, op) as h:
        rt.obs_jacobian(prs, path, h, mols=(1,))
        rt.rtm_obs_jacobian(prs, O, path, h)
    tb1 = rt.rtm(prs, O)[4]
    sc1 = rt.rtm_scan(prs, O, path)["tb"]
    assert np.array_equal(tb0, tb1) and np.array_equal(sc0, sc1)


def test_surface_arrays_per_path(rt):
    b = sj.Batch(BATCHES["B30"], 23, irt=(1,))
    op = oc.operator("A", "nested", NWN)
    path = b.path(oc.factors(9))
    rng = np.random.default_rng(5)
    em = rng.uniform(0.5, 1.0, (b.nprof, 9, b.nwn))
    rf = 1.0 - em
    mono = mono_ref(rt, b, path, 1, em=em, rf=rf)
    with handle(rt, op) as h:
        rc, got = raw_obs(rt, b, path, 1, h, op, em=em, rf=rf)
        assert rc == 0, err(rt)
        check_fields(got, mono, op, TOL8, RTM_OUT, what="surface per path")
        rc, shared = raw_obs(rt, b, path, 1, h, op)
        assert rc == 0
        assert not np.array_equal(got["k_sfc"], shared["k_sfc"])
        rep = lambda x: np.ascontiguousarray(np.broadcast_to(x[:, None, :], (b.nprof, 9, b.nwn)))  # noqa: E731
        rc, replicated = raw_obs(rt, b, path, 1, h, op, em=rep(b.em), rf=rep(b.rf))
        assert rc == 0
    for k in RTM_OUT:
        np.testing.assert_array_equal(replicated[k], shared[k])


def test_zero_factor_layer(rt):
    """A layer that does not absorb along some paths of a view: everything still equals the contracted per-path reference."""
    b = sj.Batch(BATCHES["C12"], 22)
    op = oc.operator("A", "comb", NWN)
    path = b.path(oc.factors(9))
    path[:, 1, 2] = 0.0
    path[1, 4, 11] = 0.0
    path[:, 5:, 0] = 0.0
    mono = mono_ref(rt, b, path, 1)
    with handle(rt, op) as h:
        rc, got = raw_obs(rt, b, path, 1, h, op)
    assert rc == 0, err(rt)
    check_fields(got, mono, op, TOL8, RTM_OUT, what="zero factor")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def raw_create(r, npath, nwn, nview, nchan, vs, wp, ch, wc):
    h = C.c_int(-5)
    a = [None if x is None else np.ascontiguousarray(x, dt) for x, dt in ((vs, np.int32), (wp, np.float64), (ch, np.int32), (wc, np.float64))]
    rc = r.lib.monortm_hip_obs_create(r.ctx, npath, nwn, nview, nchan, *[_p(x) for x in a], C.byref(h))
    return rc, h.value


def test_refusals_leave_the_context_working(rt, rt4, case):
    b, path, _ = shared_mono(rt, "C12", "A", 1)
    op = oc.operator("A", "nested", NWN)
    good = dict(npath=9, nwn=NWN, nview=3, nchan=7, vs=op.view_start, wp=op.wpath, ch=op.chan, wc=op.wchan)
    with handle(rt, op) as h:
        rc, want = raw_obs(rt, b, path, 1, h, op)
        assert rc == 0

        def edit(name, idx, v):
            x = np.array(good[name], np.float64 if name in ("wp", "wc") else np.int32)
            x[idx] = v
            return {name: x}

        for bad in (edit("vs", 1, 6), edit("vs", 0, 1), edit("vs", 3, 8), edit("ch", 5, 7), edit("ch", 5, -2), edit("wp", 2, np.nan),
                    edit("wc", 69, np.nan), edit("wc", 0, np.inf), dict(npath=0), dict(npath=1 << 20), dict(nwn=0), dict(nview=0), dict(nchan=0),
                    dict(vs=None), dict(wp=None), dict(ch=None), dict(wc=None)):
            rc, hb = raw_create(rt, **dict(good, **bad))
            assert rc == EARG and hb == 0 and err(rt), bad          # ([0, 6, 5, 9] is unsorted; 7 >= nchan; NaN / inf weights)
        assert rt.lib.monortm_hip_obs_create(rt.ctx, 9, NWN, 3, 7, _p(op.view_start), _p(op.wpath), _p(op.chan), _p(op.wchan), None) == EARG
        # a call whose npath or nwn is not the handle's
        op13 = oc.operator("B", "nested", NWN)
        with handle(rt, op13) as h13:
            rc, got = raw_obs(rt, b, path, 1, h13, op)
            assert rc == EARG and b"npath = 13" in err(rt) and all(np.all(got[k] == FILL) for k in RTM_OUT)
        op60 = oc.operator("A", "nested", 60)
        with handle(rt, op60) as h60:
            assert raw_obs(rt, b, path, 1, h60, op)[0] == EARG and b"nwn = 60" in err(rt)
        # destroyed, never created, foreign
        assert raw_obs(rt, b, path, 1, h13, op)[0] == EARG and b"handle" in err(rt)
        assert rt.lib.monortm_hip_obs_destroy(rt.ctx, h13) == EARG
        for hb in (0, -1, h + 16, 1 << 30):
            assert raw_obs(rt, b, path, 1, hb, op)[0] == EARG, hb
        with handle(rt4, op) as h4:
            assert h4 != h and raw_obs(rt, b, path, 1, h4, op)[0] == EARG
        # the refusals of monortm_hip_rtm_scan_jac
        for over in (dict(npath=0), dict(nprof=0), dict(nwn=0), dict(nlay_max=0), dict(nlay_max=604), dict(sfc_per_path=2)):
            assert raw_obs(rt, b, path, 1, h, op, **over)[0] == EARG, over
        for q in (2, -1):
            assert raw_obs(rt, b, path, q, h, op)[0] == EARG, q
        for name in ("wn", "nlay", "irt", "T", "TZ", "O", "path", "ts", "em", "rf", "y", "k_t", "k_tz", "k_sfc"):
            assert raw_obs(rt, b, path, 1, h, op, drop=(name,))[0] == EARG, name
        for v in (-1e-3, np.nan, np.inf):
            f = path.copy()
            f[0, 2, 2] = v                               # an active layer of profile 0 (3 layers)
            rc, got = raw_obs(rt, b, f, 1, h, op)
            assert rc == EARG, v
            assert all(np.all(got[k] == FILL) for k in RTM_OUT)
        f = path.copy()
        f[0, 1, 3:] = -1.0                               # padded layers of profile 0: ignored
        rc, got = raw_obs(rt, b, f, 1, h, op)
        assert rc == 0, err(rt)
        for k in RTM_OUT:
            np.testing.assert_array_equal(got[k], want[k])
    # a 17th operator is refused, and all are released by close()
    r = api.MonoRTM("", 0.0, 0.0)
    hs = [r.obs_create(op) for _ in range(16)]
    assert len(set(hs)) == 16
    with pytest.raises(api.MonoRTMError) as e:
        r.obs_create(op)
    assert e.value.code == EARG
    r.obs_destroy(hs[3])
    assert r.obs_create(op) not in hs                    # a handle is never given out twice
    r.close()
    # the full entry: a float context, and the refusals of monortm_hip_scan_jacobian
    _, wn, rc8 = case
    prs = [synth.perturbed_profile(490, wn, nlay=16)]
    opw = oc.operator("A", "nested", len(wn))
    one = np.ones((9, 16))
    with handle(rt4, opw) as h4:
        with pytest.raises(api.MonoRTMError) as e:
            rt4.obs_jacobian(prs, one, h4)
        assert api.ERRORS[e.value.code] == "EUNSUPPORTED"
    with handle(rc8, opw) as h8:
        for kw in (dict(mols=(0,)), dict(mols=(8,)), dict(mols=(1, 1)), dict(quantity=2)):
            with pytest.raises(api.MonoRTMError) as e:
                rc8.obs_jacobian(prs, one, h8, **kw)
            assert e.value.code == EARG, kw
        f = one.copy()
        f[8, 15] = np.nan
        with pytest.raises(api.MonoRTMError) as e:
            rc8.obs_jacobian(prs, f, h8)
        assert e.value.code == EARG and "path 8 layer 15" in str(e.value)
        cold = copy.deepcopy(prs[0])
        cold.t = cold.t.copy()
        cold.t[3] = 70.0 + 0.5 * api.JAC_DT
        with pytest.raises(api.MonoRTMError) as e:
            rc8.obs_jacobian([cold], one, h8)
        assert api.ERRORS[e.value.code] == "ETEMP"
        with pytest.raises(api.MonoRTMError):
            rc8.obs_jacobian(prs, np.ones((5, 16)), h8)      # npath is not the handle's
        res = rc8.obs_jacobian(prs, one, h8)
        assert all(np.all(np.isfinite(v)) for v in res.values())


def test_device_entry_flags_bad_factors(rt):
    import torch

    b, path, _ = shared_mono(rt, "C12", "A", 1)
    op = oc.operator("A", "nested", NWN)
    dev = torch.device("cuda:0")
    up = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
    wn, nlay, irt = up(b.wn), up(b.nlay, torch.int32), up(b.irt, torch.int32)
    T, TZ, O, em, rf, ts = up(b.pad(b.T, 0.0)), up(b.pad(b.TZ, 0.0)), up(b.pad(b.O, 0.0)), up(b.em), up(b.rf), up(b.ts)
    outs = {k: torch.full(s, FILL, dtype=torch.float64, device=dev) for k, s in out_shapes(b, op).items()}
    d = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with handle(rt, op) as h:
        rc, want = raw_obs(rt, b, path, 1, h, op)
        assert rc == 0

        def call(f, npath=9, hh=h):
            fd = up(f)
            rc = rt.lib.monortm_hip_rtm_obs_jac_dev(rt.ctx, b.nprof, npath, b.nwn, d(wn), d(nlay), b.lm, d(irt), 1, d(T), d(TZ), d(O), d(fd),
                                                    d(ts), 0, d(em), d(rf), hh, *[d(outs[k]) for k in RTM_OUT], s)
            return rc, rt.lib.monortm_hip_check(rt.ctx, s)

        assert call(path) == (0, 0)
        for k in RTM_OUT:
            np.testing.assert_array_equal(outs[k].cpu().numpy(), want[k])     # the device entry's bits are the host entry's
        for v in (-2.0, np.nan, np.inf):
            f = path.copy()
            f[1, 8, 11] = v                              # the last active layer of profile 1, last path of the last view
            assert call(f) == (0, EARG), v               # the launch succeeds, the flag tells
            assert rt.lib.monortm_hip_check(rt.ctx, s) == 0   # ... once
        f = path.copy()
        f[0, 0, 6] = -5.0                                # a padded layer
        assert call(f) == (0, 0)
        for k in RTM_OUT:
            np.testing.assert_array_equal(outs[k].cpu().numpy(), want[k])
        assert call(path, npath=8)[0] == EARG
        assert call(path, hh=h + 16)[0] == EARG
        assert call(path) == (0, 0)
