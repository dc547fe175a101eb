"""rtm_jac_kernel, rtm_scan_jac_kernel, rtm_obs_jac_kernel and rtm_obs_kernel against the extended-precision truth of tests/rtm_truth.py
(truth() and its closed-form adjoint truth_adjoint()), on the inputs of tests/test_rtm_extremes.py: the nine column classes, 70
wavenumbers from 0.5 to 57000 cm-1, batches A64 / B30 / C12 (G = 8 with eight layers a group and empty groups, G = 8, G = 2; in the obs
kernels A64's profiles of 1, 2, 7 and 23 layers work with two of the eight groups), path factors down to 1e-3, both real kinds.
Contexts without TAPE3: RTM needs no line table.

The reference of path j is the truth at tau = (double)O x (double)f_j rounded once, as the kernels form it; k_o is f_j times the
truth's dq/dtau and k_path is O times it.  real_kind 4 gets Batch.rounded(float32) and the truth is taken on those floats.  Every
call is made twice, the padding beyond nlay[p] once zero and once NaN: the results must be identical, and padded outputs are exactly
0 in arrays pre-filled with -7.

Bounds (none is fitted to the kernels; E, k_error and the classes are defined in tests/rtm_truth.py; E_orc = E(oracle, truth) is taken
per path on the same inputs in the same test):
  1. RAD, TB and every term of a contracted Y: assertion 1 of tests/test_rtm_extremes.py, E(kernel, truth) <= 4 E_orc + 64 eps
     (real_kind 4: + 2^-24, one rounding of the output).
  2. The monochromatic K_O, K_PATH, K_T, K_TZ: k_error <= 1e-6 (real_kind 4: + 2^-24), the bound of
     test_rtm_extremes.py::test_jacobian_against_truth_differences; K_SFC 1e-6 per element, exactly 0 for irt 2 and 3.  K_PATH has
     a test of its own: it weighs dq/dtau with the layer's O, and found what K_O's scale hides (test_rtm_scan_jac_k_path).
  3. A contracted K field: |got - ref| <= contract(|W|, b) + 64 eps S (real_kind 4: + 2^-24 S), ref and S = obs_cases.reference of the
     truth's monochromatic fields, b = bound 2 of each term: 1e-6 x the k_error scale of its (profile, path, wavenumber) column (K_SFC:
     1e-6 |term|).  A contracted Y likewise with b = (4 E_orc + 64 eps) |q|; where S = 0 an exact 0.
  4. The band brightness temperature: the relative bound of its contracted radiance, unchanged - d ln TB / d ln RAD =
     x / ((1 + x) ln(1 + x)) <= 1 with x = c3 / RAD - against RADCN2 vc / log1p(c3(vc) / ybar) of the truth's contracted radiance.
  5. The _dev entries of a real_kind 4 context (<float, float>: the float output holds the running sum): bound 3 plus
     (1 + tiles x blocks) 2^-24 S, the term of tests/test_obs_jacobian.py::test_device_entry_real_kind_4.
Which K figures are asserted.  Bound 2 is asserted where the REFERENCE itself keeps its digits: on the classes outside CANCELLING,
and there on the (profile, path) pairs whose E_orc of RUP and RDN is <= 1e-7 - the condition under which tests/test_rtm_extremes.py
holds a kernel to the oracle at 1e-6.  The factor 1e-3 turns a `thin` column (1e-8 .. 1e-4 a layer) into a `thinnest` one, and so
the thinnest columns of `mixed`: 1 - exp(-tau) of the reference's own formula keeps 16 + log10(tau) digits, whatever the kernel
does.  Those pairs, `thinnest` and `degenerate` are printed and recorded only.  Every other factor is asserted on every profile of
every class outside CANCELLING (checked from the oracle and the truth alone).  A contracted K element is asserted where every path of
its view is.
The float floor (a condition, not a tolerance): a float cannot hold a column whose k_error scale is below SGL_FLOOR = 1e-30.  In
real_kind 4 such a column must have |k| <= 2e-30 and is left out of the maximum; at most a quarter of a case's columns may be left
out this way, asserted from the truth alone.  A contracted element with S below the floor of its format (1e-30; in real_kind 8 the
smallest normal double, as in E) must likewise be <= 2 x that floor and is left out.

Run with -s for every figure; MONORTM_TRUTH_RECORD names a file that collects the worst of each."""
import ctypes as C
import types

import numpy as np
import pytest

import common  # noqa: F401  (puts the repository root on sys.path)
import obs_cases as oc
import rtm_truth as tr
from monortm_amd import api
from test_rtm_extremes import _p, raw_jac, same

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -52
F24 = 2.0 ** -24
FILL = -7.0
FACTORS9 = [1.0, 0.7, 5.76, 19.1, 1e-3, 1.3, 2.0, 11.0, 0.05]   # cycled over the paths; the first five are two tiles (4 + 1)
NAMES = ("A64", "B30", "C12")
OPS = (("A", "nested"), ("B", "comb"))       # mixed-sign weights, an empty view, an empty channel, channels in both wavenumber blocks
DEV_CLASSES = ("lognormal", "opaque_middle")
QUANT = {"rad": 0, "tb": 1}
SCAN_OUT = api.SCAN_JAC_RTM_FIELDS           # rad, tb, k_o, k_path, k_t, k_tz, k_sfc
OBS_OUT = api.OBS_JAC_RTM_FIELDS             # y, k_t, k_tz, k_sfc


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    yield True
    tr.dump_record()


@pytest.fixture(scope="module")
def ctx(gpu):
    c = {8: api.MonoRTM("", 0.0, 0.0), 4: api.MonoRTM("", 0.0, 0.0, real_kind=4)}
    yield c
    for r in c.values():
        r.close()


def err(r):
    return r.lib.monortm_hip_last_error(r.ctx)


# ---- the calls -----------------------------------------------------------------------------------------------------------------------
def raw_scan_jac(r, b, a, path, quantity):
    """monortm_hip_rtm_scan_jac on the arrays a (Batch.rounded) and path [nprof, npath, lm] -> dict of outputs pre-filled with FILL."""
    n, lm, nw, npath = b.nprof, b.lm, b.nwn, path.shape[1]
    sh = dict(rad=(n, npath, nw), tb=(n, npath, nw), k_o=(n, npath, lm, nw), k_path=(n, npath, lm, nw), k_t=(n, npath, lm, nw),
              k_tz=(n, npath, lm + 1, nw), k_sfc=(n, npath, 3, nw))
    out = {k: np.full(s, FILL, r.dtype) for k, s in sh.items()}
    rc = r.lib.monortm_hip_rtm_scan_jac(r.ctx, n, npath, nw, _p(b.wn), _p(b.nlay), lm, _p(b.irt), QUANT[quantity], _p(a["T"]), _p(a["TZ"]),
                                        _p(a["O"]), _p(path), _p(a["ts"]), 0, _p(a["em"]), _p(a["rf"]), *[_p(out[k]) for k in SCAN_OUT])
    assert rc == 0, err(r)
    return out


def obs_shapes(b, op):
    n, lm, nv, nc = b.nprof, b.lm, op.nview, op.nchan
    return dict(y=(n, nv, nc), k_t=(n, nv, lm, nc), k_tz=(n, nv, lm + 1, nc), k_sfc=(n, nv, 3, nc))


def raw_obs_jac(r, b, a, path, quantity, h, op):
    out = {k: np.full(s, FILL, r.dtype) for k, s in obs_shapes(b, op).items()}
    rc = r.lib.monortm_hip_rtm_obs_jac(r.ctx, b.nprof, path.shape[1], b.nwn, _p(b.wn), _p(b.nlay), b.lm, _p(b.irt), QUANT[quantity], _p(a["T"]),
                                       _p(a["TZ"]), _p(a["O"]), _p(path), _p(a["ts"]), 0, _p(a["em"]), _p(a["rf"]), h, *[_p(out[k]) for k in OBS_OUT])
    assert rc == 0, err(r)
    return out


def raw_obs(r, b, a, path, quantity, h, op, vcen=None):
    """monortm_hip_rtm_obs, quantity 0 (RAD), 1 (TB) or 2 (band TB at vcen) -> Y pre-filled with FILL."""
    y = np.full((b.nprof, op.nview, op.nchan), FILL, r.dtype)
    vc = None if vcen is None else np.ascontiguousarray(vcen, np.float64)
    v = None if vc is None else _p(vc)
    rc = r.lib.monortm_hip_rtm_obs(r.ctx, b.nprof, path.shape[1], b.nwn, _p(b.wn), _p(b.nlay), b.lm, _p(b.irt), quantity, _p(a["T"]), _p(a["TZ"]),
                                   _p(a["O"]), _p(path), _p(a["ts"]), 0, _p(a["em"]), _p(a["rf"]), h, v, _p(y))
    assert rc == 0, err(r)
    return y


def dev_calls(r, b, a, path, h, op):
    """monortm_hip_rtm_obs_jac_dev and monortm_hip_rtm_obs_dev, quantity TB, on device tensors of the context's REAL kind -> (the
    adjoint's outputs, the forward entry's Y) as numpy arrays."""
    import torch

    dev = torch.device("cuda:0")
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    d = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    t = {k: up(v) for k, v in dict(a, wn=b.wn, nlay=b.nlay, irt=b.irt, path=path).items()}
    real = t["O"].dtype
    outs = {k: torch.full(s, FILL, dtype=real, device=dev) for k, s in obs_shapes(b, op).items()}
    y = torch.full((b.nprof, op.nview, op.nchan), FILL, dtype=real, device=dev)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = (r.ctx, b.nprof, path.shape[1], b.nwn, d(t["wn"]), d(t["nlay"]), b.lm, d(t["irt"]), 1, d(t["T"]), d(t["TZ"]), d(t["O"]), d(t["path"]),
            d(t["ts"]), 0, d(t["em"]), d(t["rf"]), h)
    assert r.lib.monortm_hip_rtm_obs_jac_dev(*head, *[d(outs[k]) for k in OBS_OUT], s) == 0, err(r)
    assert r.lib.monortm_hip_rtm_obs_dev(*head, None, d(y), s) == 0, err(r)
    assert r.lib.monortm_hip_check(r.ctx, s) == 0
    return {k: v.cpu().numpy() for k, v in outs.items()}, y.cpu().numpy()


# ---- the references ------------------------------------------------------------------------------------------------------------------
class Case:
    """One (batch, class, real kind): the arrays as the context receives them and, per path factor, the truth, its adjoint and the
    oracle at tau = (double)O x (double)f rounded once.  Computed once per case, shared by its tests, never modified."""

    def __init__(self, r, name, cls, kind):
        self.r, self.name, self.cls, self.kind = r, name, cls, kind
        self.b = b = tr.make_batch(name, cls)
        self.a0, self.an = b.rounded(r.dtype, 0.0), b.rounded(r.dtype, np.nan)
        self.f = np.asarray(FACTORS9, r.dtype)
        self._ref = {}

    def paths(self, npath, fill=0.0):
        """[nprof, npath, lm] in the context's REAL kind: the same factor for every layer of a path, `fill` beyond nlay[p]."""
        f = self.f[np.arange(npath) % len(self.f)]
        path = np.ascontiguousarray(np.broadcast_to(f[None, :, None], (self.b.nprof, npath, self.b.lm)))
        path[np.broadcast_to(~self.b.lay[:, None, :], path.shape)] = fill
        return path

    def ref(self, i):
        """Factor i of FACTORS9 -> dict(t = truth, o = the oracle, adj = truth_adjoint, gate [nprof]: E_orc of RUP and RDN <= 1e-7)."""
        if i not in self._ref:
            b = self.b
            Oj = self.a0["O"].astype(np.float64) * np.float64(self.f[i])
            args = b.args(self.a0, O=Oj)
            t, (o, _), adj = tr.truth(*args), tr.oracle(*args), tr.truth_adjoint(*args)
            gate = np.array([max(tr.E(o[k][p:p + 1], t[k][p:p + 1], o[k][p:p + 1]) for k in ("rup", "rdn")) <= 1e-7 for p in range(b.nprof)])
            fl, O = LD(self.f[i]), np.asarray(self.a0["O"], LD)
            for q in adj:
                dqdtau = adj[q]["k_o"]
                adj[q]["k_o"], adj[q]["k_path"] = fl * dqdtau, np.where(b.lay[:, :, None], O * dqdtau, LD(0))
            self._ref[i] = dict(t=t, o=o, adj=adj, gate=gate)
        return self._ref[i]

    def mono(self, npath, quantity, fields):
        """The references of `npath` paths stacked on axis 1 -> (dict of the truth's `fields` and q, the oracle's q, gate [nprof, npath],
        E_orc of q per path)."""
        refs = [self.ref(j % len(self.f)) for j in range(npath)]
        m = {k: np.stack([x["adj"][quantity][k] for x in refs], axis=1) for k in fields}
        m["q"] = np.stack([x["t"][quantity] for x in refs], axis=1)
        oq = np.stack([x["o"][quantity] for x in refs], axis=1)
        gate = np.stack([x["gate"] for x in refs], axis=1)
        if self.cls in tr.CANCELLING:
            gate = np.zeros_like(gate)
        e_orc = np.array([tr.E(oq[:, j], m["q"][:, j], oq[:, j]) for j in range(npath)])
        return m, oq, gate, e_orc


@pytest.fixture(scope="module", params=[(n, c, k) for n in NAMES for c in tr.CLASSES for k in (8, 4)], ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def case(request, ctx):
    name, cls, kind = request.param
    return Case(ctx[kind], name, cls, kind)


# ---- the measures --------------------------------------------------------------------------------------------------------------------
def k_columns(k, ref, q, axis, kind):
    """Per (profile[, path], wavenumber) column: (max over the layer axis of |k - ref| / the k_error scale max(max |ref|, 1e-6 |q|), the
    scale, the columns a float cannot hold).  A column below the float floor must have |k| <= 2e-30: inf otherwise."""
    k, ref, q = np.asarray(k, LD), np.asarray(ref, LD), np.asarray(q, LD)
    with np.errstate(all="ignore"):
        scale = np.maximum(np.abs(ref).max(axis=axis), LD(1e-6) * np.abs(q))
        e = np.abs(k - ref).max(axis=axis) / scale
    e = np.where(scale > 0, e, np.where(np.abs(k).max(axis=axis) == 0, LD(0), LD(np.inf)))
    e = np.where(np.isfinite(k).all(axis=axis), e, LD(np.inf))
    low = np.zeros(scale.shape, bool)
    if kind == 4:
        low = (scale > 0) & (scale < LD(tr.SGL_FLOOR))
        e = np.where(low, np.where(np.abs(k).max(axis=axis) <= 2 * LD(tr.SGL_FLOOR), LD(0), LD(np.inf)), e)
    return e, scale, low


def check_mono(what, case, quantity, got, m, oq, gate, e_orc, fields):
    """Bounds 1 and 2 of the module docstring on monochromatic outputs [nprof, npath, ...] (monortm_hip_rtm_jac: npath = 1)."""
    b, kind, cls = case.b, case.kind, case.cls
    npath = got["rad"].shape[1]
    fails = []
    rnd = 64 * EPS if kind == 8 else F24
    for j in range(npath):   # 1. the quantity itself, per path
        e = tr.E(got[quantity][:, j], m["q"][:, j], oq[:, j], kind)
        print(f"{what} {cls:14s} {quantity:3s} path {j} (f = {FACTORS9[j % 9]:g}) E_orc {e_orc[j]:.1e}  E(kernel, truth) {e:.1e}  asserted K: "
              f"{int(gate[:, j].sum())} of {b.nprof} profiles")
        tr.record(f"{what}/E_truth/{cls}/{kind}/{quantity}", e)
        if not e <= 4 * e_orc[j] + rnd:
            fails.append(f"{quantity} path {j}: E(kernel, truth) {e:.2e} > 4 x {e_orc[j]:.2e} + rounding")
    tol = 1e-6 + (F24 if kind == 4 else 0.0)
    lay = np.broadcast_to(b.lay[:, None, :], (b.nprof, npath, b.lm))
    lev = np.broadcast_to(b.lev[:, None, :], (b.nprof, npath, b.lm + 1))
    for k in fields:   # 2. the K fields, per column over the layer axis
        assert np.all(got[k][~(lev if k == "k_tz" else lay)] == 0), f"{what}: {k} padding is not zero"
        e, scale, low = k_columns(got[k], m[k], m["q"], 2, kind)
        if gate.any():
            assert low[gate].sum() <= 0.25 * low[gate].size, f"{what}: {k}: more than a quarter of the columns lie below the float floor"
        ea = float(np.max(e[gate], initial=0.0))
        er = float(np.max(e[~gate], initial=0.0))
        print(f"{what} {cls:14s} {quantity:3s} {k:6s} k_error asserted {ea:.1e}  recorded only {er:.1e}  below the float floor {int(low.sum())}")
        tr.record(f"{what}/{k}/{cls}/{kind}/{quantity}", ea)
        tr.record(f"{what}/{k}_recorded_only/{cls}/{kind}/{quantity}", er)
        if not ea <= tol:
            fails.append(f"{k} {ea:.2e}")
    one = b.irt == 1
    assert np.all(got["k_sfc"][~one] == 0), f"{what}: k_sfc is not zero for irt 2, 3"
    ks, kr = np.asarray(got["k_sfc"], LD), m["k_sfc"]
    assert np.all(np.isfinite(ks)), f"{what}: k_sfc"
    with np.errstate(all="ignore"):
        if kind == 8:
            e = np.abs(ks - kr) / np.maximum(np.abs(kr), LD(1e-290))
        else:
            held = np.abs(kr) >= LD(tr.SGL_FLOOR)
            e = np.where(held, np.abs(ks - kr) / np.abs(kr), np.where(np.abs(ks) <= 2 * LD(tr.SGL_FLOOR), LD(0), LD(np.inf)))
    e = e.max(axis=(2, 3))
    ea, er = float(np.max(e[gate & one[:, None]], initial=0.0)), float(np.max(e[~gate & one[:, None]], initial=0.0))
    print(f"{what} {cls:14s} {quantity:3s} k_sfc  relative asserted {ea:.1e}  recorded only {er:.1e}")
    tr.record(f"{what}/k_sfc/{cls}/{kind}/{quantity}", ea)
    if not ea <= tol:
        fails.append(f"k_sfc {ea:.2e}")
    assert not fails, f"{what} {cls} {quantity}: " + "; ".join(fails)


def term_bounds(m, e_orc, kind):
    """The monochromatic bound b of every term of the fields in m ([nprof, npath, ..., nwn]): bounds 1 and 2 of the module docstring."""
    with np.errstate(all="ignore"):
        fac = np.where(np.isfinite(e_orc), 4 * e_orc + 64 * EPS, np.inf)[None, :, None]
        q = np.abs(np.asarray(m["q"], np.float64))
        bq = np.minimum(np.where(q == 0, 0.0, fac * q), 1e300)   # (an oracle that breaks a rule of E: no bound, and no inf x 0 in the contraction)
        b = {"q": bq}
        for k in m:
            if k in ("k_t", "k_tz"):
                scale = np.maximum(np.abs(m[k]).max(axis=2), LD(1e-6) * np.abs(m["q"]))
                b[k] = np.broadcast_to(1e-6 * np.asarray(scale, np.float64)[:, :, None, :], m[k].shape)
            elif k == "k_sfc":
                b[k] = 1e-6 * np.abs(np.asarray(m[k], np.float64))
    return b


def view_gate(op, gate):
    """[nprof, nview]: every path of the view is asserted (an empty view: S = 0 asks for the exact 0 anyway)."""
    return np.stack([gate[:, op.view_start[v]:op.view_start[v + 1]].all(axis=1) for v in range(op.nview)], axis=1)


def contributions(op):
    """tiles(view) x blocks(channel) [nview, nchan]: the additions into a float element of the _dev entries."""
    tiles = -(-np.diff(op.view_start) // 4)
    blocks = np.array([len(set(np.nonzero(op.chan == c)[0] // 64)) for c in range(op.nchan)])
    return tiles[:, None] * blocks[None, :]


def live_terms(b, k, npath):
    """1 where a monochromatic term of field k exists ([nprof, npath, ..., nwn]): active layers and levels, K_SFC of irt 1."""
    sh = {"y": (), "k_t": (b.lm,), "k_tz": (b.lm + 1,), "k_sfc": (3,)}[k]
    m = {"y": np.ones((b.nprof, 1)), "k_t": b.lay, "k_tz": b.lev, "k_sfc": np.broadcast_to((b.irt == 1)[:, None], (b.nprof, 3))}[k]
    return np.broadcast_to(np.asarray(m, np.float64).reshape((b.nprof, 1) + sh + (1,)), (b.nprof, npath) + sh + (b.nwn,))


def check_contracted(what, case, quantity, op, got, m, bterm, vgate, fields, dev=False):
    """Bound 3 (5 with dev) of the module docstring on the contracted outputs `fields` of got; "y" is held on every class, a K field
    where vgate[profile, view], and an element with S = 0 is exactly 0 there; an element without a term (padding, an empty view, an
    empty channel, K_SFC of irt 2 and 3) is exactly 0 on every class."""
    kind, cls = case.kind, case.cls
    W = op.dense()
    fails = []
    for k in fields:
        mk = "q" if k == "y" else k
        ref, S = oc.reference(op, m[mk])
        B = oc.contract(np.abs(W), bterm[mk], op.nview, op.nchan)
        g = np.asarray(got[k], np.float64)
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(S)), f"{what}: the truth's {k} is not finite"
        sel = np.ones(S.shape, bool) if k == "y" else np.broadcast_to(vgate.reshape(vgate.shape + (1,) * (ref.ndim - 2)), S.shape)
        none = oc.contract(np.abs(W), live_terms(case.b, k, op.npath), op.nview, op.nchan) == 0   # padding, an empty view or channel, irt 2, 3
        assert np.all(g[none] == 0) and np.all(g[(S == 0) & sel] == 0), f"{what}: {k} is not exactly 0 where no term is"
        n = contributions(op).reshape((1, op.nview) + (1,) * (ref.ndim - 3) + (op.nchan,))
        with np.errstate(all="ignore"):
            bound = B + ((64 * EPS if kind == 8 else F24) + ((1 + n) * F24 if dev else 0.0)) * S
            ratio = np.abs(g - ref) / bound
        ratio = np.where(S == 0, 0.0, np.where(np.isfinite(g), ratio, np.inf))
        floor = tr.DBL_TINY if kind == 8 else tr.SGL_FLOOR   # below it the output format does not hold the element's terms: E's rule
        low = (S > 0) & (S < floor)
        ratio = np.where(low, np.where(np.abs(g) <= 2 * floor, 0.0, np.inf), ratio)
        ea, er = float(np.max(ratio[sel], initial=0.0)), float(np.max(ratio[~sel], initial=0.0))
        print(f"{what} {cls:14s} {quantity:3s} {k:5s} max |got - ref| / bound: asserted {ea:.2e}  recorded only {er:.2e}  below the format's floor {int(low.sum())}")
        tr.record(f"{what}/{k}/{cls}/{kind}/{quantity}", ea)
        tr.record(f"{what}/{k}_recorded_only/{cls}/{kind}/{quantity}", er)
        if not ea <= 1.0:
            fails.append(f"{k} {ea:.2e} x the bound")
    assert not fails, f"{what} {cls} {quantity}: " + "; ".join(fails)


def test_every_factor_but_the_smallest_is_asserted(case):
    """The statement of the module docstring about which K figures are asserted, from the oracle and the truth alone."""
    if case.cls in tr.CANCELLING:
        return
    for i, f in enumerate(FACTORS9):
        if f != 1e-3 or case.cls not in ("thin", "mixed"):
            assert case.ref(i)["gate"].all(), (case.name, case.cls, f)


# ---- monortm_hip_rtm_jac ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", ["rad", "tb"])
def test_rtm_jac(case, quantity):
    """rtm_jac_kernel<R, 8, false> (A64, B30) and <R, 2, false> (C12), R = double and float."""
    r, b = case.r, case.b
    got, got_n = raw_jac(r, b, case.a0, quantity), raw_jac(r, b, case.an, quantity)
    assert same(got, got_n), "padding beyond nlay[p] is read"
    got = {k: v[:, None] for k, v in got.items()}
    fields = ("k_o", "k_t", "k_tz")
    m, oq, gate, e_orc = case.mono(1, quantity, fields + ("k_sfc",))
    check_mono(f"rtm_jac {case.name}", case, quantity, got, m, oq, gate, e_orc, fields)


# ---- monortm_hip_rtm_scan_jac ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", ["rad", "tb"])
def test_rtm_scan_jac(case, quantity):
    """rtm_scan_jac_kernel<R, 8, 4, false> and <R, 2, 4, false> with five paths (tiles of 4 + 1)."""
    r, b = case.r, case.b
    got = raw_scan_jac(r, b, case.a0, case.paths(5), quantity)
    got_n = raw_scan_jac(r, b, case.an, case.paths(5, np.nan), quantity)
    assert same(got, got_n), "padding beyond nlay[p] is read"
    fields = ("k_o", "k_t", "k_tz")
    m, oq, gate, e_orc = case.mono(5, quantity, fields + ("k_sfc",))
    check_mono(f"rtm_scan_jac {case.name}", case, quantity, got, m, oq, gate, e_orc, fields)


@pytest.mark.parametrize("quantity", ["rad", "tb"])
def test_rtm_scan_jac_k_path(case, quantity):
    """K_PATH = O x dq/dtau of the same call, by bound 2 on its own columns: the one field that weighs a layer's dq/dtau with its O.
    It is what found the residue of pass 2's upward prefix sum (LABNOTES section 23): held as a running difference from pass 1's group
    sum, sum_{l<k} up_l kept ~10 eps x RUP at and under an opaque layer - invisible on K_O's scale, 1.5e-6 .. 2.4e-5 here on
    `opaque_bottom`, `opaque_top`, `opaque_middle` and `underflow` once the layer's O = 1e6 multiplies it.  With the error-free sum
    (jac_up_sum, rtm_tile.hpp) the four classes stand where K_O does: 1.5e-9, 1.8e-9, 8.4e-8, 2.3e-10 (MI355X)."""
    r, b = case.r, case.b
    got = raw_scan_jac(r, b, case.a0, case.paths(5), quantity)
    m, oq, gate, e_orc = case.mono(5, quantity, ("k_path",))
    e, scale, low = k_columns(got["k_path"], m["k_path"], m["q"], 2, case.kind)
    lay = np.broadcast_to(b.lay[:, None, :], (b.nprof, 5, b.lm))
    assert np.all(got["k_path"][~lay] == 0), "k_path padding is not zero"
    if gate.any():
        assert low[gate].sum() <= 0.25 * low[gate].size, "more than a quarter of the columns lie below the float floor"
    ea, er = float(np.max(e[gate], initial=0.0)), float(np.max(e[~gate], initial=0.0))
    print(f"rtm_scan_jac {case.name} {case.cls:14s} {quantity:3s} k_path k_error asserted {ea:.1e}  recorded only {er:.1e}")
    tr.record(f"rtm_scan_jac {case.name}/k_path/{case.cls}/{case.kind}/{quantity}", ea)
    tr.record(f"rtm_scan_jac {case.name}/k_path_recorded_only/{case.cls}/{case.kind}/{quantity}", er)
    assert ea <= 1e-6 + (F24 if case.kind == 4 else 0.0), f"rtm_scan_jac {case.name} {case.cls} {quantity}: k_path {ea:.2e}"


# ---- monortm_hip_rtm_obs_jac and monortm_hip_rtm_obs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", ["rad", "tb"])
@pytest.mark.parametrize("views,chmap", OPS)
def test_rtm_obs_jac_and_obs(case, views, chmap, quantity):
    """The host entries: rtm_obs_jac_kernel<R, double, G, 4, false> and rtm_obs_kernel<R, double, G, 4>, G = 8 (A64, B30) and 2 (C12); on
    a real_kind 4 context, TB, classes `lognormal` and `opaque_middle`, the _dev entries as well (<float, float, G, 4>)."""
    r, b = case.r, case.b
    op = oc.operator(views, chmap, b.nwn)
    path, path_n = case.paths(op.npath), case.paths(op.npath, np.nan)
    h = r.obs_create(op)
    try:
        adj, adj_n = raw_obs_jac(r, b, case.a0, path, quantity, h, op), raw_obs_jac(r, b, case.an, path_n, quantity, h, op)
        y, y_n = raw_obs(r, b, case.a0, path, QUANT[quantity], h, op), raw_obs(r, b, case.an, path_n, QUANT[quantity], h, op)
        dev = dev_calls(r, b, case.a0, path, h, op) if case.kind == 4 and quantity == "tb" and case.cls in DEV_CLASSES else None
    finally:
        r.obs_destroy(h)
    assert same(adj, adj_n) and np.array_equal(y, y_n, equal_nan=True), "padding beyond nlay[p] is read"
    fields = ("k_t", "k_tz", "k_sfc")
    m, oq, gate, e_orc = case.mono(op.npath, quantity, fields)
    bterm, vgate = term_bounds(m, e_orc, case.kind), view_gate(op, gate)
    what = f"{case.name} {views}/{chmap}"
    check_contracted(f"rtm_obs_jac {what}", case, quantity, op, adj, m, bterm, vgate, OBS_OUT)
    check_contracted(f"rtm_obs {what}", case, quantity, op, {"y": y}, m, bterm, vgate, ("y",))
    if dev is not None:
        check_contracted(f"rtm_obs_jac_dev {what}", case, quantity, op, dev[0], m, bterm, vgate, OBS_OUT, dev=True)
        check_contracted(f"rtm_obs_dev {what}", case, quantity, op, {"y": dev[1]}, m, bterm, vgate, ("y",), dev=True)


def centres(op, wn):
    """Per channel the wchan-weighted mean wavenumber of its members, as tests/test_obs_forward.py::test_band_tb passes them."""
    return np.array([np.sum(op.wchan[op.chan == c] * wn[op.chan == c]) / np.sum(op.wchan[op.chan == c]) for c in range(op.nchan)])


@pytest.mark.parametrize("views", ["A", "B"])
def test_band_tb(case, views):
    """Quantity 2 of monortm_hip_rtm_obs: positive weights on the comb map, vcen = the weighted mean wavenumber of each channel.  The
    reference is RADCN2 vc / log1p(c3(vc) / ybar) of the truth's contracted radiance, contracted and converted in longdouble; bound 4 of
    the module docstring."""
    r, b, kind = case.r, case.b, case.kind
    op = oc.operator(views, "comb", b.nwn, mixed=False)
    vcen = centres(op, b.wn)
    h = r.obs_create(op)
    try:
        got = raw_obs(r, b, case.a0, case.paths(op.npath), 2, h, op, vcen=vcen)
        got_n = raw_obs(r, b, case.an, case.paths(op.npath, np.nan), 2, h, op, vcen=vcen)
    finally:
        r.obs_destroy(h)
    assert np.array_equal(got, got_n, equal_nan=True), "padding beyond nlay[p] is read"
    m, oq, gate, e_orc = case.mono(op.npath, "rad", ())
    W = op.dense().astype(LD)
    ybar = (m["q"].reshape(b.nprof, -1) @ W.T).reshape(b.nprof, op.nview, op.nchan)         # positive weights: S = ybar
    B = oc.contract(np.abs(op.dense()), term_bounds(m, e_orc, kind)["q"], op.nview, op.nchan)
    live = np.broadcast_to((np.diff(op.view_start) > 0)[None, :, None], ybar.shape)
    assert np.all(got[~live] == 0) and np.all(ybar[live] >= tr.DBL_TINY) and np.all(np.isfinite(ybar))
    vc = np.asarray(vcen, LD)[None, None, :]
    with np.errstate(all="ignore"):
        ref = tr.RADCN2 * vc / np.log1p(tr.RADCN1 * (vc * vc * vc) / ybar)
        rel = np.asarray(B, LD) / ybar + (64 * EPS if kind == 8 else F24)
        ratio = np.abs(np.asarray(got, LD) - ref) / (rel * ref)
    ratio = np.where(live, np.where(np.isfinite(np.asarray(got, LD)), ratio, LD(np.inf)), LD(0))
    e = float(np.max(ratio))
    print(f"band TB {case.name} {views} {case.cls:14s} max error / bound {e:.2e}  TB {float(ref[live].min()):.1f} .. {float(ref[live].max()):.1f} K")
    tr.record(f"band_tb/{case.cls}/{kind}", e)
    assert e <= 1.0, f"band TB {case.name} {views} {case.cls}: {e:.2e} x the bound"


# ---- the surface term where exp(hc v / k tmpsfc) overflows ---------------------------------------------------------------------------
COLD = 60.0                                           # K: hc v / k T > 709.78 (exp overflows a double) above 29599 cm-1


def cold_case(r):
    """B30, `lognormal`, every profile irt 1 with a surface at 60 K; the wavenumbers below the overflow and the same inputs cut to them."""
    b = tr.Batch(tr.BATCHES["B30"], "lognormal", 9100, irt=(1,))
    b.ts[:] = COLD
    a = b.rounded(r.dtype, 0.0)
    over = float(tr.RADCN2) * b.wn / COLD > 709.78
    nlow = int(np.argmax(over))
    assert 64 < nlow < b.nwn and np.all(over[nlow:]) and not np.any(over[:nlow])      # both wavenumber blocks hold samples below it
    bl = types.SimpleNamespace(nprof=b.nprof, lm=b.lm, nwn=nlow, nlay=b.nlay, irt=b.irt, wn=np.ascontiguousarray(b.wn[:nlow]))
    al = dict(a, O=np.ascontiguousarray(a["O"][:, :, :nlow]), em=np.ascontiguousarray(a["em"][:, :nlow]), rf=np.ascontiguousarray(a["rf"][:, :nlow]))
    return b, a, bl, al, nlow


@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("quantity", ["rad", "tb"])
def test_cold_surface_rtm_jac(ctx, quantity, kind):
    """The truth's dq/dTMPSFC underflows to 0 where exp(hc v / k tmpsfc) overflows; 0 x (inf / inf) there was NaN (LABNOTES section 23)."""
    r = ctx[kind]
    b, a, bl, al, nlow = cold_case(r)
    got, low = raw_jac(r, b, a, quantity), raw_jac(r, bl, al, quantity)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert np.all(got["k_sfc"][:, 0, nlow:] == 0) and np.any(got["k_sfc"][:, 0, :nlow] != 0)
    for k in got:
        np.testing.assert_array_equal(got[k][..., :nlow], low[k], err_msg=k)


@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("quantity", ["rad", "tb"])
def test_cold_surface_rtm_scan_jac(ctx, quantity, kind):
    r = ctx[kind]
    b, a, bl, al, nlow = cold_case(r)
    path = np.ascontiguousarray(np.broadcast_to(np.asarray(FACTORS9[:5], r.dtype)[None, :, None], (b.nprof, 5, b.lm)))
    got, low = raw_scan_jac(r, b, a, path, quantity), raw_scan_jac(r, bl, al, path, quantity)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert np.all(got["k_sfc"][:, :, 0, nlow:] == 0) and np.any(got["k_sfc"][:, :, 0, :nlow] != 0)
    for k in got:
        np.testing.assert_array_equal(got[k][..., :nlow], low[k], err_msg=k)


@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("quantity", ["rad", "tb"])
def test_cold_surface_rtm_obs_jac(ctx, quantity, kind):
    """Views A; channels 0 .. 4 comb the wavenumbers below the overflow (members in both blocks), channels 5 and 6 those above it: the
    call cut to the lower wavenumbers has the first five, bit for bit, and K_SFC[0] of the last two is exactly 0."""
    r = ctx[kind]
    b, a, bl, al, nlow = cold_case(r)
    vs, wp = oc.view_arrays("A")
    i = np.arange(b.nwn)
    chan = np.where(i < nlow, i % 5, 5 + i % 2).astype(np.int32)
    wc = np.random.default_rng(9).normal(0.0, 1.0, b.nwn)
    op, opl = api.ObsOperator(vs, wp, chan, wc, nchan=7), api.ObsOperator(vs, wp, chan[:nlow], wc[:nlow], nchan=5)
    path = np.ascontiguousarray(np.broadcast_to(np.asarray(FACTORS9, r.dtype)[None, :, None], (b.nprof, 9, b.lm)))
    h, hl = r.obs_create(op), r.obs_create(opl)
    try:
        got, low = raw_obs_jac(r, b, a, path, quantity, h, op), raw_obs_jac(r, bl, al, path, quantity, hl, opl)
    finally:
        r.obs_destroy(h)
        r.obs_destroy(hl)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert np.all(got["k_sfc"][:, :, 0, 5:] == 0) and np.any(got["k_sfc"][:, :, 0, :5] != 0)
    for k in got:
        np.testing.assert_array_equal(got[k][..., :5], low[k], err_msg=k)
