"""The step of the adaptive loop on the GPU (monortm_hip_oe_step_lm[_dev], the DUAL instantiations of oe_step_kernel; DESIGN.md section
3.15) against the long-double step_lm of tests/oe_lm_truth.py, on the cases of tests/test_oe_step.py (variances) and
tests/oe_full_truth.py (a full Se): (nview, nchan) from MSHAPES x n in 1, 7, 65, 300, three profiles, per-profile and shared Sa / Se.

The iterate's dual vector c is Sa^-1 (x - xa) solved in float64: the truth takes the same float64 c as an input, so the identity is not
under test here (tests/test_oe_lm_cpu.py holds it) - the kernel's arithmetic is.

Bounds: c_new within 1e-12 of the profile's max |c_new|, cost within 1e-12 relative - the bound DESIGN section 3.13 stands on, eps x
cond(M) x 10 at cond(M) < 1e4, which every case asserts from the truth's own M first: q = b^T u is a dot product of two solves against
the same factor, as a . u in x_new is."""
import ctypes as C
import os

import numpy as np
import pytest

import oe_full_truth as oft
import oe_lm_truth as lt
import test_oe_step as tos
from monortm_amd import api
from test_oe_step import EARG, EUNSUPPORTED, KEYS, MSHAPES, NJAC, NSTATES, bits, dev  # noqa: F401  (dev: the line-table-free context)

pytestmark = pytest.mark.gpu

BASE = ("x_new", "post_var", "avk_diag", "chi2", "status")
DUAL = ("c_new", "cost")
GAMMA = [0.0, 10.0, 2.5]


def case(nview, nchan, n, full, seed=0, shared=False, nprof=3):
    """A case of test_oe_step.make (variances, under "Se") or oe_full_truth.make_gpu_case, with c = Sa^-1 (x - xa) in float64."""
    if full:
        c = oft.make_gpu_case(nview, nchan, n, seed=seed, nprof=nprof, shared_sa=shared, shared_se=shared)
    else:
        c = tos.make(nview, nchan, n, seed=seed, nprof=nprof, shared_sa=shared, shared_se=shared)
        c["Se"] = c.pop("se")
    c["c"] = np.stack([np.linalg.solve(np.tril(S) + np.tril(S, -1).T, d) for S, d in zip(c["Sa"], c["x"] - c["xa"])])
    c["full"] = full
    return c


def upload(db, c, gamma=None, sl=slice(None)):
    import torch

    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(db.dev)  # noqa: E731
    t = {k: up(v[sl]) for k, v in c["ka"].items()}
    t.update(y=up(c["F"][sl].reshape(-1, c["nview"], c["nchan"])), y_obs=up(c["y"][sl].reshape(-1, c["nview"], c["nchan"])), x=up(c["x"][sl]),
             xa=up(c["xa"][sl]), Sa=up(c["Sa"][0] if c["shared_sa"] else c["Sa"][sl]), Se=up(c["Se"][0] if c["shared_se"] else c["Se"][sl]),
             gamma=None if gamma is None else up(np.asarray(gamma, np.float64)[sl]), c=None if c["c"] is None else up(c["c"][sl]))
    return t


def call(db, c, t, entry="lm", want=()):
    """DeviceBatch.oe_step_lm (or, entry "full", oe_step_full on the same tensors): outputs as numpy.  se_kind is stated - three
    profiles of three measurements leave a [3, 3] Se ambiguous."""
    import torch

    args = (t, (c["kind"], c["row"]), t["y_obs"], t["x"], t["xa"], t["Sa"], t["Se"])
    kw = dict(gamma=t["gamma"], want=want, se_kind=int(c["full"]))
    out = db.oe_step_lm(*args, c=t["c"], **kw) if entry == "lm" else db.oe_step_full(*args, **kw)
    torch.cuda.synchronize()
    db.check()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def same(a, b, keys):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def check_truth(c, got, gamma, what):
    worst = dict(c_new=0.0, cost=0.0, x_new=0.0)
    for p in range(c["K"].shape[0]):
        t = lt.step_lm(c["K"][p], c["Sa"][p], c["Se"][p], c["xa"][p], c["x"][p], c["y"][p], c["F"][p], gamma[p], c["c"][p])
        cond = np.linalg.cond(np.asarray(t["M"], np.float64))
        assert cond < 1e4, cond                                   # what the bounds below stand on
        assert got["status"][p] == 0
        worst["c_new"] = max(worst["c_new"], float(np.max(np.abs(got["c_new"][p].astype(lt.LD) - t["c_new"])) / np.max(np.abs(t["c_new"]))))
        worst["cost"] = max(worst["cost"], float(abs(lt.LD(got["cost"][p]) - t["cost"]) / t["cost"]))
        worst["x_new"] = max(worst["x_new"], float(np.max(np.abs(got["x_new"][p].astype(lt.LD) - t["x_new"])) / np.max(np.abs(t["x_new"] - c["x"][p]))))
    print(f"{what}: worst error / scale " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["c_new"] <= 1e-12 and worst["cost"] <= 1e-12 and worst["x_new"] <= 1e-12


# ---- 1. the numbers, and the bits of the full step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["variances", "full_se"])
@pytest.mark.parametrize("n", NSTATES)
@pytest.mark.parametrize("nview,nchan", MSHAPES)
def test_dual_step_matches_the_truth_and_the_full_step(dev, nview, nchan, n, full):
    """Per-profile Sa and Se, then shared ones: c_new and cost against the truth; everything else bit-equal to oe_step_full."""
    _, db = dev
    for kw in (dict(seed=0), dict(seed=1, shared=True)):
        c = case(nview, nchan, n, full, **kw)
        t = upload(db, c, GAMMA)
        got = call(db, c, t)
        check_truth(c, got, GAMMA, f"m {nview * nchan} n {n} {'full' if full else 'diag'} {'shared' if kw.get('shared') else 'per-profile'}")
        same(got, call(db, c, t, "full"), BASE)


@pytest.mark.parametrize("full", [False, True], ids=["variances", "full_se"])
def test_diagnostics_ride_along_unchanged(dev, full):
    _, db = dev
    c = case(5, 13, 65, full)
    t = upload(db, c, GAMMA)
    want = ("gain_t", "avk", "post_cov", "dofs")
    same(call(db, c, t, want=want), call(db, c, t, "full", want=want), BASE + want)


# ---- 2. the same bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nview,nchan,n,full", [(5, 13, 300, False), (8, 16, 65, True), (3, 1, 7, True)])
def test_same_bits_without_c_repeated_and_alone(dev, nview, nchan, n, full):
    """c = None against c = 0; a call repeated; profile 1 alone against profile 1 in the batch."""
    _, db = dev
    c = case(nview, nchan, n, full)
    t = upload(db, c, GAMMA)
    a = call(db, c, t)
    same(a, call(db, c, t), BASE + DUAL)
    same({k: v[1:2] for k, v in a.items()}, call(db, c, upload(db, c, GAMMA, slice(1, 2))), BASE + DUAL)
    c["c"] = np.zeros_like(c["c"])
    zero = call(db, c, upload(db, c, GAMMA))
    c["c"] = None
    none = call(db, c, upload(db, c, GAMMA))
    same(zero, none, BASE + DUAL)
    assert np.array_equal(bits(none["cost"]), bits(none["chi2"])) and not np.array_equal(zero["c_new"], a["c_new"])


# ---- 3. one profile fails, the batch does not -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["variances", "full_se"])
def test_failure_keeps_c_and_marks_its_profile_only(dev, full):
    """Profile 1: a negative gamma; profile 2: a NaN in K.  c_new = c, cost = 0; profile 0 as it is alone."""
    _, db = dev
    c = case(5, 13, 65, full)
    solo = call(db, c, upload(db, c, GAMMA, slice(0, 1)))
    s = int(np.nonzero(c["kind"] == 0)[0][0])
    c["ka"]["k_t"][2, 3, c["row"][s], 5] = np.nan
    got = call(db, c, upload(db, c, [0.0, -1.0, 2.5]))
    assert got["status"].tolist() == [0, 1, 1]
    for p in (1, 2):
        assert np.array_equal(bits(got["c_new"][p]), bits(c["c"][p])) and got["cost"][p] == 0 and np.array_equal(bits(got["x_new"][p]), bits(c["x"][p]))
    same({k: v[:1] for k, v in got.items()}, solo, BASE + DUAL)
    c["c"] = None
    got = call(db, c, upload(db, c, [0.0, -1.0, 2.5]))
    assert np.all(got["c_new"][1:] == 0) and np.all(got["cost"][1:] == 0) and got["cost"][0] == got["chi2"][0]


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def raw(rt, t, c, out, **over):
    """monortm_hip_oe_step_lm_dev through ctypes; over: a map, se_kind, or names of arrays handed over as NULL (drop) or swapped (alias)."""
    drop = over.get("drop", ())
    d = lambda k: None if k in drop or {**t, **out}.get(k) is None else C.c_void_p({**t, **out}[k].data_ptr())  # noqa: E731
    kind = np.ascontiguousarray(over.get("kind", c["kind"]), np.int32)
    row = np.ascontiguousarray(c["row"], np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return rt.lib.monortm_hip_oe_step_lm_dev(rt.ctx, 3, c["nview"], c["nchan"], c["lm"], NJAC, over.get("nstate", len(kind)), p(kind), p(row),
                                             *[d(k) for k in KEYS], d("y"), d("y_obs"), d("x"), d("xa"), d("Sa"), 1, d("Se"),
                                             over.get("se_kind", int(c["full"])), 1, d("gamma"), *[d(k) for k in BASE], None, None, None, None,
                                             d("c"), d(over.get("c_new", "c_new")), d("cost"), None)


def test_refusals_come_before_any_launch(dev):
    import torch

    rt, db = dev
    c = case(5, 13, 7, True)
    t = upload(db, c, GAMMA)
    got = call(db, c, t)
    full = call(db, c, t, "full")
    out = {k: torch.full_like(torch.as_tensor(got[k]), -7).to(db.dev) for k in BASE + DUAL}
    assert raw(rt, t, c, out) == 0
    torch.cuda.synchronize()
    same({k: v.cpu().numpy() for k, v in out.items()}, got, BASE + DUAL)
    for v in out.values():
        v.fill_(-7)
    k5 = c["kind"].copy()
    k5[3] = 5
    for over in (dict(kind=k5), dict(se_kind=2), dict(nstate=0), dict(nstate=2049), dict(drop=("x_new",)), dict(drop=("Se",)), dict(c_new="c")):
        assert raw(rt, t, c, out, **over) == EARG, over
        assert rt.lib.monortm_hip_last_error(rt.ctx)
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in out.values())                                   # nothing ran
    assert raw(rt, t, c, out, drop=("c", "c_new", "cost", "post_var", "avk_diag", "chi2")) == 0   # all three NULL: the full step's launch
    torch.cuda.synchronize()
    assert np.array_equal(bits(out["x_new"].cpu().numpy()), bits(full["x_new"])) and bool((out["c_new"] == -7).all())
    rt4 = api.MonoRTM("", 0.0, 0.0, real_kind=4)
    assert raw(rt4, t, c, out) == EUNSUPPORTED
    rt4.close()
    with pytest.raises(ValueError):
        db.oe_step_lm(t, (c["kind"], c["row"]), t["y_obs"], t["x"], t["xa"], t["Sa"], t["Se"], c=t["c"].float(), se_kind=1)


# ---- 5. the host entry, sharded -------------------------------------------------------------------------------------------------------------
def test_host_entry_sharded_equals_the_device_entry(dev):
    """MonoRTM.oe_step_lm on a three-shard context (blocks of 2, 2, 1 profiles) and on one device against DeviceBatch.oe_step_lm."""
    rt, db = dev
    old = os.environ.get("MONORTM_DEVICES")
    os.environ["MONORTM_DEVICES"] = "0,0,0"
    try:
        multi = api.MonoRTM("", 0.0, 0.0, ngpu=0)
    finally:
        if old is None:
            del os.environ["MONORTM_DEVICES"]
        else:
            os.environ["MONORTM_DEVICES"] = old
    assert multi.lib.monortm_hip_device_count(multi.ctx) == 3
    c = case(3, 5, 7, True, nprof=5)
    gamma = np.array([0.0, 10.0, 0.0, 1.0, 0.5])
    want = ("dofs",)

    def host(r):
        jac = dict(c["ka"], y=c["F"].reshape(-1, 3, 5))
        return r.oe_step_lm(jac, (c["kind"], c["row"]), c["y"].reshape(-1, 3, 5), c["x"], c["xa"], c["Sa"], c["Se"], gamma, c["c"], want=want, se_kind=1)

    whole, one = host(multi), host(rt)
    multi.close()
    import torch

    t = upload(db, c, gamma)
    out = db.oe_step_lm(t, (c["kind"], c["row"]), t["y_obs"], t["x"], t["xa"], t["Sa"], t["Se"], gamma=t["gamma"], c=t["c"], want=want, se_kind=1)
    torch.cuda.synchronize()
    devout = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.all(whole["status"] == 0)
    same(whole, one, BASE + DUAL + want)
    same(whole, devout, BASE + DUAL + want)
