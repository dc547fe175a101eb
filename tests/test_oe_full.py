"""The full optimal-estimation step on the GPU (monortm_hip_oe_step_full[_dev], oe_kernel.hip) against the
long-double step_full of tests/oe_full_truth.py.

K comes through the scrambled five-kind state map of tests/test_oe_step.py; Se is the full matrix of oe_full_truth.full_se.  Shapes:
m from test_oe_step.MSHAPES (1, 3, 64, 65, 128), n in 1, 7, 64, 65, 130, 300 - against the 64-wide tiles of oe_cov_kernel one state, less
than a tile row, one tile exactly, one tile plus one, three tiles (mirrored off-diagonal tiles exist) and more than the 256 threads of a
workgroup -, 3 profiles.

Bounds: x_new, post_var, avk_diag as tests/test_oe_step.py (1e-12 of the largest step, of max Sa_ii, absolute); gain_t within 1e-12 of the
profile's max |G|; avk within 1e-12 of max(1, max |A|); post_cov within 1e-12 of max Sa_ii; dofs within 1e-11 max(1, n).  chi2 with a
full Se comes out of a forward substitution, whose error is bounded by m eps cond(L_e), doubled for the square: (m + 3) 2^-52 cond(Se)
relative, cond(Se) taken from the truth's Se, is looser than that."""
import ctypes as C
import os

import numpy as np
import pytest

import oe_full_truth as oft
import test_oe_step as tos
from monortm_amd import api, synth
from test_oe_step import EARG, EUNSUPPORTED, KEYS, MSHAPES, NJAC, bits, same_bits

pytestmark = pytest.mark.gpu

BASE = ("x_new", "post_var", "avk_diag", "chi2", "status")
WANT = ("gain_t", "avk", "post_cov", "dofs")
ALL = BASE + WANT


@pytest.fixture(scope="module")
def dev():
    """(a context without a line table, a DeviceBatch on it: oe_step_full reads none of the batch's own arrays)."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    rt = api.MonoRTM("", 0.0, 0.0)
    db = api.DeviceBatch(rt, [synth.perturbed_profile(0, synth.c2_channels(4, seed=1), nlay=3)])
    yield rt, db
    rt.close()


def upload(db, c, gamma=None, sl=slice(None), Se=None):
    """The device tensors of the profiles sl of a case; Se: the case's own (its first when shared), or what is given ([nprof]...)."""
    import torch

    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(db.dev)  # noqa: E731
    t = {k: up(v[sl]) for k, v in c["ka"].items()}
    if Se is None:
        Se = c["Se"]
    t.update(y=up(c["F"][sl].reshape(-1, c["nview"], c["nchan"])), y_obs=up(c["y"][sl].reshape(-1, c["nview"], c["nchan"])), x=up(c["x"][sl]),
             xa=up(c["xa"][sl]), Sa=up(c["Sa"][0] if c["shared_sa"] else c["Sa"][sl]), Se=up(Se[0] if c["shared_se"] else Se[sl]),
             gamma=None if gamma is None else up(np.asarray(gamma, np.float64)[sl]))
    return t


def call(db, c, t, want=WANT, se_kind=1):
    """(se_kind is stated: three profiles of three measurements leave a [3, 3] Se ambiguous)"""
    import torch

    out = db.oe_step_full(t, (c["kind"], c["row"]), t["y_obs"], t["x"], t["xa"], t["Sa"], t["Se"], gamma=t["gamma"], want=want, se_kind=se_kind)
    torch.cuda.synchronize()
    db.check()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def run(db, c, gamma=None, sl=slice(None), Se=None, want=WANT):
    t = upload(db, c, gamma, sl, Se)
    return call(db, c, t, want), t


def check_truth(c, got, gamma, what):
    """Every output of every profile against step_full; prints the worst error / scale per output, then asserts the module's bounds."""
    worst = {k: 0.0 for k in ("x_new", "post_var", "avk_diag", "chi2", "gain_t", "avk", "post_cov", "dofs")}
    nprof, m, n = c["K"].shape
    chi2_bound = 0.0
    for p in range(nprof):
        g = 0.0 if gamma is None else gamma[p]
        t = oft.step_full(c["K"][p], c["Sa"][p], c["Se"][p], c["xa"][p], c["x"][p], c["y"][p], c["F"][p], g)
        smax = np.max(np.diag(c["Sa"][p]))
        scale = dict(x_new=np.max(np.abs(t["x_new"] - c["x"][p])), post_var=smax, avk_diag=oft.LD(1), chi2=t["chi2"],
                     gain_t=np.max(np.abs(t["gain_t"])), avk=max(oft.LD(1), np.max(np.abs(t["avk"]))), post_cov=smax, dofs=oft.LD(max(1, n)))
        for k in worst:
            worst[k] = max(worst[k], float(np.max(np.abs(got[k][p].astype(oft.LD) - t[k])) / scale[k]))
        chi2_bound = max(chi2_bound, (m + 3) * 2.0 ** -52 * np.linalg.cond(np.asarray(t["Se"], np.float64)))
        assert got["status"][p] == 0
    print(f"{what}: worst error / scale " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k in ("x_new", "post_var", "avk_diag", "gain_t", "avk", "post_cov"):
        assert worst[k] <= 1e-12, (k, worst[k])
    assert worst["dofs"] <= 1e-11 and worst["chi2"] <= chi2_bound


# ---- 1. the numbers, at every seam ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", oft.NFULL)
@pytest.mark.parametrize("nview,nchan", MSHAPES)
def test_full_step_matches_the_long_double_truth(dev, nview, nchan, n):
    """Per-profile Sa and full Se with gamma 0 / 10 / 0, then shared Sa and Se with gamma NULL."""
    _, db = dev
    gamma = [0.0, 10.0, 0.0]
    c = oft.make_gpu_case(nview, nchan, n)
    got, _ = run(db, c, gamma)
    check_truth(c, got, gamma, f"m {nview * nchan} n {n} per-profile")
    c = oft.make_gpu_case(nview, nchan, n, seed=1, shared_sa=True, shared_se=True)
    got, _ = run(db, c, None)
    check_truth(c, got, None, f"m {nview * nchan} n {n} shared")


# ---- 2. the same bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nview,nchan,n", [(5, 13, 300), (8, 16, 65), (3, 1, 7)])
def test_variances_without_matrices_are_the_step_itself(dev, nview, nchan, n):
    """(a) se_kind 0 and nothing wanted: the bits of oe_step.  (b) Se = diag(se) as a matrix: the bits of oe_step but for chi2, which is
    the same sum through a square root and back: (m + 3) 2^-52 relative."""
    _, db = dev
    gamma = [0.0, 10.0, 0.0]
    c = tos.make(nview, nchan, n)
    ref, t = tos.run(db, c, gamma)
    t["Se"] = t["se"]
    same_bits(ref, call(db, c, t, want=(), se_kind=0), BASE)
    with_dofs = call(db, c, t, want=("dofs",), se_kind=0)
    same_bits(ref, with_dofs, BASE)
    assert np.allclose(with_dofs["dofs"], ref["dfs"], rtol=0, atol=1e-11 * max(1, n))
    import torch

    t["Se"] = torch.diag_embed(t["se"]).contiguous()
    got = call(db, c, t, want=())
    same_bits(ref, got, ("x_new", "post_var", "avk_diag", "status"))
    assert np.all(np.abs(got["chi2"] - ref["chi2"]) <= (nview * nchan + 3) * 2.0 ** -52 * ref["chi2"])


@pytest.mark.parametrize("nview,nchan,n", [(5, 13, 300), (8, 16, 65), (3, 1, 7), (4, 16, 130)])
def test_diagonals_are_the_vectors_and_the_covariance_is_symmetric(dev, nview, nchan, n):
    """(c) diag(post_cov) is post_var, diag(avk) is avk_diag, post_cov is its transpose: bit for bit."""
    _, db = dev
    got, _ = run(db, oft.make_gpu_case(nview, nchan, n), [0.0, 10.0, 0.0])
    for p in range(3):
        assert np.array_equal(bits(np.diag(got["post_cov"][p]).copy()), bits(got["post_var"][p]))
        assert np.array_equal(bits(np.diag(got["avk"][p]).copy()), bits(got["avk_diag"][p]))
        assert np.array_equal(bits(got["post_cov"][p]), bits(got["post_cov"][p].T.copy()))


@pytest.mark.parametrize("nview,nchan,n", [(5, 13, 300), (8, 16, 65), (3, 1, 7)])
def test_same_bits_repeated_alone_and_replayed(dev, nview, nchan, n):
    """(d) A call repeated; profile 1 alone against profile 1 in the batch; a graph capture replayed after every input changed in place,
    against a plain call on the changed inputs.  Every output."""
    import torch

    _, db = dev
    gamma = [0.0, 10.0, 0.0]
    c = oft.make_gpu_case(nview, nchan, n)
    a, t = run(db, c, gamma)
    same_bits(a, call(db, c, t), ALL)
    alone, _ = run(db, c, gamma, slice(1, 2))
    same_bits({k: v[1:2] for k, v in a.items()}, alone, ALL)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = db.oe_step_full(t, (c["kind"], c["row"]), t["y_obs"], t["x"], t["xa"], t["Sa"], t["Se"], gamma=t["gamma"], want=WANT, se_kind=1)
    torch.cuda.current_stream().wait_stream(s)
    c2 = oft.make_gpu_case(nview, nchan, n, seed=5)
    c2.update(kind=c["kind"], row=c["row"])   # (the captured call holds the first case's map: K is whatever that map reads)
    c2.update(oft.finish_full(tos.gather(c2["ka"], c["kind"], c["row"]), c2["Sa"], np.random.default_rng(3)))
    gamma2 = [10.0, 0.0, 2.5]
    t2 = upload(db, c2, gamma2)
    for k, v in t.items():
        v.copy_(t2[k])
    for k in ALL:
        out[k].fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    replayed = {k: v.cpu().numpy().copy() for k, v in out.items()}
    assert np.all(replayed["status"] == 0) and not np.array_equal(replayed["avk"], a["avk"])
    same_bits(replayed, call(db, c2, t2), ALL)
    check_truth(c2, replayed, gamma2, f"m {nview * nchan} n {n} replayed")


def test_upper_triangles_of_sa_and_se_are_never_read(dev):
    """(e)"""
    _, db = dev
    c = oft.make_gpu_case(5, 13, 130)
    ref, _ = run(db, c, None)
    for k in ("Sa", "Se"):
        c[k] = np.tril(c[k]) + np.triu(np.full_like(c[k], np.nan), 1)
    got, _ = run(db, c, None)
    same_bits(ref, got, ALL)


# ---- 3. one profile fails, the batch does not; refusals ------------------------------------------------------------------------------------
def test_a_bad_se_marks_its_profile_only(dev):
    """Profile 1: a negative diagonal element of Se; 2: an off-diagonal element larger than the diagonals; 3: a NaN in the lower triangle.
    Status 1, x_new = x, every diagnostic 0, the matrices included; profiles 0 and 4 have the bits of their solo runs; check() is clean."""
    _, db = dev
    c = oft.make_gpu_case(5, 13, 65, nprof=5)
    solo = {p: run(db, c, None, slice(p, p + 1))[0] for p in (0, 4)}
    big = 10.0 * float(np.max(np.diagonal(c["Se"], axis1=1, axis2=2)))
    c["Se"][1, 7, 7] = -big
    c["Se"][2, 9, 2] = big
    c["Se"][3, 40, 11] = np.nan
    got, _ = run(db, c, None)         # (call() runs check())
    assert got["status"].tolist() == [0, 1, 1, 1, 0]
    for p in (1, 2, 3):
        assert np.array_equal(bits(got["x_new"][p]), bits(c["x"][p]))
        for k in ALL[1:]:
            if k != "status":
                assert np.all(got[k][p] == 0), (p, k)
    for p in (0, 4):
        same_bits({k: v[p: p + 1] for k, v in got.items()}, solo[p], ALL)
        assert np.any(got["avk"][p] != 0) and np.any(got["gain_t"][p] != 0)


def raw(rt, t, c, **over):
    """monortm_hip_oe_step_full_dev through ctypes; over: se_kind, a map, or names of arrays handed over as NULL (drop)."""
    drop = over.get("drop", ())
    d = lambda k: None if k in drop or t.get(k) is None else C.c_void_p(t[k].data_ptr())  # noqa: E731
    kind = np.ascontiguousarray(over.get("kind", c["kind"]), np.int32)
    row = np.ascontiguousarray(over.get("row", c["row"]), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return rt.lib.monortm_hip_oe_step_full_dev(rt.ctx, tos.NPROF, c["nview"], c["nchan"], c["lm"], NJAC, len(kind), p(kind), p(row),
                                               *[d(k) for k in KEYS], d("y"), d("y_obs"), d("x"), d("xa"), d("Sa"), 1, d("Se"),
                                               over.get("se_kind", 1), 1, d("gamma"), *[d(k) for k in ALL], None)


def test_refusals_come_before_any_launch(dev):
    import torch

    rt, db = dev
    c = oft.make_gpu_case(5, 13, 7)
    got, t = run(db, c, None)
    t.update({k: torch.full_like(torch.as_tensor(got[k]), -7).to(db.dev) for k in ALL})
    assert raw(rt, t, c) == 0
    torch.cuda.synchronize()
    for k in ALL:
        assert np.array_equal(bits(t[k].cpu().numpy()), bits(got[k])), k
        t[k].fill_(-7)
    k5, rbad = c["kind"].copy(), c["row"].copy()
    k5[3] = 5
    s = int(np.nonzero(c["kind"] == 0)[0][0])
    rbad[s] = c["lm"]                                      # K_T has rows 0 .. lm - 1
    for over in (dict(se_kind=2), dict(se_kind=-1), dict(kind=k5), dict(row=rbad), dict(drop=("Se",))):
        assert raw(rt, t, c, **over) == EARG, over
        assert rt.lib.monortm_hip_last_error(rt.ctx)
    rt4 = api.MonoRTM("", 0.0, 0.0, real_kind=4)
    assert raw(rt4, t, c) == EUNSUPPORTED
    rt4.close()
    torch.cuda.synchronize()
    for k in ALL:
        assert np.all(t[k].cpu().numpy() == -7), k        # nothing ran
    assert raw(rt, t, c, drop=("post_var", "avk_diag", "chi2", "gamma") + WANT) == 0    # the optional ones
    torch.cuda.synchronize()
    assert np.array_equal(bits(t["x_new"].cpu().numpy()), bits(got["x_new"])) and np.all(t["avk"].cpu().numpy() == -7)
    assert raw(rt, t, c, drop=("avk_diag", "avk", "gain_t")) == 0                       # dofs without avk_diag; one matrix of two
    torch.cuda.synchronize()
    for k in ("dofs", "post_cov"):
        assert np.array_equal(bits(t[k].cpu().numpy()), bits(got[k])), k
    assert np.all(t["avk"].cpu().numpy() == -7) and np.all(t["gain_t"].cpu().numpy() == -7)
    with pytest.raises(ValueError):
        db.oe_step_full(t, (c["kind"], c["row"]), t["y_obs"], t["x"], t["xa"], t["Sa"], t["Se"][:, :, :-1].contiguous())


# ---- 4. the host entry, sharded ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nprof", [5, 4])
def test_host_entry_sharded_equals_the_block_alone(dev, nprof):
    """MonoRTM.oe_step_full on a three-shard context (blocks of 2, 2, 1 and 2, 2, 0 profiles) against the one-device host call on each
    block alone, bit for bit, and that against the device entry - the matrices included."""
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
    c = oft.make_gpu_case(3, 5, 7, nprof=nprof, shared_se=True)
    gamma = np.array([0.0, 10.0, 0.0, 1.0, 0.5])[:nprof]
    def host(r, sl):
        jac = dict({k: v[sl] for k, v in c["ka"].items()}, y=c["F"][sl].reshape(-1, 3, 5))
        return r.oe_step_full(jac, (c["kind"], c["row"]), c["y"][sl].reshape(-1, 3, 5), c["x"][sl], c["xa"][sl], c["Sa"][sl], c["Se"][0], gamma[sl],
                              want=WANT)

    whole = host(multi, slice(None))
    multi.close()
    assert np.all(whole["status"] == 0) and np.all(whole["dofs"] > 0)
    per = -(-nprof // 3)
    for p0 in range(0, nprof, per):
        sl = slice(p0, min(nprof, p0 + per))
        same_bits({k: v[sl] for k, v in whole.items()}, host(rt, sl), ALL)
    devout, _ = run(db, c, gamma)
    same_bits(whole, devout, ALL)
    with pytest.raises(api.MonoRTMError) as e:
        rt.oe_step_full(dict(c["ka"], y=c["F"].reshape(-1, 3, 5)), (c["kind"] + 5, c["row"]), c["y"].reshape(-1, 3, 5), c["x"], c["xa"], c["Sa"], c["Se"][0])
    assert e.value.code == EARG
