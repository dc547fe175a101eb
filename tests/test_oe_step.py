"""The optimal-estimation step on the GPU (monortm_hip_oe_step, monortm_hip_oe_step_dev, oe_kernel.hip) against
the long-double step of tests/oe_truth.py.

K comes from synthetic K_T, K_TZ, K_W (njac = 2), K_CLW and K_SFC arrays in the layout of monortm_hip_obs_jacobian, every row live; the
state map mixes all five kinds in scrambled order, with one state named twice.  Shapes: m = nview x nchan in 1, 3, 64, 65, 128 (one
measurement; fewer than a row block of the solves; the 16-wide blocks of the W pass exactly, plus one; the limit, whose LDS needs the raised
bound), n in 1, 7, 65, 300 (one state; fewer than the 8-wide tiles; tiles plus one; more than the 256 threads of a workgroup), 3 profiles.

Bounds: x_new within 1e-12 of max |x_new - x| of the profile, post_var within 1e-12 of max Sa_ii - eps x cond(M) x 10 for cond(M) < 1e4,
which the generator asserts.  avk_diag: its entries are O(1) (the eigenvalues of the averaging kernel lie in [0, 1)), the same 1e-12
absolute.  chi2: m terms of three roundings each, summed in order: (m + 3) 2^-52 relative."""
import ctypes as C
import os

import numpy as np
import pytest

import oe_truth as ot
from monortm_amd import api, synth

pytestmark = pytest.mark.gpu

NJAC, NPROF = 2, 3
MSHAPES = [(1, 1), (3, 1), (4, 16), (5, 13), (8, 16)]      # (nview, nchan): m = 1, 3, 64, 65, 128
NSTATES = [1, 7, 65, 300]
KEYS = ("k_t", "k_tz", "k_w", "k_clw", "k_sfc")
OUT = ("x_new", "post_var", "avk_diag", "chi2", "status")
EUNSUPPORTED, EARG = 3, 6


@pytest.fixture(scope="module")
def dev():
    """(a context without a line table, a DeviceBatch on it: oe_step reads none of the batch's own arrays)."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    rt = api.MonoRTM("", 0.0, 0.0)
    db = api.DeviceBatch(rt, [synth.perturbed_profile(0, synth.c2_channels(4, seed=1), nlay=3)])
    yield rt, db
    rt.close()


def rows_of(lm):
    return dict(k_t=lm, k_tz=lm + 1, k_w=lm * NJAC, k_clw=lm, k_sfc=3)


def k_arrays(nprof, nview, nchan, lm, rng):
    """Smooth weighting functions along the rows of every kind, one bump per measurement, 5 % noise, another amplitude per profile."""
    out = {}
    for key, R in rows_of(lm).items():
        u = (np.arange(R) + 0.5) / R
        c, w = rng.uniform(0, 1, (nview, 1, nchan)), rng.uniform(0.05, 0.4, (nview, 1, nchan))
        amp = rng.uniform(0.3, 1.5, (nprof, nview, 1, nchan)) * rng.choice([-1.0, 1.0], (1, nview, 1, nchan))
        a = amp * np.exp(-(((u[None, :, None] - c) / w) ** 2))[None] * (1.0 + 0.05 * rng.normal(size=(nprof, nview, R, nchan)))
        out[key] = a.reshape(nprof, nview, lm, NJAC, nchan) if key == "k_w" else a
    return out


def state_map(n, lm, rng):
    """n states: distinct (kind, row) pairs in scrambled order - every kind present once n >= 5 - and, for n >= 2, one of them twice."""
    rows = list(rows_of(lm).values())
    if n == 1:
        return np.array([0], np.int32), np.array([lm - 1], np.int32)
    first = [(k, int(rng.integers(rows[k]))) for k in range(5)][: n - 1]
    rest = [(k, r) for k in range(5) for r in range(rows[k]) if (k, r) not in first]
    pick = first + [rest[i] for i in rng.permutation(len(rest))[: n - 1 - len(first)]]
    pick.append(pick[int(rng.integers(len(pick)))])
    pick = [pick[i] for i in rng.permutation(n)]
    return np.array([k for k, _ in pick], np.int32), np.array([r for _, r in pick], np.int32)


def gather(ka, kind, row):
    """K [nprof][m][n] of the state map, in numpy."""
    cols = []
    for k, r in zip(kind, row):
        a = ka[KEYS[k]]
        a = a.reshape(a.shape[0], a.shape[1], -1, a.shape[-1])
        cols.append(a[:, :, r, :].reshape(a.shape[0], -1))
    return np.stack(cols, axis=2)


def make(nview, nchan, n, seed=0, nprof=NPROF, shared_sa=False, shared_se=False):
    rng = np.random.default_rng(7 + 31 * nview + 1009 * nchan + 17 * n + 7919 * seed)
    lm = max(2, -(-n // 5) + 1)
    ka = k_arrays(nprof, nview, nchan, lm, rng)
    kind, row = state_map(n, lm, rng)
    Sa = np.stack([ot.blocks_cov(n, rng) for _ in range(nprof)])
    if shared_sa:
        Sa[:] = Sa[0]
    c = ot.finish_case(gather(ka, kind, row), Sa, rng, shared_se=shared_se)
    c.update(ka=ka, kind=kind, row=row, lm=lm, nview=nview, nchan=nchan, shared_sa=shared_sa, shared_se=shared_se)
    return c


def run(db, c, gamma=None, sl=slice(None)):
    """DeviceBatch.oe_step on the profiles sl of the case: (outputs as numpy, the device tensors of the call)."""
    import torch

    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(db.dev)  # noqa: E731
    t = {k: up(v[sl]) for k, v in c["ka"].items()}
    t.update(y=up(c["F"][sl].reshape(-1, c["nview"], c["nchan"])), y_obs=up(c["y"][sl].reshape(-1, c["nview"], c["nchan"])), x=up(c["x"][sl]),
             xa=up(c["xa"][sl]), Sa=up(c["Sa"][0] if c["shared_sa"] else c["Sa"][sl]), se=up(c["se"][0] if c["shared_se"] else c["se"][sl]),
             gamma=None if gamma is None else up(np.asarray(gamma, np.float64)[sl]))
    return call(db, c, t), t


def call(db, c, t):
    import torch

    out = db.oe_step(t, (c["kind"], c["row"]), t["y_obs"], t["x"], t["xa"], t["Sa"], t["se"], gamma=t["gamma"])
    torch.cuda.synchronize()
    db.check()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def check_truth(c, got, gamma, what):
    worst = dict(x_new=0.0, post_var=0.0, avk_diag=0.0, chi2=0.0)
    m = c["K"].shape[1]
    for p in range(c["K"].shape[0]):
        g = 0.0 if gamma is None else gamma[p]
        t = ot.step(c["K"][p], c["Sa"][p], c["se"][p], c["xa"][p], c["x"][p], c["y"][p], c["F"][p], g)
        e = {k: np.abs(got[k][p].astype(ot.LD) - t[k]) for k in worst}
        scale = dict(x_new=np.max(np.abs(t["x_new"] - c["x"][p])), post_var=np.max(np.diag(c["Sa"][p])), avk_diag=ot.LD(1), chi2=t["chi2"])
        for k in worst:
            worst[k] = max(worst[k], float(np.max(e[k]) / scale[k]))
        assert got["status"][p] == 0
        assert np.isclose(float(got["dfs"][p]), float(np.sum(t["avk_diag"])), rtol=0, atol=1e-11 * max(1, len(c["kind"])))
    print(f"{what}: worst error / scale " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["x_new"] <= 1e-12 and worst["post_var"] <= 1e-12 and worst["avk_diag"] <= 1e-12 and worst["chi2"] <= (m + 3) * 2.0 ** -52


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b, keys=OUT + ("dfs",)):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


# ---- 1. the numbers, at every seam ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NSTATES)
@pytest.mark.parametrize("nview,nchan", MSHAPES)
def test_step_matches_the_long_double_truth(dev, nview, nchan, n):
    """Per-profile Sa and se with gamma 0 / 10 / 0, then shared Sa and se with gamma NULL."""
    _, db = dev
    gamma = [0.0, 10.0, 0.0]
    c = make(nview, nchan, n)
    got, _ = run(db, c, gamma)
    check_truth(c, got, gamma, f"m {nview * nchan} n {n} per-profile")
    c = make(nview, nchan, n, seed=1, shared_sa=True, shared_se=True)
    got, _ = run(db, c, None)
    check_truth(c, got, None, f"m {nview * nchan} n {n} shared")


def test_upper_triangle_of_sa_is_never_read(dev):
    _, db = dev
    c = make(5, 13, 65)
    ref, _ = run(db, c, None)
    c["Sa"] = np.tril(c["Sa"]) + np.triu(np.full_like(c["Sa"], np.nan), 1)
    got, _ = run(db, c, None)
    same_bits(ref, got)


# ---- 2. the same bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nview,nchan,n", [(5, 13, 300), (8, 16, 65), (3, 1, 7)])
def test_same_bits_repeated_alone_and_replayed(dev, nview, nchan, n):
    """A call repeated; profile 1 alone against profile 1 in the batch; a graph capture replayed after every input changed in place,
    against a plain call on the changed inputs."""
    import torch

    _, db = dev
    gamma = [0.0, 10.0, 0.0]
    c = make(nview, nchan, n)
    a, t = run(db, c, gamma)
    same_bits(a, call(db, c, t))
    alone, _ = run(db, c, gamma, slice(1, 2))
    same_bits({k: v[1:2] for k, v in a.items()}, alone)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = db.oe_step(t, (c["kind"], c["row"]), t["y_obs"], t["x"], t["xa"], t["Sa"], t["se"], gamma=t["gamma"])
    torch.cuda.current_stream().wait_stream(s)
    c2 = make(nview, nchan, n, seed=5)
    c2.update(kind=c["kind"], row=c["row"])   # (the captured call holds the first case's map: K is whatever that map reads)
    c2.update(ot.finish_case(gather(c2["ka"], c["kind"], c["row"]), c2["Sa"], np.random.default_rng(3)))
    _, t2 = run(db, c2, [10.0, 0.0, 2.5])
    for k, v in t.items():
        v.copy_(t2[k])
    for k in OUT:
        out[k].fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    replayed = {k: v.cpu().numpy().copy() for k, v in out.items()}
    assert np.all(replayed["status"] == 0) and not np.array_equal(replayed["x_new"], a["x_new"])
    same_bits(replayed, call(db, c2, t2))
    check_truth(c2, replayed, [10.0, 0.0, 2.5], f"m {nview * nchan} n {n} replayed")


# ---- 3. one profile fails, the batch does not ---------------------------------------------------------------------------------------------
def test_failure_marks_its_profile_only(dev):
    """Profile 1: a negative se that makes M indefinite; profile 2: a NaN in K.  A checked argument: nothing faults, check() stays clean."""
    _, db = dev
    c = make(5, 13, 65)
    solo, _ = run(db, c, None, slice(0, 1))
    lam = float(np.linalg.eigvalsh(c["K"][1] @ c["Sa"][1] @ c["K"][1].T)[-1])
    c["se"][1, 7] = -10.0 * lam
    s = int(np.nonzero(c["kind"] == 0)[0][0])
    c["ka"]["k_t"][2, 3, c["row"][s], 5] = np.nan
    got, t = run(db, c, None)
    assert got["status"].tolist() == [0, 1, 1]
    for p in (1, 2):
        assert np.array_equal(bits(got["x_new"][p]), bits(c["x"][p]))
        assert np.all(got["post_var"][p] == 0) and np.all(got["avk_diag"][p] == 0) and got["chi2"][p] == 0 and got["dfs"][p] == 0
    same_bits({k: v[:1] for k, v in got.items()}, solo)
    # a negative, an infinite and a NaN gamma fail their profile the same way; NaN in x reaches r
    c = make(3, 1, 7)
    got, _ = run(db, c, [-1.0, np.inf, np.nan])
    assert got["status"].tolist() == [1, 1, 1] and np.array_equal(bits(got["x_new"]), bits(c["x"]))
    c["x"][1, 2] = np.nan
    got, _ = run(db, c, None)
    assert got["status"].tolist() == [0, 1, 0]


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def raw(rt, t, c, **over):
    """monortm_hip_oe_step_dev through ctypes; over: sizes, a map, or names of arrays handed over as NULL (drop)."""
    drop = over.get("drop", ())
    d = lambda k: None if k in drop or t.get(k) is None else C.c_void_p(t[k].data_ptr())  # noqa: E731
    kind = np.ascontiguousarray(over.get("kind", c["kind"]), np.int32)
    row = np.ascontiguousarray(over.get("row", c["row"]), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return rt.lib.monortm_hip_oe_step_dev(rt.ctx, NPROF, over.get("nview", c["nview"]), over.get("nchan", c["nchan"]), c["lm"], NJAC,
                                          over.get("nstate", len(kind)), p(kind), p(row), *[d(k) for k in KEYS], d("y"), d("y_obs"), d("x"), d("xa"),
                                          d("Sa"), 1, d("se"), 1, d("gamma"), *[d(k) for k in OUT], None)


def test_refusals_come_before_any_launch(dev):
    import torch

    rt, db = dev
    c = make(5, 13, 7)
    got, t = run(db, c, None)
    t.update({k: torch.full_like(torch.as_tensor(got[k]), -7).to(db.dev) for k in OUT})
    assert raw(rt, t, c) == 0
    torch.cuda.synchronize()
    assert np.array_equal(t["x_new"].cpu().numpy(), got["x_new"])
    t["x_new"].fill_(-7.0)
    k5, rbad = c["kind"].copy(), c["row"].copy()
    k5[3] = 5
    s = int(np.nonzero(c["kind"] == 0)[0][0])
    rbad[s] = c["lm"]                                      # K_T has rows 0 .. lm - 1
    used = KEYS[int(c["kind"][0])]
    for over in (dict(kind=k5), dict(kind=-k5), dict(row=rbad), dict(row=-1 - c["row"]), dict(drop=(used,)), dict(nview=3, nchan=43),
                 dict(nview=0), dict(nstate=0), dict(nstate=2049), dict(drop=("x_new",)), dict(drop=("status",)), dict(drop=("Sa",))):
        assert raw(rt, t, c, **over) == EARG, over
        assert rt.lib.monortm_hip_last_error(rt.ctx)
    torch.cuda.synchronize()
    assert np.all(t["x_new"].cpu().numpy() == -7.0)      # nothing ran
    assert raw(rt, t, c, drop=("post_var", "avk_diag", "chi2", "gamma")) == 0    # the optional ones
    torch.cuda.synchronize()
    assert np.array_equal(t["x_new"].cpu().numpy(), got["x_new"])
    rt4 = api.MonoRTM("", 0.0, 0.0, real_kind=4)
    assert raw(rt4, t, c) == EUNSUPPORTED
    rt4.close()
    with pytest.raises(ValueError):
        db.oe_step(t, (c["kind"], c["row"]), t["y_obs"], t["x"].float(), t["xa"], t["Sa"], t["se"])


# ---- 5. the host entry, sharded ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nprof", [5, 4])
def test_host_entry_sharded_equals_the_block_alone(dev, nprof):
    """MonoRTM.oe_step on a three-shard context (blocks of 2, 2, 1 and 2, 2, 0 profiles) against the one-device host call on each block
    alone, bit for bit, and that against the device entry."""
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
    c = make(3, 5, 7, nprof=nprof, shared_se=True)
    gamma = np.array([0.0, 10.0, 0.0, 1.0, 0.5])[:nprof]

    def host(r, sl):
        jac = dict({k: v[sl] for k, v in c["ka"].items()}, y=c["F"][sl].reshape(-1, 3, 5))
        return r.oe_step(jac, (c["kind"], c["row"]), c["y"][sl].reshape(-1, 3, 5), c["x"][sl], c["xa"][sl], c["Sa"][sl], c["se"][0], gamma[sl])

    whole = host(multi, slice(None))
    multi.close()
    assert np.all(whole["status"] == 0)
    per = -(-nprof // 3)
    for p0 in range(0, nprof, per):
        sl = slice(p0, min(nprof, p0 + per))
        same_bits({k: v[sl] for k, v in whole.items()}, host(rt, sl))
    devout, _ = run(db, c, gamma)
    same_bits(whole, devout, OUT)
    with pytest.raises(api.MonoRTMError) as e:
        rt.oe_step(dict(c["ka"], y=c["F"].reshape(-1, 3, 5)), (c["kind"] + 5, c["row"]), c["y"].reshape(-1, 3, 5), c["x"], c["xa"], c["Sa"], c["se"][0])
    assert e.value.code == EARG
