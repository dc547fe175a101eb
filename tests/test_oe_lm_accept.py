"""The decision and the scatter of the adaptive loop on the GPU (monortm_hip_oe_accept_dev, monortm_hip_oe_scatter_dev; DESIGN.md
section 3.15) against tests/oe_lm_truth.py, with a synthetic Y_trial: no forward model runs here.

The decision: one batch with one profile per branch -
  0 accept   1 accept and converge   2 accept, gamma falls through gamma_floor to 0   3 reject from gamma 0 (gamma_first)
  4 reject by trial_ok = 0   5 reject by a NaN J_trial   6 reject past gamma_max   7 step_status 1   8 done already   9 (full Se) a bad Se
run with last = 0 and last = 1, variances and a full Se, m in 1, 65, 128, n in 1, 300.  J_cur of every profile is set from the truth's
J_trial so that |J_trial - J_cur| > 1e-9 J_cur (asserted): no decision rests on rounding, and every integer, gamma and the bits of x_cur
and c_cur must be the truth's.  An accepted J_trial is within 1e-12 relative of the truth (cond(Se) < 1e3 asserted: eps x cond x 10).

The scatter: a three-profile DeviceBatch of 12 / 9 / 10 layers, every case against oe_lm_truth.scatter on copies of the arrays -
everything bit-equal except the WKL it wrote, which is within 4 ulp of exp(x)."""
import numpy as np
import pytest

import oe_lm_truth as lt
from monortm_amd import api, synth
from test_oe_step import EARG, EUNSUPPORTED, bits, dev  # noqa: F401  (dev: the line-table-free context)

pytestmark = pytest.mark.gpu

KN = lt.KNOBS
NB = 10


def decision_case(m, n, full, seed=0, shared=False):
    """shared: one Se for every profile (and no profile with a bad one)."""
    rng = np.random.default_rng(100 * m + n + 7 * full + 1009 * seed)
    nprof = NB if full and not shared else NB - 1
    j = np.arange(m)
    if full:
        Se = np.stack([(lambda dh: dh[:, None] * np.exp(-np.abs(j[:, None] - j[None, :]) / rng.uniform(0.5, 2.0)) * dh[None, :])(
            np.sqrt(rng.uniform(0.5, 2.0, m))) for _ in range(nprof)])
        if shared:
            Se[:] = Se[0]
        assert max(np.linalg.cond(S) for S in Se) < 1e3
        noise = np.stack([np.linalg.cholesky(S) @ rng.normal(size=m) for S in Se])
    else:
        Se = rng.uniform(0.5, 2.0, (nprof, m))
        if shared:
            Se[:] = Se[0]
        noise = np.sqrt(Se) * rng.normal(size=(nprof, m))
    y = rng.normal(250.0, 20.0, (nprof, m))
    Yt = y + 3.0 * noise
    xa = rng.normal(0.0, 5.0, (nprof, n))
    xt = xa + rng.normal(size=(nprof, n))
    ct = (xt - xa) * rng.uniform(0.2, 2.0, (nprof, n))
    Jt = np.array([float(lt.cost_of(Yt[p], y[p], Se[p], ct[p], xt[p], xa[p])) for p in range(nprof)])
    J = 2.0 * Jt + m                                      # J_cur far above J_trial: accepted, not converged
    J[1], J[3], J[6] = Jt[1] + 0.5 * KN["conv"] * m, 0.5 * Jt[3], 0.5 * Jt[6]
    assert np.all(np.abs(Jt - J) > 1e-9 * J)
    gamma = np.array([4.0, 4.0, 1.5e-3, 0.0, 4.0, 4.0, 5e7, 4.0, 4.0, 4.0][:nprof])
    ok = np.ones(nprof, np.int32)
    ok[4] = 0
    status = np.zeros(nprof, np.int32)
    status[7] = 1
    done = np.zeros(nprof, np.int32)
    done[8] = 1
    Yt[5, 0] = np.nan
    if nprof == NB:
        Se[9, 0, 0] = -1.0
    return dict(m=m, n=n, full=full, nprof=nprof, Se=Se, y=y, Yt=Yt, xa=xa, xt=xt, ct=ct, J=J, gamma=gamma, ok=ok, status=status, done=done,
                x=xa + 0.1, c=rng.normal(size=(nprof, n)), n_acc=np.arange(nprof, dtype=np.int32), n_rej=np.arange(nprof, dtype=np.int32)[::-1].copy())


def truth(c, last, sl=slice(None), knobs=KN):
    out = []
    for p in range(c["nprof"])[sl]:
        st = dict(x=c["x"][p], c=c["c"][p], J=c["J"][p], gamma=c["gamma"][p], done=int(c["done"][p]), n_acc=int(c["n_acc"][p]), n_rej=int(c["n_rej"][p]))
        bad = p == 9
        Jt = np.nan if bad else lt.cost_of(c["Yt"][p], c["y"][p], c["Se"][p], c["ct"][p], c["xt"][p], c["xa"][p])
        out.append((st, lt.accept(st, c["xt"][p], c["ct"][p], Jt, bool(c["ok"][p]), int(c["status"][p]), c["m"], last=last, se_bad=bad, **knobs)))
    return out


def run(db, c, last, sl=slice(None), shared_se=False, **knobs):
    import torch

    up = lambda a: torch.as_tensor(np.ascontiguousarray(a[sl])).to(db.dev)  # noqa: E731
    loop = dict(x_cur=up(c["x"]), c_cur=up(c["c"]), J_cur=up(c["J"]), gamma=up(c["gamma"]), done=up(c["done"]), n_acc=up(c["n_acc"]), n_rej=up(c["n_rej"]))
    Se = torch.as_tensor(c["Se"][0]).to(db.dev) if shared_se else up(c["Se"])
    db.oe_accept(up(c["Yt"]), up(c["y"]), Se, up(c["xt"]), up(c["ct"]), up(c["xa"]), up(c["status"]), up(c["ok"]), loop, last=last,
                 se_kind=int(c["full"]), **dict(KN, **knobs))
    torch.cuda.synchronize()
    db.check()
    return {k: v.cpu().numpy() for k, v in loop.items()}


def check(c, got, last, sl=slice(None), knobs=KN):
    worst = 0.0
    for i, (st, want) in enumerate(truth(c, last, sl, knobs)):
        for k, key in (("done", "done"), ("n_acc", "n_acc"), ("n_rej", "n_rej")):
            assert int(got[key][i]) == want[k], (i, k)
        assert got["gamma"][i] == float(want["gamma"]), i
        accepted = want["n_acc"] > st["n_acc"]
        assert np.array_equal(bits(got["x_cur"][i]), bits(c["xt"][sl][i] if accepted else c["x"][sl][i])), i
        assert np.array_equal(bits(got["c_cur"][i]), bits(c["ct"][sl][i] if accepted else c["c"][sl][i])), i
        if accepted:
            worst = max(worst, float(abs(lt.LD(got["J_cur"][i]) - want["J"]) / want["J"]))
        else:
            assert bits(got["J_cur"][i: i + 1])[0] == bits(c["J"][sl][i: i + 1])[0], i
    return worst


@pytest.mark.parametrize("full", [False, True], ids=["variances", "full_se"])
@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("m", [1, 65, 128])
def test_every_branch_of_the_decision(dev, m, n, full):
    _, db = dev
    c = decision_case(m, n, full)
    for last in (False, True):
        t = truth(c, last)
        dn = [w["done"] for _, w in t]
        assert dn == ([3, 1, 3, 3, 3, 3, 4, 2, 1, 2] if last else [0, 1, 0, 0, 0, 0, 4, 2, 1, 2])[: c["nprof"]]      # the case is what it says
        assert [float(w["gamma"]) for _, w in t][:7] == [2.0, 2.0, 0.0, 1.0, 40.0, 40.0, 5e8]
        got = run(db, c, last)
        worst = check(c, got, last)
        print(f"m {m} n {n} {'full' if full else 'diag'} last {last}: accepted J_trial within {worst:.2e} of the truth")
        assert worst <= 1e-12
        # a finished profile: nothing of it changed (profile 8); a profile alone: the bits it has in the batch
        alone = run(db, c, last, slice(2, 3))
        for k in got:
            assert np.array_equal(bits(got[k][2:3]), bits(alone[k])), k


def test_shared_se_and_other_knobs(dev):
    _, db = dev
    kn = dict(up=3.0, down=0.25, gamma_first=0.5, gamma_floor=1.5, gamma_max=10.0, conv=1e-4)
    for full in (False, True):
        c = decision_case(65, 7, full, seed=1, shared=True)
        got = run(db, c, False, shared_se=True, **kn)
        assert check(c, got, False, knobs=kn) <= 1e-12
        assert got["gamma"][:5].tolist() == [0.0, 0.0, 0.0, 0.5, 12.0] and got["done"][:5].tolist() == [0, 0, 0, 0, 4]


def test_decision_refusals(dev):
    import torch

    rt, db = dev
    c = decision_case(3, 2, False)
    for kw in (dict(up=0.5), dict(down=1.5), dict(gamma_first=0.0), dict(conv=-1.0), dict(gamma_max=float("nan"))):
        with pytest.raises(api.MonoRTMError) as e:
            run(db, c, False, **kw)
        assert e.value.code == EARG, kw
    rt4 = api.MonoRTM("", 0.0, 0.0, real_kind=4)
    db4 = object.__new__(api.DeviceBatch)
    db4.torch, db4.rt, db4.dev = torch, rt4, db.dev
    with pytest.raises(api.MonoRTMError) as e:
        run(db4, c, False)
    assert e.value.code == EUNSUPPORTED
    rt4.close()
    with pytest.raises(ValueError):
        c["ok"] = c["ok"].astype(np.int64)
        run(db, c, False)


# ---- the scatter --------------------------------------------------------------------------------------------------------------------------
NLAY = (12, 9, 10)
SPEC = [("t", range(12)), ("w", "H2O", range(12)), ("tz", [0, 9, 12]), ("tmpsfc",), ("t", [3])]
KEYS = ("T", "TZ", "WKL", "CLW", "tmpsfc", "tmpsfc0")


@pytest.fixture(scope="module")
def batch(dev):
    rt, _ = dev
    wn = synth.c2_channels(4, seed=1)
    return api.DeviceBatch(rt, [synth.perturbed_profile(20 + i, wn, nlay=nl) for i, nl in enumerate(NLAY)])


def scatter_both(db, x, fb=None, done=None, lo=None, hi=None):
    """The device scatter and the truth's on the same starting arrays: asserts their agreement, returns trial_ok."""
    import torch

    wmap = api.oe_write_map(SPEC, db.lm, db.nmol)
    before = {k: getattr(db, k).cpu().numpy().copy() for k in KEYS}
    want = {k: v.copy() for k, v in before.items()}
    ok_want = lt.scatter(wmap, np.array(NLAY), want, x, fb, done, lo, hi)
    want["tmpsfc0"] = want["tmpsfc"].copy()
    up = lambda a, dt=None: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dt)).to(db.dev)  # noqa: E731
    ok = torch.full((3,), -1, dtype=torch.int32, device=db.dev)
    db.oe_scatter(wmap, up(x), up(fb), up(done, np.int32), up(lo), up(hi), ok)
    torch.cuda.synchronize()
    db.check()
    got = {k: getattr(db, k).cpu().numpy() for k in KEYS}
    assert ok.cpu().numpy().tolist() == ok_want.tolist()
    for k in KEYS:
        if k != "WKL":
            assert np.array_equal(bits(got[k]), bits(want[k])), k
    same = bits(want["WKL"]) == bits(before["WKL"])                 # what the truth left alone
    assert np.array_equal(bits(got["WKL"])[same], bits(before["WKL"])[same])
    assert np.all(np.abs(got["WKL"] - want["WKL"]) <= 4 * np.spacing(want["WKL"]))
    assert np.array_equal(bits(got["CLW"]), bits(before["CLW"]))    # no column names it
    return ok_want, before, got


def state_of(db, rng):
    """A state vector near what the batch holds: T + noise, ln H2O + noise, TZ, TMPSFC."""
    x = rng.normal(size=(3, 29))
    x[:, :12] += 250.0
    x[:, 12:24] = np.log(1e21) + 0.1 * x[:, 12:24]
    x[:, 24:] += 260.0
    return x


def test_scatter_writes_live_elements_only(batch):
    db = batch
    rng = np.random.default_rng(5)
    x = state_of(db, rng)
    ok, before, got = scatter_both(db, x)
    assert ok.tolist() == [1, 1, 1]
    for p, nl in enumerate(NLAY):
        assert np.array_equal(got["T"][p, :nl], np.where(np.arange(nl) == 3, x[p, 28], x[p, :nl]))       # layer 3 from the last column naming it
        assert np.array_equal(bits(got["T"][p, nl:]), bits(before["T"][p, nl:]))
        assert np.array_equal(bits(got["WKL"][p, nl:]), bits(before["WKL"][p, nl:])) and np.array_equal(bits(got["WKL"][p, :, 1:]), bits(before["WKL"][p, :, 1:]))
        assert not np.any(got["WKL"][p, :nl, 0] == before["WKL"][p, :nl, 0])
    assert np.array_equal(got["TZ"][:, 0], x[:, 24]) and np.array_equal(got["TZ"][:, 9], x[:, 25])
    assert got["TZ"][0, 12] == x[0, 26] and np.array_equal(bits(got["TZ"][1:, 12]), bits(before["TZ"][1:, 12]))
    assert np.array_equal(got["tmpsfc"], x[:, 27]) and np.array_equal(got["tmpsfc0"], x[:, 27])


def test_scatter_box_fallback_and_done(batch):
    db = batch
    rng = np.random.default_rng(6)
    x, fb = state_of(db, rng), state_of(db, rng)
    lo, hi = np.full((3, 29), -np.inf), np.full((3, 29), np.inf)
    hi[1, 4] = x[1, 4] - 0.5                                 # a live layer of profile 1
    ok, _, got = scatter_both(db, x, fb, None, lo, hi)
    assert ok.tolist() == [1, 0, 1] and got["T"][1, 4] == fb[1, 4] and got["T"][0, 4] == x[0, 4]
    hi[1, 4], hi[1, 10], lo[1, 22] = np.inf, x[1, 10] - 0.5, x[1, 22] + 0.5     # layer 10 of a 9-layer profile: padding, T and ln H2O
    ok, _, got = scatter_both(db, x, fb, None, lo, hi)
    assert ok.tolist() == [1, 1, 1] and got["T"][1, 4] == x[1, 4]
    lo[:], hi[:] = -np.inf, np.inf
    lo[2, 3] = x[2, 3] + 0.5                                 # the shadowed column of layer 3 is still checked
    assert scatter_both(db, x, fb, None, lo, hi)[0].tolist() == [1, 1, 0]
    ok, _, got = scatter_both(db, x, fb, np.array([0, 0, 1]))
    assert ok.tolist() == [1, 1, 1] and got["T"][2, 0] == fb[2, 0] and got["T"][1, 0] == x[1, 0]        # a finished profile keeps its iterate
    x2 = x.copy()
    x2[0, 13], x2[2, 26] = np.nan, np.inf                    # live ln H2O of profile 0; level 12 of a 10-layer profile: padding
    assert scatter_both(db, x2, fb)[0].tolist() == [0, 1, 1]
    assert scatter_both(db, x, None, None, lo, hi)[0].tolist() == [1, 1, 0]          # without a fallback the source is written as it is
    # one box for all profiles
    lo1 = np.full(29, -np.inf)
    lo1[27] = np.sort(x[:, 27])[1]                           # TMPSFC: the smallest of the three lies below
    assert scatter_both(db, x, fb, None, lo1, None)[0].tolist() == (x[:, 27] >= lo1[27]).astype(int).tolist()


def test_scatter_refusals(batch):
    import torch

    db = batch
    x = torch.zeros(3, 3, dtype=torch.float64, device=db.dev)
    T0 = db.T.clone()
    i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
    for wmap in ((i32(0, 0, 4), i32(1, 1, 0), i32(0, 0, 0)),          # two written columns on one target
                 (i32(0, 5, 4), i32(1, 2, 0), i32(0, 0, 0)), (i32(0, -2, 4), i32(1, 2, 0), i32(0, 0, 0)),     # kinds outside -1..4
                 (i32(0, 0, 4), i32(1, 12, 0), i32(0, 0, 0)), (i32(1, 0, 4), i32(13, 2, 0), i32(0, 0, 0)),    # a layer, a level outside the array
                 (i32(2, 0, 4), i32(1, 2, 0), i32(db.nmol, 0, 0)), (i32(4, 0, 4), i32(0, 2, 0), i32(0, 0, 0))):
        with pytest.raises(api.MonoRTMError) as e:
            db.oe_scatter(wmap, x)
        assert e.value.code == EARG, wmap
    with pytest.raises(ValueError):
        db.oe_scatter((i32(0, 0, 4), i32(1, 2, 0), i32(0, 0, 0)), x.float())
    with pytest.raises(ValueError):
        db.oe_scatter((i32(0, 0, 4), i32(1, 2, 0), i32(0, 0, 0)), x, lo=np.zeros(3))          # a numpy box
    with pytest.raises(ValueError):
        db.oe_scatter((i32(0, 0, 4), i32(1, 2, 0), i32(0, 0, 0)), x, lo=torch.zeros(3, dtype=torch.float64, device=db.dev),
                      hi=torch.zeros(3, 3, dtype=torch.float64, device=db.dev))
    torch.cuda.synchronize()
    assert torch.equal(db.T, T0)
