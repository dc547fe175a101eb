"""DeviceBatch.retrieve_lm on the set-up of tests/test_oe_retrieve.py, rebuilt here: the line list and channels
of tests/test_obs_jacobian.py::case, the operator of views "A" with the comb map (3 views x 10 channels = 30 measurements), three
profiles of 12, 9 and 10 layers, the state T and ln H2O of every layer and TMPSFC (n = 25); y_obs is DeviceBatch.obs at the prior plus a
smooth perturbation.

Profile 0 and 2 run freely from gamma 0.  Profile 1 has a box of xa +- 0.05 K on its temperature columns: its undamped first step (a few K)
leaves the box - asserted in long double from the kept K, Y and x - and must be rejected with the batch restored.

Every decision of the device is replayed through oe_lm_truth.accept from the kept records, with J_trial recomputed in long double; the
replay first asserts that no decision rests on rounding (|J_trial - J_cur| > 1e-9 J_cur wherever the two are compared)."""
import dataclasses

import numpy as np
import pytest

import obs_cases as oc
import oe_lm_truth as lt
from monortm_amd import api, synth, tape3
from test_oe_step import bits, gather

pytestmark = pytest.mark.gpu

NLAY = (12, 9, 10)
MAXIT = 8
BOX = 0.05
RES = ("T", "TZ", "WKL", "CLW", "tmpsfc")


@pytest.fixture(scope="module")
def setup(workdir):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    t3 = f"{workdir}/TAPE3_oe_lm_retrieve"
    tape3.write_tape3(t3, synth.synthetic_lines(300, seed=777, lc_frac=0.5, sdep_frac=0.2))
    wn = np.unique(np.concatenate([synth.c2_channels(12, seed=11), synth.sounder_channels()]))
    rt = api.MonoRTM(t3, wn[0], wn[-1])
    prior = [synth.perturbed_profile(450 + i, wn, nlay=n, cloud=False, irt=1) for i, n in enumerate(NLAY)]
    truth = []
    for p in prior:
        u = (np.arange(p.nlay) + 0.5) / p.nlay
        wkl = p.wkl.copy()
        wkl[:, 0] *= np.exp(0.45 * np.cos(2.0 * u))
        truth.append(dataclasses.replace(p, t=p.t + 6.0 * np.sin(3.0 * u), wkl=wkl, tmpsfc=p.tmpsfc + 4.5))
    op = oc.operator("A", "comb", len(wn), mixed=False)
    h = rt.obs_create(op)
    lm = max(NLAY)
    path = torch.as_tensor(oc.factors(9)[:, None] * np.ones(lm)[None, :]).cuda()
    y_obs = api.DeviceBatch(rt, truth).obs(path, h).clone()
    spec = [("t", range(lm)), ("w", "H2O", range(lm)), ("tmpsfc",)]
    n = 2 * lm + 1
    xa = np.zeros((3, n))
    for i, p in enumerate(prior):
        xa[i, : p.nlay], xa[i, lm: lm + p.nlay], xa[i, -1] = p.t, np.log(p.wkl[:, 0]), p.tmpsfc
    k = np.arange(lm)
    corr = np.exp(-np.abs(k[:, None] - k[None, :]) / 3.0)
    Sa = np.zeros((n, n))
    Sa[:lm, :lm], Sa[lm: 2 * lm, lm: 2 * lm], Sa[-1, -1] = 9.0 * corr, 0.04 * corr, 9.0
    se = np.ones(op.nview * op.nchan)
    lo, hi = np.full((3, n), -np.inf), np.full((3, n), np.inf)
    lo[1, :lm], hi[1, :lm] = xa[1, :lm] - BOX, xa[1, :lm] + BOX
    dev = lambda a: torch.as_tensor(a).cuda()  # noqa: E731
    s = dict(rt=rt, prior=prior, h=h, op=op, path=path, y_obs=y_obs, spec=spec, xa=xa, Sa=Sa, se=se, lm=lm, n=n, lo=lo, hi=hi,
             args=(y_obs, path, h, spec, dev(xa), dev(Sa)), kw=dict(se=dev(se), lo=dev(lo), hi=dev(hi)))
    yield s
    rt.close()


@pytest.fixture(scope="module")
def retrieved(setup):
    """One retrieve_lm with keep, shared by the tests below (none of them changes it), and the batch arrays lm_start leaves."""
    import torch

    s = setup
    db = api.DeviceBatch(s["rt"], s["prior"])
    out = db.retrieve_lm(*s["args"], maxit=MAXIT, keep=True, diagnostics=("dofs",), **s["kw"])
    torch.cuda.synchronize()
    db.check()
    db0 = api.DeviceBatch(s["rt"], s["prior"])
    db0.lm_start(*s["args"], **s["kw"])
    torch.cuda.synchronize()
    start = {k: getattr(db0, k).cpu().numpy() for k in RES}
    npy = lambda d: {k: v.cpu().numpy() for k, v in d.items()}  # noqa: E731
    return db, {k: v.cpu().numpy() for k, v in out.items() if k != "kept"}, [npy(k) for k in out["kept"]], start


def test_first_step_of_the_boxed_profile_is_rejected_and_the_batch_restored(setup, retrieved):
    s = setup
    lm = s["lm"]
    _, out, kept, start = retrieved
    k0 = kept[0]
    kind, row = api.oe_state_map(s["spec"], lm, [1])
    K = gather(k0, kind, row)
    y = s["y_obs"].cpu().numpy().reshape(3, -1)
    assert np.array_equal(k0["x"], s["xa"]) and np.all(k0["c"] == 0) and np.all(k0["gamma"] == 0) and np.all(k0["done"] == 0)
    t = lt.step_lm(K[1], s["Sa"], s["se"], s["xa"][1], k0["x"][1], y[1], k0["y"][1].reshape(-1), 0.0, k0["c"][1])
    leave = float(np.max(np.abs(t["x_new"][: NLAY[1]] - s["xa"][1, : NLAY[1]])))
    print(f"profile 1, iteration 0: the undamped step moves a temperature by {leave:.3g} K (box {BOX} K)")
    assert leave > 2 * BOX                                               # in long double: the step leaves the box
    assert k0["trial_ok"].tolist() == [1, 0, 1] and k0["n_rej"][1] == 1 and k0["n_acc"][1] == 0 and k0["gamma_after"][1] == 1.0
    assert np.array_equal(bits(k0["x_after"][1]), bits(s["xa"][1])) and k0["J_after"][1] == k0["J"][1]
    for k in RES:                                                        # after step 6 the batch is what it was before the iteration
        assert np.array_equal(bits(k0[k][1]), bits(start[k][1])), k
    assert not np.array_equal(k0["T"][0], start["T"][0])                 # (profile 0 moved)


def test_every_decision_replays_through_the_truth(setup, retrieved):
    s = setup
    _, out, kept, _ = retrieved
    y = s["y_obs"].cpu().numpy().reshape(3, -1)
    m = y.shape[1]
    acc, rej = np.zeros(3, int), np.zeros(3, int)
    for it, k in enumerate(kept):
        for p in range(3):
            st = dict(x=k["x"][p], c=k["c"][p], J=k["J"][p], gamma=k["gamma"][p], done=int(k["done"][p]), n_acc=acc[p], n_rej=rej[p])
            Jt = lt.cost_of(k["y_trial"][p].reshape(-1), y[p], s["se"], k["c_new"][p], k["x_new"][p], s["xa"][p])
            if st["done"] == 0 and k["status"][p] == 0 and k["trial_ok"][p]:
                assert abs(Jt - st["J"]) > 1e-9 * st["J"], (it, p)      # no decision rests on rounding
            new = lt.accept(st, k["x_new"][p], k["c_new"][p], Jt, bool(k["trial_ok"][p]), int(k["status"][p]), m, last=it + 1 == MAXIT)
            got = (int(k["done_after"][p]), int(k["n_acc"][p]), int(k["n_rej"][p]), float(k["gamma_after"][p]))
            assert got == (new["done"], new["n_acc"], new["n_rej"], float(new["gamma"])), (it, p)
            assert np.array_equal(bits(k["x_after"][p]), bits(np.asarray(new["x"], np.float64))), (it, p)
            if new["n_acc"] > st["n_acc"]:
                assert abs(lt.LD(k["J_after"][p]) - Jt) <= 1e-12 * Jt
            acc[p], rej[p] = new["n_acc"], new["n_rej"]
        if it:
            for key, prev in (("x", "x_after"), ("gamma", "gamma_after"), ("done", "done_after"), ("J", "J_after")):
                assert np.array_equal(bits(k[key]), bits(kept[it - 1][prev])), key
    print("done", out["done"], "n_acc", out["n_acc"], "n_rej", out["n_rej"], "gamma", out["gamma"])
    assert np.array_equal(out["n_acc"], acc) and np.array_equal(out["n_rej"], rej) and np.all(out["done"] != 0)
    assert out["n_acc"][0] >= 1 and out["n_acc"][2] >= 1                 # the free profiles descend


def test_cost_never_rises_and_finished_profiles_rest(setup, retrieved):
    s = setup
    lm = s["lm"]
    db, out, kept, start = retrieved
    hist = out["J_history"]
    print("J_history [iteration][profile]:\n" + np.array2string(hist, precision=6))
    assert hist.shape == (MAXIT + 1, 3) and np.all(np.diff(hist, axis=0) <= 0) and np.all(hist[-1, [0, 2]] < hist[0, [0, 2]])
    assert np.array_equal(hist[0], kept[0]["cost"]) and np.array_equal(hist[-1], out["J"])
    for p in range(3):
        fin = [it for it, k in enumerate(kept) if k["done_after"][p] != 0]
        for it in fin[1:]:
            assert np.array_equal(bits(kept[it]["x_after"][p]), bits(kept[fin[0]]["x_after"][p]))
            for k in RES:
                assert np.array_equal(bits(kept[it][k][p]), bits(kept[fin[0]][k][p])), (k, p, it)
    # the batch holds x
    x = out["x"]
    T, W = db.T.cpu().numpy(), db.WKL.cpu().numpy()
    assert np.array_equal(db.tmpsfc.cpu().numpy(), x[:, -1]) and np.array_equal(db.tmpsfc0.cpu().numpy(), x[:, -1])
    for p, nl in enumerate(NLAY):
        assert np.array_equal(bits(T[p, :nl]), bits(x[p, :nl]))
        want = np.exp(x[p, lm: lm + nl])
        assert np.all(np.abs(W[p, :nl, 0] - want) <= 4 * np.spacing(want))
        for k in ("T", "WKL"):                                           # padded layers are never written (their states do move: Sa couples them)
            assert np.array_equal(bits(getattr(db, k)[p, nl:].cpu().numpy()), bits(start[k][p, nl:])), k
    assert np.all(np.abs(x[1, : NLAY[1]] - s["xa"][1, : NLAY[1]]) <= BOX)  # the boxed profile stayed inside
    assert out["status"].tolist() == [0, 0, 0] and np.all(out["post_var"][:, : NLAY[1]] > 0) and np.all(out["dofs"] > 0)


def test_a_captured_iteration_replays_the_eager_bits(setup):
    """Two batches from the same state, one warm iteration each; the second iteration eager on one, captured and replayed on the other."""
    import torch

    s = setup
    dbs = [api.DeviceBatch(s["rt"], s["prior"]) for _ in range(2)]
    Ls = []
    for db in dbs:
        L = db.lm_start(*s["args"], **s["kw"])
        db.lm_iterate(L, first=True)
        Ls.append(L)
    torch.cuda.synchronize()
    dbs[0].lm_iterate(Ls[0])
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            dbs[1].lm_iterate(Ls[1])
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert torch.equal(Ls[1]["n_acc"] + Ls[1]["n_rej"], torch.ones_like(Ls[1]["n_acc"]))     # the capture itself ran nothing
    g.replay()
    torch.cuda.synchronize()
    for db in dbs:
        db.check()
    assert torch.equal(Ls[0]["n_acc"] + Ls[0]["n_rej"], torch.full_like(Ls[0]["n_acc"], 2))
    for k in ("x_cur", "c_cur", "J_cur", "gamma", "done", "n_acc", "n_rej", "trial_ok"):
        assert np.array_equal(bits(Ls[0][k].cpu().numpy()), bits(Ls[1][k].cpu().numpy())), k
    for k in RES:
        assert np.array_equal(bits(getattr(dbs[0], k).cpu().numpy()), bits(getattr(dbs[1], k).cpu().numpy())), k
    # a warm iteration allocates nothing through torch (the caching allocator's count; the library's own hipMalloc of its workspace and
    # maps is outside it - those are sized by the first call of a shape and map, which the header states and the capture above relies on)
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    dbs[0].lm_iterate(Ls[0])
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before


def test_refusals(setup):
    import torch

    s = setup
    db = api.DeviceBatch(s["rt"], s["prior"])
    T0 = db.T.clone()
    with pytest.raises(ValueError, match="x0 needs c0"):
        db.retrieve_lm(*s["args"], x0=s["args"][4].clone(), **s["kw"])
    for spec in ([("t", range(s["lm"])), ("emiss",)], [("reflc",)], [("w", "p", [0])], [("w", "xself", [0])]):
        n = len(api._oe_items(spec, s["lm"]))
        z = torch.zeros(3, n, dtype=torch.float64).cuda()
        with pytest.raises(ValueError):
            db.retrieve_lm(s["y_obs"], s["path"], s["h"], spec, z, torch.eye(n, dtype=torch.float64).cuda(), se=s["kw"]["se"])
    assert torch.equal(db.T, T0)


def test_start_from_x0_with_its_dual_vector(setup, retrieved):
    """Restarting at the retrieved x with c0 = Sa^-1 (x - xa): the first cost is the final cost of the run that got there, to rounding."""
    import torch

    s = setup
    _, out, _, _ = retrieved
    c0 = np.linalg.solve(s["Sa"], (out["x"] - s["xa"]).T).T
    db = api.DeviceBatch(s["rt"], s["prior"])
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    r = db.retrieve_lm(*s["args"], maxit=1, x0=dev(out["x"]), c0=dev(c0), **s["kw"])
    torch.cuda.synchronize()
    db.check()
    J0 = r["J_history"][0].cpu().numpy()
    print("restart: first cost", J0, "final cost before", out["J"])
    assert np.allclose(J0, out["J"], rtol=1e-9, atol=0)
