"""DeviceBatch.retrieve: obs_jacobian -> oe_step -> write-back, on the line list and channels of
tests/test_obs_jacobian.py::case with the operator of views "A" and the comb map (3 views x 10 channels = 30 measurements) and three
profiles of 12, 9 and 10 layers.  The state is T and ln H2O of every layer and TMPSFC (n = 25); the truth is the prior plus a smooth
perturbation, y_obs is DeviceBatch.obs at the truth.

The bound on x_new is relative to the iteration's largest step, max |x_new - x|, while x_new = x + step carries the rounding of x
itself: half an ulp of a temperature near 250 K is 1.4e-14 K, so no float64 result can stay within 1e-12 of a step below 0.014 K.  On
a noise-free y_obs an undamped iteration gets there at once (gammas 1, 0, 0, 0: steps of 1 K, 0.1 K, 1e-4 K and errors of 2.9e-14,
2.7e-13 and 1.9e-10 of them - the same 2e-14 K each time).  The damping schedule below keeps every iteration's largest step above
STEP_MIN, which the test asserts before it applies the bound."""
import dataclasses

import numpy as np
import pytest

import obs_cases as oc
import oe_truth as ot
from monortm_amd import api, synth, tape3
from test_oe_step import gather

pytestmark = pytest.mark.gpu

NLAY = (12, 9, 10)
GAMMAS = (300.0, 100.0, 30.0)
STEP_MIN = 0.1      # K: 1e-12 of it is 7 times half an ulp of 250 K


@pytest.fixture(scope="module")
def setup(workdir):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    t3 = f"{workdir}/TAPE3_oe_retrieve"
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
    yield dict(rt=rt, prior=prior, h=h, op=op, path=path, y_obs=y_obs, spec=spec, xa=xa, Sa=Sa, se=se, lm=lm, n=n)
    rt.close()


def test_retrieve(setup):
    import torch

    s = setup
    lm, n = s["lm"], s["n"]
    db = api.DeviceBatch(s["rt"], s["prior"])
    before = {k: getattr(db, k).clone() for k in ("T", "WKL", "TZ", "CLW")}
    dev = lambda a: torch.as_tensor(a).to(db.dev)  # noqa: E731
    out = db.retrieve(s["y_obs"], s["path"], s["h"], s["spec"], dev(s["xa"]), dev(s["Sa"]), dev(s["se"]), gammas=GAMMAS, keep=True)
    torch.cuda.synchronize()
    db.check()
    assert out["status"].tolist() == [0, 0, 0] and len(out["kept"]) == len(GAMMAS)
    kind, row = api.oe_state_map(s["spec"], lm, [1])
    # (a) every iteration's step is the long-double step from that iteration's own Y and K
    x_prev = None
    for it, kp in enumerate(out["kept"]):
        ka = {k: v.cpu().numpy() for k, v in kp.items()}
        K = gather(ka, kind, row)
        if x_prev is not None:
            assert np.array_equal(ka["x"], x_prev)          # the iterate is the step before's x_new
        x_prev = ka["x_new"]
        for p in range(3):
            y, F = s["y_obs"][p].cpu().numpy().reshape(-1), ka["y"][p].reshape(-1)
            t = ot.step(K[p], s["Sa"], s["se"], s["xa"][p], ka["x"][p], y, F, GAMMAS[it])
            cond = np.linalg.cond(np.asarray(t["M"], np.float64))
            assert cond < 1e4, cond                           # what the bound below stands on
            step = float(np.max(np.abs(t["x_new"] - ka["x"][p])))
            e = float(np.max(np.abs(ka["x_new"][p].astype(ot.LD) - t["x_new"]))) / step
            print(f"iteration {it} profile {p}: cond(M) {cond:.3g}, max |x_new - x| {step:.3g}, x_new error {e:.2e} of it")
            assert step >= STEP_MIN                           # (the schedule's business, not the kernel's: see the module's docstring)
            assert e <= 1e-12
    assert np.array_equal(out["x_new"].cpu().numpy(), x_prev) and np.array_equal(out["x"].cpu().numpy(), out["kept"][-1]["x"].cpu().numpy())
    # (b) the batch holds the final state; layers >= nlay[p] are untouched
    xn = out["x_new"].cpu().numpy()
    T, W, ts = db.T.cpu().numpy(), db.WKL.cpu().numpy(), db.tmpsfc.cpu().numpy()
    assert np.array_equal(ts, xn[:, -1]) and np.array_equal(db.tmpsfc0.cpu().numpy(), xn[:, -1])
    for p, nl in enumerate(NLAY):
        assert np.array_equal(T[p, :nl], xn[p, :nl])
        want = np.exp(xn[p, lm: lm + nl])
        assert np.all(np.abs(W[p, :nl, 0] - want) <= 4 * np.spacing(want))
        for k in ("T", "WKL", "TZ", "CLW"):
            assert torch.equal(getattr(db, k)[p, nl:], before[k][p, nl:]), k
        assert torch.equal(db.WKL[p, :, 1:], before["WKL"][p, :, 1:])
    assert torch.equal(db.TZ, before["TZ"]) and torch.equal(db.CLW, before["CLW"])
    assert not torch.equal(db.T, before["T"])
    # (c) the cost of the measurements falls
    hist = out["chi2_history"].cpu().numpy()
    print("chi2_history [iteration][profile]:\n" + np.array2string(hist, precision=4))
    assert hist.shape == (len(GAMMAS), 3) and np.all(hist[-1] < hist[0])


def test_retrieve_refuses_what_it_cannot_write_back(setup):
    import torch

    s = setup
    db = api.DeviceBatch(s["rt"], s["prior"])
    dev = lambda a: torch.as_tensor(a).to(db.dev)  # noqa: E731
    T0 = db.T.clone()
    for spec in ([("t", range(s["lm"])), ("emiss",)], [("reflc",)], [("w", "p", [0])], [("w", "xself", [0])]):
        n = len(api._oe_items(spec, s["lm"]))
        with pytest.raises(ValueError):
            db.retrieve(s["y_obs"], s["path"], s["h"], spec, dev(np.zeros((3, n))), dev(np.eye(n)), dev(s["se"]))
    assert torch.equal(db.T, T0)
