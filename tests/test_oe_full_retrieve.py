"""DeviceBatch.retrieve with a full Se and the full diagnostics, on the small batch and the damped schedule of
tests/test_oe_retrieve.py: 30 measurements, n = 25, three profiles of 12, 9 and 10 layers.

With Se = diag(se) handed over as a matrix every iteration goes through monortm_hip_oe_step_full_dev with se_kind 1, and x_new keeps
the bits of the diagonal route; the matrices come from the last iteration alone and are held to the long-double step_full on that
iteration's own Y and K under the bounds of tests/test_oe_full.py.  Without the new arguments retrieve is the loop it was."""
import numpy as np
import pytest

import oe_full_truth as oft
from monortm_amd import api
from test_oe_retrieve import GAMMAS, NLAY, setup  # noqa: F401  (the fixture: one context and one y_obs for this module)
from test_oe_step import bits, gather

pytestmark = pytest.mark.gpu

DIAG = ("avk", "post_cov", "dofs")


def retrieve(s, **kw):
    import torch

    db = api.DeviceBatch(s["rt"], s["prior"])
    dev = lambda a: torch.as_tensor(a).to(db.dev)  # noqa: E731
    se = kw.pop("se", None)
    out = db.retrieve(s["y_obs"], s["path"], s["h"], s["spec"], dev(s["xa"]), dev(s["Sa"]), None if se is None else dev(se), gammas=GAMMAS,
                      **{k: dev(v) if k == "Se" else v for k, v in kw.items()})
    torch.cuda.synchronize()
    db.check()
    return db, out


def test_full_se_retrieve_keeps_the_bits_and_adds_the_matrices(setup):  # noqa: F811
    s = setup
    lm, n = s["lm"], s["n"]
    _, ref = retrieve(s, se=s["se"])
    _, out = retrieve(s, Se=np.diag(s["se"]), diagnostics=DIAG, keep=True)
    assert out["status"].tolist() == [0, 0, 0]
    for k in ("x_new", "x", "post_var", "avk_diag"):
        assert np.array_equal(bits(out[k].cpu().numpy()), bits(ref[k].cpu().numpy())), k
    m = len(s["se"])
    c2, c2ref = out["chi2_history"].cpu().numpy(), ref["chi2_history"].cpu().numpy()
    assert np.all(np.abs(c2 - c2ref) <= (m + 3) * 2.0 ** -52 * c2ref)
    assert set(DIAG) <= set(out) and "gain_t" not in out
    assert tuple(out["avk"].shape) == (3, n, n) and tuple(out["post_cov"].shape) == (3, n, n) and tuple(out["dofs"].shape) == (3,)
    # the matrices are the truth's on the last iteration's kept K
    kind, row = api.oe_state_map(s["spec"], lm, [1])
    kp = {k: v.cpu().numpy() for k, v in out["kept"][-1].items()}
    K = gather(kp, kind, row)
    got = {k: out[k].cpu().numpy() for k in DIAG + ("post_var", "avk_diag")}
    for p in range(len(NLAY)):
        y, F = s["y_obs"][p].cpu().numpy().reshape(-1), kp["y"][p].reshape(-1)
        t = oft.step_full(K[p], s["Sa"], np.diag(s["se"]), s["xa"][p], kp["x"][p], y, F, GAMMAS[-1])
        assert np.linalg.cond(np.asarray(t["M"], np.float64)) < 1e4
        ea = float(np.max(np.abs(got["avk"][p].astype(oft.LD) - t["avk"])) / max(oft.LD(1), np.max(np.abs(t["avk"]))))
        es = float(np.max(np.abs(got["post_cov"][p].astype(oft.LD) - t["post_cov"])) / np.max(np.diag(s["Sa"])))
        ed = float(abs(got["dofs"][p] - t["dofs"]))
        print(f"profile {p}: avk {ea:.2e}, post_cov {es:.2e} of max Sa_ii, dofs {float(t['dofs']):.4f} off by {ed:.2e}")
        assert ea <= 1e-12 and es <= 1e-12 and ed <= 1e-11 * n
        assert np.array_equal(bits(np.diag(got["post_cov"][p]).copy()), bits(got["post_var"][p]))
        assert np.array_equal(bits(np.diag(got["avk"][p]).copy()), bits(got["avk_diag"][p]))
        assert np.array_equal(bits(got["post_cov"][p]), bits(got["post_cov"][p].T.copy()))


def test_diagnostics_with_variances_keep_every_bit(setup):  # noqa: F811
    """se as before plus diagnostics: the full entry with se_kind 0 - every output of the diagonal route, chi2 included, bit for bit."""
    s = setup
    _, ref = retrieve(s, se=s["se"])
    _, out = retrieve(s, se=s["se"], diagnostics=("gain_t", "dofs"))
    for k in ("x_new", "x", "post_var", "avk_diag", "chi2", "chi2_history", "status"):
        assert np.array_equal(bits(out[k].cpu().numpy()), bits(ref[k].cpu().numpy())), k
    assert tuple(out["gain_t"].shape) == (3, len(s["se"]), s["n"]) and "avk" not in out
    assert np.allclose(out["dofs"].cpu().numpy(), ref["dfs"].cpu().numpy(), rtol=0, atol=1e-11 * s["n"])


def test_retrieve_without_the_new_arguments_is_the_loop_it_was(setup):  # noqa: F811
    """Against a direct loop of obs_jacobian + oe_step with the write-back of the state (T, ln H2O, TMPSFC), bit for bit."""
    import torch

    s = setup
    lm = s["lm"]
    db, out = retrieve(s, se=s["se"])
    d2 = api.DeviceBatch(s["rt"], s["prior"])
    dev = lambda a: torch.as_tensor(a).to(d2.dev)  # noqa: E731
    xa, Sa, se = dev(s["xa"]), dev(s["Sa"]), dev(s["se"])
    live = torch.arange(lm, device=d2.dev)[None, :] < d2.nlay[:, None]
    x = xa.clone()                                   # the first iterate is what the batch holds
    x[:, :lm] = torch.where(live, d2.T[:, :lm], x[:, :lm])
    x[:, lm: 2 * lm] = torch.where(live, torch.log(d2.WKL[:, :lm, 0]), x[:, lm: 2 * lm])
    x[:, -1] = d2.tmpsfc0
    gam = torch.zeros(3, dtype=torch.float64, device=d2.dev)
    for it, g in enumerate(GAMMAS):
        gam.fill_(g)
        jac = d2.obs_jacobian(s["path"], s["h"], mols=(1,), quantity="tb")
        step = d2.oe_step(jac, s["spec"], s["y_obs"], x, xa, Sa, se, gamma=gam)
        xn = step["x_new"]
        d2.T[:, :lm] = torch.where(live, xn[:, :lm], d2.T[:, :lm])
        d2.WKL[:, :lm, 0] = torch.where(live, torch.exp(xn[:, lm: 2 * lm]), d2.WKL[:, :lm, 0])
        d2.tmpsfc0.copy_(xn[:, -1])
        d2.tmpsfc.copy_(d2.tmpsfc0)
        if it + 1 < len(GAMMAS):
            x.copy_(xn)
    torch.cuda.synchronize()
    for k in ("x_new", "post_var", "avk_diag", "chi2", "status", "dfs"):
        assert np.array_equal(bits(out[k].cpu().numpy()), bits(step[k].cpu().numpy())), k
    assert torch.equal(out["x"], x) and torch.equal(db.T, d2.T) and torch.equal(db.WKL, d2.WKL) and torch.equal(db.tmpsfc, d2.tmpsfc)
    assert set(out) == {"x_new", "post_var", "avk_diag", "dfs", "chi2", "status", "x", "chi2_history"}
