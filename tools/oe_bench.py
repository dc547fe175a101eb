"""Time of the optimal-estimation step (monortm_hip_oe_step_dev) on the configs[3] shape
(bench.build_workload("c4"): 1024 profiles x 64 layers x 50 channels x 500 lines, f64), against what surrounds and what replaces it.

    python tools/oe_bench.py [--calls 20] [--warmup 3] [--full | --lm] [--out FILE]

Operators of 14 channels (the 50 wavenumbers in runs of 3 or 4) and 1 or 6 views of 4 paths: m = 14 and 84 measurements.  States:
n = 64 (T of every layer), 130 (T, ln H2O, TMPSFC, EMISS), 200 (T, TZ, ln H2O, 4 layers of CLW, TMPSFC, EMISS, REFLC).  Sa is
sigma^2 exp(-|i - j| / 4) within each variable, se = 0.25, x = xa + a draw, y_obs = Y + noise; K is what DeviceBatch.obs_jacobian leaves.
Per m, device-event times of the variants, one of each in turn (interleaved, after warm-up):
  a      DeviceBatch.obs_jacobian, njac = 1: the call that produces K - what an iteration costs anyway;
  k<n>   DeviceBatch.oe_step: one launch of oe_kernel.hip, K read in place;
  t<n>   the same algebra in torch: K gathered dense (cat + index), matmul, torch.linalg.cholesky and one cholesky_solve of
         [W^T | r], which gives z and the diagnostics (W_i . M^-1 W_i, K_i . M^-1 W_i).  A variant the libraries refuse (a failed
         workspace allocation has been seen) is dropped and its error recorded.
With --full (monortm_hip_oe_step_full_dev; Se = 0.25 exp(-|j - j'| / 1.5), one matrix for the batch) also
  f<n>   DeviceBatch.oe_step_full with the variances se and nothing wanted: the launch of k<n> through the other entry;
  s<n>   the full Se, nothing wanted: the second Cholesky and M's off-diagonals;
  c<n>   the full Se + avk + post_cov + dofs: the second launch, oe_cov_kernel;
  g<n>   the full Se + avk + post_cov + dofs + gain_t: the back substitution on top;
  u<n>   the algebra of c<n> in torch on a gathered K: cholesky, cholesky_solve of W^T, and the two matmul that form A and S_hat.
With --lm (DeviceBatch.retrieve_lm) nothing of the above: per m and n, on two batches of the same profiles,
  r<n>   one iteration of DeviceBatch.retrieve (gammas = (0,)): obs_jacobian, oe_step, the write-back in torch ops;
  l<n>   one DeviceBatch.lm_iterate: obs_jacobian, oe_step_lm, scatter, obs, accept, scatter.
The states are those retrieve can write back: n = 64 (T), 130 (T, ln H2O, one layer of CLW, TMPSFC), 200 (T, TZ, ln H2O, 6 layers of CLW,
TMPSFC); xa is what the batch holds, y_obs the forward model there plus noise, so that every iterate stays physical.  Before every
timed call the loop is restarted at xa (lm_start, outside the events): what is timed is the first iteration, in which all 1024 profiles
are live; done_n<n> and accepted_rejected_n<n> record the state after the last one.
Median / min / max / IQR of each, the largest difference of x_new between k and t relative to max |x_new - x|, and the number of
profiles with status 1.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCHAN = 14


def stats(ms):
    a = np.asarray(ms)
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()), iqr=float(q3 - q1), n=len(a))


def specs(lm):
    L = range(lm)
    return {64: [("t", L)],
            130: [("t", L), ("w", "H2O", L), ("tmpsfc",), ("emiss",)],
            200: [("t", L), ("tz", range(lm + 1)), ("w", "H2O", L), ("clw", range(4)), ("tmpsfc",), ("emiss",), ("reflc",)]}


def covariance(spec, rng):
    """sigma^2 exp(-|i - j| / 4) within each item of the spec."""
    sizes = [len(it[-1]) if len(it) > 1 else 1 for it in spec]
    n = sum(sizes)
    Sa, o = np.zeros((n, n)), 0
    for s in sizes:
        i = np.arange(s)
        Sa[o:o + s, o:o + s] = rng.uniform(0.3, 3.0) ** 2 * np.exp(-np.abs(i[:, None] - i[None, :]) / 4.0)
        o += s
    return Sa


def torch_step(torch, jac, rowidx, y_obs, x, xa, Sa, se, gam):
    kall = torch.cat([jac["k_t"], jac["k_tz"], jac["k_w"].flatten(2, 3), jac["k_clw"], jac["k_sfc"]], dim=2)
    K = kall[:, :, rowidx, :].permute(0, 1, 3, 2).reshape(x.shape[0], -1, x.shape[1])        # [nprof][m][n]
    g = (1.0 / (1.0 + gam))[:, None]
    d = (xa - x) * g
    W = torch.matmul(Sa, K.transpose(1, 2)) * g[:, :, None]
    M = torch.matmul(K, W) + torch.diag(se)
    L = torch.linalg.cholesky(M)
    dy = (y_obs - jac["y"]).reshape(x.shape[0], -1)
    r = dy - torch.matmul(K, d[:, :, None])[:, :, 0]
    G = torch.cholesky_solve(torch.cat([W.transpose(1, 2), r[:, :, None]], dim=2), L)      # M^-1 [W^T | r]
    Wt, z = G[:, :, :-1], G[:, :, -1:]
    return dict(x_new=x + d + torch.matmul(W, z)[:, :, 0], post_var=torch.diagonal(Sa)[None, :] * g - (W.transpose(1, 2) * Wt).sum(1),
                avk_diag=(K * Wt).sum(1), chi2=(dy * dy / se).sum(1))


def torch_full(torch, jac, rowidx, x, Sa, Se, gam):
    """avk and post_cov as torch forms them: G^T = M^-1 W^T by cholesky_solve, A = G K, S_hat = g Sa - W G^T."""
    kall = torch.cat([jac["k_t"], jac["k_tz"], jac["k_w"].flatten(2, 3), jac["k_clw"], jac["k_sfc"]], dim=2)
    K = kall[:, :, rowidx, :].permute(0, 1, 3, 2).reshape(x.shape[0], -1, x.shape[1])        # [nprof][m][n]
    g = (1.0 / (1.0 + gam))[:, None, None]
    W = torch.matmul(Sa, K.transpose(1, 2)) * g
    L = torch.linalg.cholesky(torch.matmul(K, W) + Se)
    Gt = torch.cholesky_solve(W.transpose(1, 2), L)                                          # [nprof][m][n]
    return dict(avk=torch.matmul(Gt.transpose(1, 2), K), post_cov=Sa[None] * g - torch.matmul(W, Gt))


def run_case(api, rt, profs, nview, calls, warmup, full=False):
    import torch

    db = api.DeviceBatch(rt, profs)
    dev, lm, nprof, nwn = db.dev, db.lm, db.nprof, db.nwn
    npath = 4 * nview
    chan = (np.arange(nwn) * NCHAN // nwn).astype(np.int32)
    wchan = np.array([1.0 / np.sum(chan == c) for c in chan])
    op = api.ObsOperator(np.arange(0, npath + 1, 4), np.full(npath, 0.25), chan, wchan, nchan=NCHAN)
    h = rt.obs_create(op)
    fd = torch.as_tensor(api.plane_parallel_path(np.linspace(0.0, 60.0, npath), lm)).to(dev).unsqueeze(0).expand(nprof, -1, -1).contiguous()
    jac = db.obs_jacobian(fd, h, mols=(1,))
    torch.cuda.synchronize()
    db.check()
    m = nview * NCHAN
    rng = np.random.default_rng(5)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    y_obs = jac["y"] + up(rng.normal(0.0, 0.5, (nprof, nview, NCHAN)))
    se, gam = up(np.full(m, 0.25)), up(np.zeros(nprof))
    jm = np.arange(m)
    Se = up(0.25 * np.exp(-np.abs(jm[:, None] - jm[None, :]) / 1.5))
    rows = np.concatenate([[0], np.cumsum([lm, lm + 1, lm, lm, 3])])      # row offsets of the kinds in the concatenated K (njac = 1)
    cases, variants, held = {}, {"a": lambda: db.obs_jacobian(fd, h, mols=(1,))}, {}
    for n, spec in specs(lm).items():
        kind, row = api.oe_state_map(spec, lm, [1])
        assert len(kind) == n
        Sa = covariance(spec, rng)
        xa = rng.normal(0.0, 1.0, (nprof, n))
        x = xa + 0.3 * rng.normal(size=(nprof, n)) @ np.linalg.cholesky(Sa).T
        c = dict(state=(kind, row), rowidx=up(rows[kind] + row), Sa=up(Sa), xa=up(xa), x=up(x))
        cases[n] = c
        variants[f"k{n}"] = lambda c=c, n=n: held.__setitem__(f"k{n}", db.oe_step(jac, c["state"], y_obs, c["x"], c["xa"], c["Sa"], se, gamma=gam))
        variants[f"t{n}"] = lambda c=c, n=n: held.__setitem__(f"t{n}", torch_step(torch, jac, c["rowidx"], y_obs, c["x"], c["xa"], c["Sa"], se, gam))
        if full:
            for tag, e, want in (("f", se, ()), ("s", Se, ()), ("c", Se, ("avk", "post_cov", "dofs")), ("g", Se, ("avk", "post_cov", "dofs", "gain_t"))):
                variants[f"{tag}{n}"] = lambda c=c, n=n, tag=tag, e=e, want=want: held.__setitem__(
                    f"{tag}{n}", db.oe_step_full(jac, c["state"], y_obs, c["x"], c["xa"], c["Sa"], e, gamma=gam, want=want))
            variants[f"u{n}"] = lambda c=c, n=n: held.__setitem__(f"u{n}", torch_full(torch, jac, c["rowidx"], c["x"], c["Sa"], Se, gam))
    refused = {}
    for k in list(variants):
        try:
            variants[k]()
            torch.cuda.synchronize()
        except RuntimeError as e:
            refused[k] = str(e).splitlines()[0][:300]
            del variants[k]
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    db.check()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)] for k in variants}
    for i in range(calls):
        for k, f in variants.items():
            a, b = ev[k][i]
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    db.check()
    res = dict(nprof=nprof, nlay=lm, nwn=nwn, npath=npath, nview=nview, nchan=NCHAN, nmeas=m, refused=refused)
    names = dict(a="obs_jacobian_njac1_ms", k="oe_step_ms_n", t="torch_ms_n", f="full_variances_ms_n", s="full_se_ms_n", c="full_se_avk_cov_ms_n",
                 g="full_se_avk_cov_gain_ms_n", u="torch_avk_cov_ms_n")
    for k in variants:
        res[names[k[0]] + k[1:]] = stats([a.elapsed_time(b) for a, b in ev[k]])
    for n, c in cases.items():
        f = variants[f"k{n}"]
        f()       # (the cached outputs hold the last shape's values only while it is the last to run)
        k, t = held[f"k{n}"], held.get(f"t{n}")
        if t is not None:
            scale = float((k["x_new"] - c["x"]).abs().max().item())
            res[f"rel_diff_x_new_n{n}"] = float((k["x_new"] - t["x_new"]).abs().max().item()) / scale
            res[f"max_diff_post_var_n{n}"] = float((k["post_var"] - t["post_var"]).abs().max().item())
        res[f"failed_profiles_n{n}"] = int(k["status"].sum().item())
        res[f"workspace_bytes_n{n}"] = nprof * 2 * m * n * 8
        if full and f"c{n}" in variants:
            variants[f"c{n}"]()
            cg, u = held[f"c{n}"], held.get(f"u{n}")
            if u is not None:
                res[f"max_diff_avk_n{n}"] = float((cg["avk"] - u["avk"]).abs().max().item())
                res[f"rel_diff_post_cov_n{n}"] = float((cg["post_cov"] - u["post_cov"]).abs().max().item()) / float(c["Sa"].diagonal().max().item())
            res[f"failed_profiles_full_n{n}"] = int(cg["status"].sum().item())
            res[f"matrix_bytes_n{n}"] = nprof * n * n * 8
    torch.cuda.synchronize()
    rt.obs_destroy(h)
    return res


def lm_specs(lm):
    L = range(lm)
    return {64: [("t", L)],
            130: [("t", L), ("w", "H2O", L), ("clw", [0]), ("tmpsfc",)],
            200: [("t", L), ("tz", range(lm + 1)), ("w", "H2O", L), ("clw", range(6)), ("tmpsfc",)]}


def run_lm_case(api, rt, profs, nview, calls, warmup):
    """One iteration of the adaptive loop against one iteration of retrieve, interleaved, device events."""
    import torch

    dbr, dbl = api.DeviceBatch(rt, profs), api.DeviceBatch(rt, profs)
    dev, lm, nprof, nwn = dbl.dev, dbl.lm, dbl.nprof, dbl.nwn
    npath = 4 * nview
    chan = (np.arange(nwn) * NCHAN // nwn).astype(np.int32)
    wchan = np.array([1.0 / np.sum(chan == c) for c in chan])
    op = api.ObsOperator(np.arange(0, npath + 1, 4), np.full(npath, 0.25), chan, wchan, nchan=NCHAN)
    h = rt.obs_create(op)
    fd = torch.as_tensor(api.plane_parallel_path(np.linspace(0.0, 60.0, npath), lm)).to(dev).unsqueeze(0).expand(nprof, -1, -1).contiguous()
    m = nview * NCHAN
    rng = np.random.default_rng(5)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    y_obs = dbl.obs(fd, h).clone() + up(rng.normal(0.0, 0.5, (nprof, nview, NCHAN)))
    se = up(np.full(m, 0.25))
    sigma = dict(t=1.0, tz=1.0, w=0.1, clw=1e-4, tmpsfc=1.0)
    res = dict(nprof=nprof, nlay=lm, nwn=nwn, npath=npath, nview=nview, nchan=NCHAN, nmeas=m)
    for n, spec in lm_specs(lm).items():
        items = api._oe_items(spec, lm)
        assert len(items) == n
        Sa, o = np.zeros((n, n)), 0
        for it in spec:
            sz = len(it[-1]) if len(it) > 1 else 1
            i = np.arange(sz)
            Sa[o:o + sz, o:o + sz] = sigma[it[0]] ** 2 * np.exp(-np.abs(i[:, None] - i[None, :]) / 4.0)
            o += sz
        res_of = dict(t=dbl.T, tz=dbl.TZ, clw=dbl.CLW)
        xa = torch.stack([dbl.tmpsfc0 if name == "tmpsfc" else torch.log(dbl.WKL[:, k, code - 1]) if name == "w" else res_of[name][:, k]
                          for name, code, k in items], dim=1).contiguous()
        Sa = up(Sa)
        # the loop is restarted at xa before every timed iteration, outside the events: every profile is live in what is timed (the
        # decision kernel of a finished profile returns at its first load, and its scatter takes the fallback path)
        start = lambda: dbl.lm_start(y_obs, fd, h, spec, xa, Sa, se=se)  # noqa: E731
        L = start()
        variants = {f"r{n}": lambda spec=spec, xa=xa, Sa=Sa: dbr.retrieve(y_obs, fd, h, spec, xa, Sa, se, gammas=(0,)),
                    f"l{n}": lambda L=L: dbl.lm_iterate(L, first=True)}
        for _ in range(warmup):
            for f in variants.values():
                start()
                f()
        torch.cuda.synchronize()
        dbr.check()
        dbl.check()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)] for k in variants}
        for i in range(calls):
            for k, f in variants.items():
                start()
                a, b = ev[k][i]
                a.record()
                f()
                b.record()
        torch.cuda.synchronize()
        dbr.check()
        dbl.check()
        res[f"retrieve_iteration_ms_n{n}"] = stats([a.elapsed_time(b) for a, b in ev[f"r{n}"]])
        res[f"lm_iteration_ms_n{n}"] = stats([a.elapsed_time(b) for a, b in ev[f"l{n}"]])
        res[f"done_n{n}"] = {str(k): int(v) for k, v in zip(*np.unique(L["done"].cpu().numpy(), return_counts=True))}
        res[f"accepted_rejected_n{n}"] = [int(L["n_acc"].sum().item()), int(L["n_rej"].sum().item())]
    rt.obs_destroy(h)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", default="1,6")
    ap.add_argument("--full", action="store_true", help="also time DeviceBatch.oe_step_full and the torch route to avk and post_cov")
    ap.add_argument("--lm", action="store_true", help="time one DeviceBatch.lm_iterate against one iteration of DeviceBatch.retrieve instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    from monortm_amd import api, tape3

    if not torch.cuda.is_available():
        raise SystemExit("oe_bench needs the GPU (no CPU fallback)")
    rec, profs, desc, _rk, _t3kw = bench.build_workload("c4", 0, 128)
    wn = profs[0].wn
    res = dict(what="DeviceBatch.oe_step (k) vs DeviceBatch.obs_jacobian, njac = 1 (a) vs the same algebra in torch on a gathered K (t), device events",
               workload=desc, cases={})
    with tempfile.TemporaryDirectory() as d:
        t3 = os.path.join(d, "TAPE3")
        tape3.write_tape3(t3, rec)
        rt = api.MonoRTM(t3, wn[0], wn[-1], device=0)
        for nview in (int(v) for v in args.views.split(",")):
            if args.lm:
                res["what"] = "one DeviceBatch.lm_iterate (l) vs one iteration of DeviceBatch.retrieve (r), interleaved, device events"
                res["cases"][str(nview * NCHAN)] = run_lm_case(api, rt, profs, nview, args.calls, args.warmup)
            else:
                res["cases"][str(nview * NCHAN)] = run_case(api, rt, profs, nview, args.calls, args.warmup, args.full)
            torch.cuda.empty_cache()
        rt.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
