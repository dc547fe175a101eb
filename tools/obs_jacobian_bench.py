"""Time of the channel- and beam-averaged Jacobians against what the API offered before them, on the configs[3] shape
(bench.build_workload("c4"): 1024 profiles x 64 layers x 50 channels x 500 lines, f64), njac = 1 (LABNOTES).

    python tools/obs_jacobian_bench.py [--paths 4,16,64] [--calls 20] [--warmup 3] [--only a] [--out FILE]

The operator: the 50 wavenumbers in 10 channels of 5 - channel 1 nested inside channel 0 (their samples interleave), the others
runs of 5 - and views of 4 adjacent paths each, uniform normalised weights.  Per number of paths, device-event times of two variants,
one of each in turn (interleaved, after warm-up):
  a  DeviceBatch.obs_jacobian: the 3 + 2 njac MODM passes once + one rtm_obs_jac launch that contracts as it goes;
  b  DeviceBatch.scan_jacobian (every monochromatic per-path K written out) followed by the contraction in torch with
     ObsOperator.dense(): one einsum per field (y = tb, k_t, k_tz, k_w, k_clw, k_sfc).
Median / min / max / IQR of each, the ratio b / a, the bytes of output tensors each variant holds, and the largest difference between
a and b relative to the largest entry over the layer axis.  --only a|b runs one variant alone.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("y", "k_t", "k_tz", "k_w", "k_clw", "k_sfc")


def stats(ms):
    a = np.asarray(ms)
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()), iqr=float(q3 - q1), n=len(a))


def operator(api, npath, nwn):
    """10 channels of 5 on 50 wavenumbers (in general nwn // 5 channels): channel 0 = samples 0, 2, 4, 6, 8, channel 1 = 1, 3, 5, 7, 9 -
    nested - and channel c >= 2 = samples 5 c .. 5 c + 4; views of 4 adjacent paths."""
    nchan = nwn // 5
    channels = [[0, 2, 4, 6, 8], [1, 3, 5, 7, 9]] + [list(range(5 * c, 5 * c + 5)) for c in range(2, nchan)]
    views = [list(range(v, min(v + 4, npath))) for v in range(0, npath, 4)]
    op, perm = api.ObsOperator.from_sets(views, channels, npath=npath, nwn=nwn)
    assert np.array_equal(perm, np.arange(npath))
    return op


def nbytes(d):
    return int(sum(v.numel() * v.element_size() for v in d.values()))


def run_case(api, rt, profs, npath, calls, warmup, only, mols=(1,)):
    import torch

    db = api.DeviceBatch(rt, profs)
    dev, lm, n, nwn = db.dev, db.lm, db.nprof, db.nwn
    zen = np.linspace(0.0, 75.0, npath)
    fd = torch.as_tensor(api.plane_parallel_path(zen, lm)).to(dev).unsqueeze(0).expand(n, -1, -1).contiguous()   # [nprof, npath, lm]
    op = operator(api, npath, nwn)
    h = rt.obs_create(op)
    W = torch.as_tensor(op.dense().reshape(op.nview, op.nchan, npath, nwn)).to(dev)
    held = {}

    def var_a():
        held["a"] = db.obs_jacobian(fd, h, mols=mols)
        return held["a"]

    def var_b():
        k = db.scan_jacobian(fd, mols=mols)
        held["b_mono"] = k
        out = dict(y=torch.einsum("pji,vcji->pvc", k["tb"], W), k_t=torch.einsum("pjli,vcji->pvlc", k["k_t"], W),
                   k_tz=torch.einsum("pjli,vcji->pvlc", k["k_tz"], W), k_w=torch.einsum("pjlmi,vcji->pvlmc", k["k_w"], W),
                   k_clw=torch.einsum("pjli,vcji->pvlc", k["k_clw"], W), k_sfc=torch.einsum("pjsi,vcji->pvsc", k["k_sfc"], W))
        held["b"] = out
        return out

    variants = {k: v for k, v in (("a", var_a), ("b", var_b)) if only in ("", k)}
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
    res = dict(nprof=n, nlay=lm, nwn=nwn, npath=npath, nview=op.nview, nchan=op.nchan, njac=len(mols))
    t = {k: stats([a.elapsed_time(b) for a, b in ev[k]]) for k in variants}
    names = dict(a="obs_jacobian_ms", b="scan_jacobian_then_contraction_ms")
    for k in variants:
        res[names[k]] = t[k]
    if "a" in held:
        res["a_output_bytes"] = nbytes(held["a"])
    if "b" in held:
        res["b_output_bytes"] = nbytes(held["b_mono"]) + nbytes(held["b"])
    if "a" in t and "b" in t:
        def rel(x, y, axis):
            scale = y.abs().amax(dim=axis, keepdim=True)
            return float(((x - y).abs() / torch.where(scale > 0, scale, torch.ones_like(scale))).max().item())

        res["rel_diff_a_b"] = {k: rel(held["a"][k], held["b"][k], 2 if held["b"][k].dim() > 3 else 1) for k in FIELDS}
        res["finite"] = bool(all(torch.isfinite(v).all().item() for v in held["a"].values()))
        res["b_over_a"] = t["b"]["median"] / t["a"]["median"]
    torch.cuda.synchronize()
    rt.obs_destroy(h)
    return res


def workload():
    """The configs[3] batch of bench.py: line records, the 1024 profiles and the description."""
    import bench

    rec, profs, desc, _rk, _t3kw = bench.build_workload("c4", 0, 128)
    return rec, profs, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default="4,16,64")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", choices=["", "a", "b"])
    args = ap.parse_args()
    import torch

    from monortm_amd import api, tape3

    if not torch.cuda.is_available():
        raise SystemExit("obs_jacobian_bench needs the GPU (no CPU fallback)")
    rec, profs, desc = workload()
    wn = profs[0].wn
    res = dict(what="DeviceBatch.obs_jacobian (a) vs DeviceBatch.scan_jacobian + torch contraction with ObsOperator.dense() (b), device events",
               workload=desc, cases={})
    with tempfile.TemporaryDirectory() as d:
        t3 = os.path.join(d, "TAPE3")
        tape3.write_tape3(t3, rec)
        rt = api.MonoRTM(t3, wn[0], wn[-1], device=0)
        for npath in (int(x) for x in args.paths.split(",")):
            res["cases"][str(npath)] = run_case(api, rt, profs, npath, args.calls, args.warmup, args.only)
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
