"""Time of the Jacobians of a path scan against what the API offered before them, on the configs[3] shape (bench.build_workload("c4"):
1024 profiles x 64 layers x 50 channels x 500 lines, f64), njac = 1 (LABNOTES).

    python tools/scan_jacobian_bench.py [--paths 2,4,8,16] [--calls 20] [--warmup 3] [--only a] [--out FILE]

Per number of paths, device-event times of two variants, one of each in turn (interleaved, after warm-up):
  a  DeviceBatch.scan_jacobian: the 3 + 2 njac MODM passes once + one rtm_scan_jac launch for all paths;
  b  per path: the amounts (WKL, WBRODL, CLW) scaled by the path on the device (three torch multiplies into scratch tensors), then
     monortm_hip_jacobian_dev on them - 3 + 2 njac MODM passes and one adjoint per path.
Median / min / max / IQR of each, the ratio b / a, and the largest difference of K_T and K_W between a and b by the rel_err of
tests/test_jacobian.py.  --only a|b runs one variant alone.  Prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    a = np.asarray(ms)
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()), iqr=float(q3 - q1), n=len(a))


def run_case(api, rt, profs, npath, calls, warmup, only, mols=(1,)):
    import torch

    db = api.DeviceBatch(rt, profs)
    dev, lm, n, nwn = db.dev, db.lm, db.nprof, db.nwn
    zen = np.linspace(0.0, 75.0, npath)
    path = torch.as_tensor(api.plane_parallel_path(zen, lm)).to(dev)                   # [npath, lm]
    fd = path.unsqueeze(0).expand(n, -1, -1).contiguous()                              # [nprof, npath, lm]
    d = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    p0, lib = db.p0, rt.lib
    jm = np.ascontiguousarray(mols, np.int32)
    nj = len(jm)
    # b: scratch amounts of one path at a time and the outputs of monortm_hip_jacobian_dev (one set: every path overwrites it, but
    # K_T and K_W of the last path are kept for the comparison)
    xW, xB, xC = torch.empty_like(db.WKL), torch.empty_like(db.WB), torch.empty_like(db.CLW)
    z = lambda *s: torch.zeros(*s, dtype=db.O.dtype, device=dev)  # noqa: E731
    ob = dict(o=z(n, lm, nwn), rad=z(n, nwn), tb=z(n, nwn), k_t=z(n, lm, nwn), k_tz=z(n, lm + 1, nwn), k_w=z(n, lm, nj, nwn),
              k_clw=z(n, lm, nwn), k_o=z(n, lm, nwn), k_sfc=z(n, 3, nwn))

    def var_a():
        return db.scan_jacobian(fd, mols=mols)

    def var_b():
        sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for j in range(npath):
            torch.mul(db.WKL, path[j][None, :, None], out=xW)
            torch.mul(db.WB, path[j][None, :], out=xB)
            torch.mul(db.CLW, path[j][None, :], out=xC)
            rt._chk(lib.monortm_hip_jacobian_dev(rt.ctx, n, nwn, d(db.wn), p0.dvset, d(db.nlay), lm, db.nmol, d(db.P), d(db.T), d(xC), d(xW),
                                                 d(xB), api._ptr(db.fac), p0.sclcpl, p0.sclhw, p0.y0res, p0.ibrd, d(db.irt), d(db.TZ),
                                                 d(db.tmpsfc0), d(db.emiss), d(db.reflc), 1, nj, api._ptr(jm),
                                                 *[d(ob[k]) for k in api.JAC_FIELDS], api._ptr(db.wn_ends), sp))

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
    res = dict(nprof=n, nlay=lm, nwn=nwn, npath=npath, njac=nj, zenith_deg=[float(x) for x in zen])
    t = {k: stats([a.elapsed_time(b) for a, b in ev[k]]) for k in variants}
    names = dict(a="scan_jacobian_ms", b="jacobian_per_path_ms")
    for k in variants:
        res[names[k]] = t[k]
    if "a" in t and "b" in t:
        out = var_a()
        var_b()
        torch.cuda.synchronize()

        def rel(x, y):   # the last path: worst difference over the layer axis relative to the largest value on it
            scale = y.abs().amax(dim=1, keepdim=True)
            return float(((x - y).abs() / torch.where(scale > 0, scale, torch.ones_like(scale))).max().item())

        res["k_t_rel_diff_a_b"] = rel(out["k_t"][:, -1], ob["k_t"])
        res["k_w_rel_diff_a_b"] = rel(out["k_w"][:, -1], ob["k_w"])
        res["finite"] = bool(all(torch.isfinite(v).all().item() for v in out.values()))
        res["b_over_a"] = t["b"]["median"] / t["a"]["median"]
    return res


def workload():
    """The configs[3] batch of bench.py: line records, the 1024 profiles and the description."""
    import bench

    rec, profs, desc, _rk, _t3kw = bench.build_workload("c4", 0, 128)
    return rec, profs, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default="2,4,8,16")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", choices=["", "a", "b"])
    args = ap.parse_args()
    import torch

    from monortm_amd import api, tape3

    if not torch.cuda.is_available():
        raise SystemExit("scan_jacobian_bench needs the GPU (no CPU fallback)")
    rec, profs, desc = workload()
    wn = profs[0].wn
    res = dict(what="DeviceBatch.scan_jacobian (a) vs monortm_hip_jacobian_dev per path on amounts scaled on the device (b), device events",
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
