"""Time of a path scan against what the API offered before it, on the configs[3] shape (bench.build_workload("c4"): 1024 profiles x
64 layers x 50 channels x 500 lines, f64) and on a single profile of the same shape (LABNOTES).

    python tools/scan_bench.py [--paths 8] [--calls 30] [--warmup 5] [--cases whole,single] [--only a] [--out FILE]

Per case, device-event times of three variants, one of each in turn (interleaved, after warm-up):
  a  DeviceBatch.scan: one MODM pass + one rtm_scan launch for all paths;
  b  one step() per path on amounts (WKL, WBRODL, CLW) scaled by the path - a full MODM + RTM per path;
  c  one MODM pass, then per path a torch multiply of O into a scratch tensor + monortm_hip_rtm_dev on it.
Median / min / max / IQR of each, the differences a - c and a - b, and the largest relative difference of TB between a and c.
--only a|b|c runs one variant alone (for a kernel trace of its own).  Prints one JSON line."""
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


def run_case(api, rt, profs, npath, calls, warmup, only):
    import torch

    db = api.DeviceBatch(rt, profs)
    dev, lm, n, nwn = db.dev, db.lm, db.nprof, db.nwn
    zen = np.linspace(0.0, 75.0, npath)
    path = torch.as_tensor(api.plane_parallel_path(zen, lm)).to(dev)                   # [npath, lm]
    fd = path.unsqueeze(0).expand(n, -1, -1).contiguous()                              # [nprof, npath, lm]
    # b: the amounts of every path, scaled beforehand (swapping them in costs nothing on the device)
    base = (db.WKL, db.WB, db.CLW)
    scaled = [(db.WKL * path[j][None, :, None], db.WB * path[j][None, :], db.CLW * path[j][None, :]) for j in range(npath)]
    # c: the scaled optical depths of one path at a time, and the outputs of every path
    scratch = torch.empty_like(db.O)
    outs_c = torch.zeros(npath, 6, n, nwn, dtype=db.O.dtype, device=dev)
    ts_c = db.tmpsfc0.clone()
    d = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    p0, lib = db.p0, rt.lib

    def var_a():
        db.scan(fd)

    def var_b():
        for j in range(npath):
            db.WKL, db.WB, db.CLW = scaled[j]
            db.step()
        db.WKL, db.WB, db.CLW = base

    def var_c():
        sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rt._chk(lib.monortm_hip_modm_dev(rt.ctx, n, nwn, d(db.wn), p0.dvset, d(db.nlay), lm, db.nmol, d(db.P), d(db.T), d(db.CLW), d(db.WKL),
                                         d(db.WB), api._ptr(db.fac), p0.sclcpl, p0.sclhw, p0.y0res, p0.ibrd, 0, d(db.O), d(db.OBM), d(db.OC),
                                         d(db.OCLW), api._ptr(db.wn_ends), sp))
        for j in range(npath):
            torch.mul(db.O, path[j][None, :, None], out=scratch)
            o = outs_c[j]   # rad, tb, trtot, tmr, rup, rdn: the order of spectral_block()
            rt._chk(lib.monortm_hip_rtm_dev(rt.ctx, n, nwn, d(db.wn), d(db.nlay), lm, d(db.irt), p0.iout, d(db.T), d(db.TZ), d(scratch),
                                            d(ts_c), d(db.emiss), d(db.reflc), d(o[4]), d(o[5]), d(o[2]), d(o[0]), d(o[1]), d(o[3]), sp))

    variants = {k: v for k, v in (("a", var_a), ("b", var_b), ("c", var_c)) if only in ("", k)}
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
    res = dict(nprof=n, nlay=lm, nwn=nwn, npath=npath, zenith_deg=[float(z) for z in zen])
    t = {k: stats([a.elapsed_time(b) for a, b in ev[k]]) for k in variants}
    names = dict(a="scan_ms", b="steps_ms", c="modm_scaled_rtm_ms")
    for k in variants:
        res[names[k]] = t[k]
    if "a" in t and "c" in t:
        blk = db.scan(fd)
        var_c()
        torch.cuda.synchronize()
        tb_a, tb_c = blk[1], outs_c[:, 1].permute(1, 0, 2)
        res["tb_max_rel_diff_a_c"] = float(((tb_a - tb_c).abs() / tb_c.abs()).max().item())
        res["finite"] = bool(torch.isfinite(blk).all().item())
        res["c_minus_a_ms"] = t["c"]["median"] - t["a"]["median"]
        res["a_faster_than_c_by_more_than_iqr"] = bool(res["c_minus_a_ms"] > max(t["a"]["iqr"], t["c"]["iqr"]))
    if "a" in t and "b" in t:
        res["b_over_a"] = t["b"]["median"] / t["a"]["median"]
    return res


def workload():
    """The configs[3] batch of bench.py: line records, the 1024 profiles and the description."""
    import bench

    rec, profs, desc, _rk, _t3kw = bench.build_workload("c4", 0, 128)
    return rec, profs, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=8)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="whole,single")
    ap.add_argument("--only", default="", choices=["", "a", "b", "c"])
    args = ap.parse_args()
    import torch

    from monortm_amd import api, tape3

    if not torch.cuda.is_available():
        raise SystemExit("scan_bench needs the GPU (no CPU fallback)")
    rec, profs, desc = workload()
    wn = profs[0].wn
    res = dict(what="path scan (a) vs one step per path (b) vs MODM + scaled O + rtm per path (c), device events", workload=desc, cases={})
    with tempfile.TemporaryDirectory() as d:
        t3 = os.path.join(d, "TAPE3")
        tape3.write_tape3(t3, rec)
        rt = api.MonoRTM(t3, wn[0], wn[-1], device=0)
        for name in args.cases.split(","):
            res["cases"][name] = run_case(api, rt, profs if name == "whole" else profs[:1], args.paths, args.calls, args.warmup, args.only)
        rt.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
