"""Time of the forward measurement operator against the ways the API offered to get the same Y before it, on the configs[3] shape
(bench.build_workload("c4"): 1024 profiles x 64 layers x 50 channels x 500 lines, f64) (LABNOTES section 20).

    python tools/obs_bench.py [--paths 4,16,64] [--calls 20] [--warmup 3] [--only a] [--quantity tb] [--out FILE]

The operator of tools/obs_jacobian_bench.py: the 50 wavenumbers in 10 channels of 5 - channel 1 nested inside channel 0, the others
runs of 5 - and views of 4 adjacent paths each, uniform normalised weights.  Per number of paths, device-event times of four
variants, one of each in turn (interleaved, after warm-up):
  a  DeviceBatch.obs: one MODM pass + one rtm_obs launch that contracts as it goes;
  b  DeviceBatch.scan (RUP, RDN, TRTOT, RAD, TB, TMR of every path and wavenumber written out) + the contraction in torch with
     ObsOperator.dense();
  c  DeviceBatch.obs_jacobian with njac = 1: what a caller had to run to get this Y in this order;
  d  DeviceBatch.step(): one MODM pass + one monochromatic RTM, the floor.
Median / min / max / IQR of each, the bytes of output tensors each variant holds, the largest difference of Y between a and b
(relative to the largest |Y|) and the number of elements of a's Y that differ in any bit from c's.  --only a|b|c|d runs one variant
alone.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = dict(a="obs_ms", b="scan_then_contraction_ms", c="obs_jacobian_njac1_ms", d="step_ms")


def stats(ms):
    a = np.asarray(ms)
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()), iqr=float(q3 - q1), n=len(a))


def operator(npath, nwn):
    """10 channels of 5 on 50 wavenumbers (in general nwn // 5 channels): channel 0 = samples 0, 2, 4, 6, 8, channel 1 = 1, 3, 5, 7, 9 -
    nested - and channel c >= 2 = samples 5 c .. 5 c + 4; views of 4 adjacent paths."""
    from monortm_amd import api

    nchan = nwn // 5
    channels = [[0, 2, 4, 6, 8], [1, 3, 5, 7, 9]] + [list(range(5 * c, 5 * c + 5)) for c in range(2, nchan)]
    views = [list(range(v, min(v + 4, npath))) for v in range(0, npath, 4)]
    op, perm = api.ObsOperator.from_sets(views, channels, npath=npath, nwn=nwn)
    assert np.array_equal(perm, np.arange(npath))
    return op


def nbytes(tensors):
    return int(sum(v.numel() * v.element_size() for v in tensors))


def run_case(api, rt, profs, npath, calls, warmup, only, quantity):
    import torch

    db = api.DeviceBatch(rt, profs)
    dev, lm, n, nwn = db.dev, db.lm, db.nprof, db.nwn
    zen = np.linspace(0.0, 75.0, npath)
    fd = torch.as_tensor(api.plane_parallel_path(zen, lm)).to(dev).unsqueeze(0).expand(n, -1, -1).contiguous()   # [nprof, npath, lm]
    op = operator(npath, nwn)
    h = rt.obs_create(op)
    W = torch.as_tensor(op.dense().reshape(op.nview, op.nchan, npath, nwn)).to(dev)
    field = dict(rad=0, tb=1)[quantity]   # index into the block of DeviceBatch.scan
    held = {}

    def var_a():
        held["a"] = db.obs(fd, h, quantity=quantity)

    def var_b():
        blk = db.scan(fd)
        held["b_mono"] = blk
        held["b"] = torch.einsum("pji,vcji->pvc", blk[field], W)

    def var_c():
        held["c"] = db.obs_jacobian(fd, h, mols=(1,), quantity=quantity)

    def var_d():
        db.step()

    variants = {k: v for k, v in (("a", var_a), ("b", var_b), ("c", var_c), ("d", var_d)) if only in ("", k)}
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
    res = dict(nprof=n, nlay=lm, nwn=nwn, npath=npath, nview=op.nview, nchan=op.nchan, quantity=quantity)
    t = {k: stats([a.elapsed_time(b) for a, b in ev[k]]) for k in variants}
    for k in variants:
        res[NAMES[k]] = t[k]
    if "a" in held:
        res["a_output_bytes"] = nbytes([held["a"]])
    if "b" in held:
        res["b_output_bytes"] = nbytes([held["b_mono"], held["b"]])
    if "c" in held:
        res["c_output_bytes"] = nbytes(held["c"].values())
    if "d" in variants:
        res["d_output_bytes"] = nbytes([db.spectral_block()])
    if "a" in held and "b" in held:
        res["max_diff_y_a_b"] = float((held["a"] - held["b"]).abs().max().item())
        res["rel_diff_y_a_b"] = res["max_diff_y_a_b"] / float(held["b"].abs().max().item())
        res["finite"] = bool(torch.isfinite(held["a"]).all().item())
    if "a" in held and "c" in held:
        res["y_elements_a_differs_from_c"] = int((held["a"] != held["c"]["y"]).sum().item())
    if "a" in t and "d" in t:
        res["a_minus_d_per_path_ms"] = (t["a"]["median"] - t["d"]["median"]) / npath
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
    ap.add_argument("--quantity", default="tb", choices=["tb", "rad"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", choices=["", "a", "b", "c", "d"])
    args = ap.parse_args()
    import torch

    from monortm_amd import api, tape3

    if not torch.cuda.is_available():
        raise SystemExit("obs_bench needs the GPU (no CPU fallback)")
    rec, profs, desc = workload()
    wn = profs[0].wn
    res = dict(what="DeviceBatch.obs (a) vs DeviceBatch.scan + torch contraction with ObsOperator.dense() (b) vs DeviceBatch.obs_jacobian, "
                    "njac = 1 (c) vs DeviceBatch.step (d), device events", workload=desc, cases={})
    with tempfile.TemporaryDirectory() as d:
        t3 = os.path.join(d, "TAPE3")
        tape3.write_tape3(t3, rec)
        rt = api.MonoRTM(t3, wn[0], wn[-1], device=0)
        for npath in (int(x) for x in args.paths.split(",")):
            res["cases"][str(npath)] = run_case(api, rt, profs, npath, args.calls, args.warmup, args.only, args.quantity)
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
