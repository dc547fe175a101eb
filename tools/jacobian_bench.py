"""Time of a Jacobian call against a plain step, on the configs[3] shape (1024 profiles x 64 layers x 50 channels x 500 lines, f64)
and on a single profile of the same shape (LABNOTES).

    python tools/jacobian_bench.py [--calls 30] [--warmup 5] [--out FILE] [--vars "1;1,p,wbrod;1,xself,xfrgn,sclcpl"]

K = T + H2O (jac_mol = 1) + cloud + surface, q = TB; --vars: the Jacobian variables instead of H2O alone - lists separated by ";",
each a comma-separated mix of molecules and names of api.JAC_VARS, one result per case and list.
Per case: device-event times of DeviceBatch.jacobian and of DeviceBatch.step,
one of each in turn (interleaved, after warm-up), median / min / max / IQR of each, the ratio of the medians, and the number of
forward runs that brute-force differences (one layer at a time) would need for the same K.  Prints one JSON line."""
from __future__ import annotations

import argparse
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


def run_case(api, rt, profs, mols, calls, warmup):
    import torch

    db = api.DeviceBatch(rt, profs)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2 * calls)]
    for _ in range(warmup):
        db.jacobian(mols=mols)
        db.step()
    torch.cuda.synchronize()
    db.check()
    jt, st = [], []
    for i in range(calls):
        a, b = ev[2 * i]
        a.record()
        db.jacobian(mols=mols)
        b.record()
        c, d = ev[2 * i + 1]
        c.record()
        db.step()
        d.record()
    torch.cuda.synchronize()
    db.check()
    for i in range(calls):
        jt.append(ev[2 * i][0].elapsed_time(ev[2 * i][1]))
        st.append(ev[2 * i + 1][0].elapsed_time(ev[2 * i + 1][1]))
    nlay, nj = db.lm, len(mols)
    j, s = stats(jt), stats(st)
    k = db.jacobian(mols=mols)
    torch.cuda.synchronize()
    finite = bool(all(torch.isfinite(v).all().item() for v in k.values()))
    return dict(nprof=db.nprof, nlay=nlay, nwn=db.nwn, jac_mol=list(mols), modm_evaluations=3 + 2 * nj, jacobian_ms=j, step_ms=s,
                ratio=j["median"] / s["median"],
                # one base run + central differences of every layer's T, ln WKL of each molecule and CLW (surface: + 6)
                brute_force_runs=1 + 2 * nlay * (1 + nj + 1) + 6, brute_force_runs_t_h2o=1 + 2 * nlay * (1 + nj), finite=finite)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="whole,single")
    ap.add_argument("--vars", default="1")
    args = ap.parse_args()
    import torch

    from monortm_amd import api, synth, tape3

    if not torch.cuda.is_available():
        raise SystemExit("jacobian_bench needs the GPU (no CPU fallback)")
    var_lists = [tuple(int(v) if v.strip().isdigit() else v.strip() for v in lst.split(",") if v.strip())
                 for lst in args.vars.split(";")]
    wn = synth.c2_channels(50)
    res = dict(what="Jacobian (T + H2O + cloud + surface, TB) vs plain step, device events", cases={})
    with tempfile.TemporaryDirectory() as d:
        t3 = os.path.join(d, "TAPE3")
        tape3.write_tape3(t3, synth.synthetic_lines(500))
        rt = api.MonoRTM(t3, wn[0], wn[-1], device=0)
        for name in args.cases.split(","):
            n = 1024 if name == "whole" else 1
            profs = [synth.perturbed_profile(i, wn, nlay=64, cloud=True, irt=(1 if i % 2 == 0 else 3)) for i in range(n)]
            for lst in var_lists:
                key = name if len(var_lists) == 1 else f"{name}[{','.join(str(v) for v in lst)}]"
                res["cases"][key] = run_case(api, rt, profs, lst, args.calls, args.warmup)
        rt.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
