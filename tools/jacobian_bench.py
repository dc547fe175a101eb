"""Time of a Jacobian call against a plain step, on the configs[3] shape (1024 profiles x 64 layers x 50 channels x 500 lines, f64)
and on a single profile of the same shape (LABNOTES).

    python tools/jacobian_bench.py [--calls 30] [--warmup 5] [--out FILE] [--vars "1;1,p,wbrod;1,xself,xfrgn,sclcpl"]
    python tools/jacobian_bench.py --xs [--calls 30] [--warmup 5] [--out FILE]

K = T + H2O (jac_mol = 1) + cloud + surface, q = TB; --vars: the Jacobian variables instead of H2O alone - lists separated by ";",
each a comma-separated mix of molecules and names of api.JAC_VARS, one result per case and list.
Per case: device-event times of DeviceBatch.jacobian and of DeviceBatch.step,
one of each in turn (interleaved, after warm-up), median / min / max / IQR of each, the ratio of the medians, and the number of
forward runs that brute-force differences (one layer at a time) would need for the same K.  Prints one JSON line.

--xs: monortm_hip_jacobian_xs_dev with ixsect = 1 against the same call with ixsect = 0, and
monortm_hip_modm_xs_dev with ixsect = 1 against 0, on a synthetic table set (xsec.synthetic_library: CCL4, F11, F12) - 64 channels over
780 - 950 cm-1, 32 layers, K = T + ln P + the three molecules against K = T + ln P.  The two differences are what the cross sections
cost a Jacobian call (xsec_kernel for the base state + xsec_jac_kernel for T +- h and P (1 +- eps)) and a plain MODM call
(xsec_kernel); their ratio, less one, is xsec_jac_kernel in units of xsec_kernel."""
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


def run_xs(api, rt, profs, calls, warmup):
    """Device-event times of the four calls in turn (interleaved, after warm-up), on device copies of the batch."""
    import ctypes as C

    import torch

    cuda = torch.device("cuda")
    n, lm, nw, nmol, nx = len(profs), max(p.nlay for p in profs), profs[0].nwn, profs[0].nmol, len(profs[0].xs_names)
    p0 = profs[0]

    def pack(get, *tail):
        out = np.zeros((n, lm) + tail)
        for i, p in enumerate(profs):
            out[i, : p.nlay] = get(p)
        return torch.from_numpy(out).to(cuda)

    P, T, CLW, WB = (pack(lambda p, k=k: getattr(p, k)) for k in ("p", "t", "clw", "wbrodl"))
    WKL, XA = pack(lambda p: p.wkl, nmol), pack(lambda p: p.xamnt, nx)
    TZ = torch.zeros(n, lm + 1, dtype=torch.float64, device=cuda)
    for i, p in enumerate(profs):
        TZ[i, : p.nlay + 1] = torch.from_numpy(np.ascontiguousarray(p.tz)).to(cuda)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=cuda)  # noqa: E731
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(cuda)  # noqa: E731
    nlay, irt, wn = i32([p.nlay for p in profs]), i32([p.irt for p in profs]), f64(p0.wn)
    ts, em, rf = f64([p.tmpsfc for p in profs]), f64(np.stack([p.emiss for p in profs])), f64(np.stack([p.reflc for p in profs]))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=cuda)  # noqa: E731
    fac, ends = np.ascontiguousarray(p0.cntnm, np.float64), np.array([p0.wn[0], p0.wn[-1]])
    d = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    h = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    sp = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    jm = {1: api.jac_codes(("p",) + tuple(f"xs:{x}" for x in p0.xs_names), p0.xs_names), 0: api.jac_codes(("p",))}
    out = {x: dict(o=z(n, lm, nw), rad=z(n, nw), tb=z(n, nw), k_t=z(n, lm, nw), k_tz=z(n, lm + 1, nw), k_w=z(n, lm, len(jm[x]), nw),
                   k_clw=z(n, lm, nw), k_o=z(n, lm, nw), k_sfc=z(n, 3, nw)) for x in (0, 1)}
    O, OBM, OC, OL, ODX = z(n, lm, nw), z(n, lm, nmol, nw), z(n, lm, api.NCONT, nw), z(n, lm, nw), z(n, lm, nw)

    def jac(x):
        rt._chk(rt.lib.monortm_hip_jacobian_xs_dev(rt.ctx, n, nw, d(wn), p0.dvset, d(nlay), lm, nmol, d(P), d(T), d(CLW), d(WKL), d(WB), h(fac),
                                                   p0.sclcpl, p0.sclhw, p0.y0res, p0.ibrd, x, d(XA) if x else None, d(irt), d(TZ), d(ts), d(em),
                                                   d(rf), 1, len(jm[x]), h(jm[x]), *[d(out[x][k]) for k in api.JAC_FIELDS], h(ends), sp()))

    def modm(x):
        rt._chk(rt.lib.monortm_hip_modm_xs_dev(rt.ctx, n, nw, d(wn), p0.dvset, d(nlay), lm, nmol, d(P), d(T), d(CLW), d(WKL), d(WB), h(fac),
                                               p0.sclcpl, p0.sclhw, p0.y0res, p0.ibrd, x, d(XA) if x else None, d(ODX) if x else None, d(O),
                                               d(OBM), d(OC), d(OL), h(ends), sp()))

    runs = [("jacobian_xs", lambda: jac(1)), ("jacobian", lambda: jac(0)), ("modm_xs", lambda: modm(1)), ("modm", lambda: modm(0))]
    for _ in range(warmup):
        for _, f in runs:
            f()
    torch.cuda.synchronize()
    rt._chk(rt.lib.monortm_hip_check(rt.ctx, sp()))
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in runs] for _ in range(calls)]
    for i in range(calls):
        for (a, b), (_, f) in zip(ev[i], runs):
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    rt._chk(rt.lib.monortm_hip_check(rt.ctx, sp()))
    t = {name: stats([ev[i][k][0].elapsed_time(ev[i][k][1]) for i in range(calls)]) for k, (name, _) in enumerate(runs)}
    dj, dm = t["jacobian_xs"]["median"] - t["jacobian"]["median"], t["modm_xs"]["median"] - t["modm"]["median"]
    finite = bool(all(torch.isfinite(v).all().item() for v in out[1].values()))
    return dict(nprof=n, nlay=lm, nwn=nw, nxs=nx, ms=t, xs_cost_jacobian_ms=dj, xs_cost_modm_ms=dm, xsec_jac_over_xsec=dj / dm - 1.0,
                finite=finite)


def main_xs(args):
    import dataclasses

    import torch

    from monortm_amd import api, synth, tape3, xsec

    if not torch.cuda.is_available():
        raise SystemExit("jacobian_bench needs the GPU (no CPU fallback)")
    wn = np.linspace(781.0, 949.0, 64)
    res = dict(what="jacobian_xs (ixsect = 1, T + ln P + 3 cross-section molecules) vs the same call with ixsect = 0; modm_xs vs modm; "
                    "device events", cases={})
    with tempfile.TemporaryDirectory() as d:
        t3 = os.path.join(d, "TAPE3")
        tape3.write_tape3(t3, synth.synthetic_lines(500))
        names = xsec.synthetic_library(os.path.join(d, "xs"))
        tabs = xsec.load_tables(os.path.join(d, "xs"), names, float(wn[0]), float(wn[-1]))
        rt = api.MonoRTM(t3, wn[0], wn[-1], device=0)
        rt.set_xsec(tabs)
        for name, n in (("batch64", 64), ("single", 1)):
            rng = np.random.default_rng(5)
            profs = [dataclasses.replace(synth.perturbed_profile(i, wn, nlay=32, irt=(1 if i % 2 == 0 else 3)), xs_names=list(names),
                                         xamnt=1e15 * rng.uniform(0.5, 2.0, (32, len(names)))) for i in range(n)]
            res["cases"][name] = run_xs(api, rt, profs, args.calls, args.warmup)
        rt.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--xs", action="store_true", help="the cross-section Jacobians against the same calls without them")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="whole,single")
    ap.add_argument("--vars", default="1")
    args = ap.parse_args()
    if args.xs:
        line = json.dumps(main_xs(args))
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
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
