#!/usr/bin/env python3
"""Dump the outputs of one bench workload (tools/ab_dump.py WORKLOAD OUT.npz) with the library named by MONORTM_HIP_LIB:
two runs with two builds, then tools/ab_dump.py --compare A B prints, per array, whether the two are bitwise equal (np.array_equal)
and the largest relative difference.  A and B are .npz files of this tool or directories of bench.py --dump-outputs (one .npy per
array); the exit status is 1 if an array differs or is missing."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

def _arrays(path):
    if os.path.isdir(path):
        return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith(".npy")}
    z = np.load(path)
    return {k: z[k] for k in z.files}


if sys.argv[1] == "--compare":
    a, b = _arrays(sys.argv[2]), _arrays(sys.argv[3])
    same = set(a) == set(b) and len(a) > 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k:16s} only in one of the two")
            continue
        x, y = a[k], b[k]
        eq = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)
        same = same and eq
        rel = float("nan")
        if x.shape == y.shape and y.size and np.issubdtype(y.dtype, np.floating):
            scale = np.maximum(np.abs(y), 1e-12 * np.nanmax(np.abs(y)))
            rel = float(np.nanmax(np.abs(x - y) / np.maximum(scale, 1e-300)))
        print(f"{k:16s} {str(x.shape):22s} array_equal {eq}  max rel diff {rel:.3e}")
    print("BITWISE EQUAL" if same else "DIFFERENT")
    sys.exit(0 if same else 1)

import bench  # noqa: E402
from monortm_amd import api, tape3  # noqa: E402

rec, profs, desc, _rk, _t3kw = bench.build_workload(sys.argv[1], 0, int(os.environ.get("AB_DUMP_PROFILES", "8")))
d = tempfile.mkdtemp()
t3 = os.path.join(d, "TAPE3")
tape3.write_tape3(t3, rec, **_t3kw)
rt = api.MonoRTM(t3, profs[0].wn[0], profs[0].wn[-1])
b = api.DeviceBatch(rt, profs)
b.step()
b.check()
np.savez(sys.argv[2], o=b.O.cpu().numpy(), obm=b.OBM.cpu().numpy(), rad=b.RAD.cpu().numpy(), tb=b.TB.cpu().numpy())
