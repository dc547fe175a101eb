"""The launch plan of a MODM evaluation (monortm_amd/csrc/modm_plan.hpp) held to the Python mirrors without a GPU.

tests/native/modm_plan_check.cpp reads one ModmPlanIn per line and prints the fields of its ModmPlan; hipcc compiles the header's host
side, no GPU is touched.  Three things are asserted:
  * far_cases.plan (the tile choice, the level count, the interval count and the workspace of far_kernel) for every case of
    far_cases.CASES, in both precisions, with the case's own tile_waves, far_levels and nslice;
  * test_ms_prepare_passes._layout (G, CL, passes, LDS bytes of lines_ms_kernel) for every row of its CASES;
  * the shapes that the comments of modm_plan.hpp name, each for what its comment states.
The mirrors are the independent statement: a heuristic edited in modm_plan.hpp alone fails here, before any GPU test runs.
A new kernel variant adds its rule to modm_plan.hpp and its row to NAMED below ("Plan, then execute").
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import far_cases as fc
import test_ms_prepare_passes as msp
from monortm_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (shutil.which(HIPCC) or os.path.exists(HIPCC)), reason="hipcc not found")

LEAST_CAPS = dict(phys_cap=fc.PHYS_CAP, far_cap=fc.FAR_CAP)            # a context's least workspace caps
MI355X_CAPS = dict(phys_cap=(288 << 30) // 8, far_cap=(288 << 30) // 32)  # an eighth / a thirty-second of 288 GB
FIELDS = ("nprof", "nwn", "nlay_max", "nmol", "real_kind", "ibrd", "ixsect", "v1", "v2", "nlines", "lines_per_cm", "lc_frac", "any_brd", "ms_nslot",
          "cus", "phys_cap", "far_cap", "nslice", "fair", "tile_waves", "far_levels", "lines_ms", "ms_items", "finish_generic", "no_physics_pass")
DEFAULTS = dict(nmol=7, real_kind=8, ibrd=0, ixsect=0, lc_frac=0.0, any_brd=0, cus=256, nslice=0, fair=-1, tile_waves=0, far_levels=-1, lines_ms=-1,
                ms_items=0, finish_generic=0, no_physics_pass=0, **LEAST_CAPS)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = tmp_path_factory.mktemp("modm_plan") / "modm_plan_check"
    src = os.path.join(ROOT, "tests", "native", "modm_plan_check.cpp")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", src, "-o", str(exe)], check=True, timeout=600)

    def run(rows):
        """rows: dicts of ModmPlanIn fields (DEFAULTS where absent) -> dicts of the plans' fields (ints; doubles as floats)."""
        text = ""
        for r in rows:
            r = {**DEFAULTS, **r}
            assert set(r) == set(FIELDS), set(r) ^ set(FIELDS)
            text += " ".join(float(r[k]).hex() if k in ("v1", "v2", "lines_per_cm", "lc_frac") else str(int(r[k])) for k in FIELDS) + "\n"
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()
        assert len(out) == len(rows)
        plans = []
        for ln in out:
            assert ln.startswith("rc=0 "), ln
            plans.append({k: (float.fromhex(v) if "0x" in v else int(v)) for k, v in (kv.split("=") for kv in ln.split())})
        return plans

    return run


def table_constants(rec, v1, v2, nmol=fc.NMOL):
    """nlines, lines per cm-1 and (molecule, isotopologue) slots of the table a context holds of `rec` for [v1, v2] (api.hip,
    monortm_hip_init; MOL = molecule + 100 x isotopologue)."""
    kept = fc.kept_records(rec, v1, v2)
    kept = kept[np.asarray(rec.iflg)[kept] >= 0]
    vnu, mol, iso = np.asarray(rec.vnu)[kept], np.asarray(rec.mol)[kept] % 100, np.asarray(rec.mol)[kept] // 100
    slots = sum(min(max(int(iso[mol == m].max()), 1), 9) for m in range(1, nmol + 1) if np.any(mol == m))
    return dict(nlines=len(kept), lines_per_cm=len(kept) / max(float(vnu.max() - vnu.min()), 1.0), ms_nslot=slots)


# ---------------------------------------------------------------------------------------------------------------------------------
# far_cases.plan
# ---------------------------------------------------------------------------------------------------------------------------------
def test_far_cases_follow_the_mirror(planner):
    rows, want = [], []
    for name, case in fc.CASES.items():
        for kind in (8, 4):
            pl = fc.plan(case, kind)
            tc = table_constants(pl.rec, float(pl.wn[0]), float(pl.wn[-1]))
            assert tc["nlines"] == pl.nlines and tc["lines_per_cm"] == pl.lines_per_cm and tc["ms_nslot"] == pl.nactive   # (isotopologue 1 only)
            for nslice in sorted({0, case.nslice}):
                rows.append(dict(nprof=len(case.layers), nwn=case.nwn, nlay_max=max(len(l) for l in case.layers), real_kind=kind,
                                 v1=float(pl.wn[0]), v2=float(pl.wn[-1]), nslice=nslice, tile_waves=0 if case.tile_waves == "auto" else case.tile_waves,
                                 far_levels=-1 if case.far_levels is None else case.far_levels, **tc))
                want.append((f"{name} real_kind={kind} nslice={nslice}", pl, nslice))
    for (what, pl, nslice), got in zip(want, planner(rows)):
        states = len(pl.case.layers) * max(len(l) for l in pl.case.layers)
        nbytes = states * fc.NMOL * (pl.ni * (fc.FAR_MOM_STRIDE * 8 + fc.FAR_GEOM_INTS * 4) + pl.ntile * fc.FAR_SEG_INTS * 4)   # far_cases.plan: bytes_for
        assert (got["TW"], got["ntiles"], got["far_levels"], got["far_ni"], got["far_bytes"]) == (pl.tw, pl.ntile, pl.levels, pl.ni, nbytes), what
        assert got["far_mom_bytes"] == states * pl.ni * fc.NMOL * fc.FAR_MOM_STRIDE * 8 and got["far_geom_bytes"] == states * pl.ni * fc.NMOL * fc.FAR_GEOM_INTS * 4, what
        assert got["far_rho_tile"] == pl.rho_tile and got["want_phys"] == 1 and got["wpl"] == 2 and got["nw"] * 128 == pl.tw, what
        if nslice:
            assert got["nslice"] == nslice, what


# ---------------------------------------------------------------------------------------------------------------------------------
# test_ms_prepare_passes._layout
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ms_layouts_follow_the_mirror(planner):
    keys = list(msp.CASES)
    rows = [dict(nprof=nprof, nwn=nwn, nlay_max=64, v1=0.3, v2=0.3 if nwn == 1 else 30.0, nlines=420, lines_per_cm=8.0, ms_nslot=5, lines_ms=1, ms_items=items)
            for nwn, nprof, items in keys]
    for (nwn, nprof, items), got in zip(keys, planner(rows)):
        g, cl, passes, _taken, lds = msp._layout(nwn, nprof, items, nslot=5)
        assert got["use_ms"] == 1 and got["ms_nprof"] == nprof, (nwn, nprof, items)
        assert (got["G"], got["CL"], got["nsteps"], got["ms_lds"]) == (g, cl, passes, lds), (nwn, nprof, items)
        assert got["spp"] == 64 // cl and got["LPS"] == (nwn + 4) // 5 and got["npg"] == -(-nprof // g) and got["nslice"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes the comments of modm_plan.hpp name (bench.py's workloads: configs[2], [3], [4] of BASELINE)
# ---------------------------------------------------------------------------------------------------------------------------------
def _c4(nprof, **kw):      # configs[3]: 64 layers x 50 channels x 500 lines, double precision
    wn = synth.c2_channels(50)
    return dict(nprof=nprof, nwn=50, nlay_max=64, v1=float(wn[0]), v2=float(wn[-1]), **table_constants(synth.synthetic_lines(500), wn[0], wn[-1]), **kw)


def _c5(runs):             # configs[4]: 64 layers x 200 channels U(0.3, 6.5) cm-1 x 500 lines, single precision
    wn = synth.c2_channels(200, lo=0.3, hi=6.5)
    return dict(nprof=runs, nwn=200, nlay_max=64, real_kind=4, v1=float(wn[0]), v2=float(wn[-1]), **table_constants(synth.synthetic_lines(500), wn[0], wn[-1]))


def _c3():                 # configs[2]: 1 profile x 64 layers x 10000 wavenumbers in steps of 0.005 cm-1 x 100000 lines
    wn = 0.5 + 0.005 * np.arange(10000)
    return dict(nprof=1, nwn=10000, nlay_max=64, v1=float(wn[0]), v2=float(wn[-1]),
                **table_constants(synth.synthetic_lines(100000, seed=20261004), wn[0], wn[-1]), **MI355X_CAPS)


def _ending_at(v2):        # configs[3]'s channel set moved so that it ends at v2
    return {**_c4(128), "v1": v2 - 29.0, "v2": v2}


# (row, what its comment states)
NAMED = {
    "configs[3]'s shape at 384 profiles goes to lines_ms_kernel": (lambda: _c4(384), lambda p: p["use_ms"] == 1 and p["ms_nprof"] == 384 and p["G"] == 6),
    "512 profiles split 384 + 128": (lambda: _c4(512), lambda p: p["use_ms"] == 1 and p["ms_nprof"] == 384 and p["grid_y"] == 512 and p["nslice"] == 1),
    "a 200-channel float sounder batch at 8192 states takes (1, 4)": (lambda: _c5(128), lambda p: (p["nw"], p["wpl"]) == (1, 4)),
    "... and at 4096 states two tiles of 128": (lambda: _c5(64), lambda p: (p["nw"], p["wpl"], p["ntiles"]) == (1, 2, 2)),
    "a dense grid of 0.005 cm-1 steps takes one-wave far tiles": (_c3, lambda p: p["far_tiles"] == 1 and (p["nw"], p["wpl"], p["TW"]) == (1, 2, 128) and p["far_levels"] >= 1),
    "below 820 cm-1: finish_mw_kernel": (lambda: _ending_at(819.9), lambda p: p["mw"] == 1 and p["finish_variant"] == 0),
    "above 820 cm-1: finish_kernel on the 2 cm-1 grid": (lambda: _ending_at(820.1), lambda p: p["mw"] == 0 and p["high"] == 0 and p["finish_variant"] in (2, 3, 4, 5)),
    "below 1340 cm-1: the 2 cm-1 grid": (lambda: _ending_at(1339.9), lambda p: p["high"] == 0 and p["finish_variant"] in (2, 3, 4, 5) and p["csize"] == p["NPTABS"] // 2 + 24),
    "above 1340 cm-1: finish_kernel<HIGH> on the 1 cm-1 grid": (lambda: _ending_at(1340.1), lambda p: p["high"] == 1 and p["finish_variant"] == 1 and p["csize"] == p["NPTABS"] + 24),
}


def test_named_shapes(planner):
    names = list(NAMED)
    for name, got in zip(names, planner([NAMED[n][0]() for n in names])):
        assert NAMED[name][1](got), f"{name}: {got}"
