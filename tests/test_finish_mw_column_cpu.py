"""The option parser and the launch rule of the microwave finish kernel's two layouts (monortm_amd/csrc/finish_mw_layout.hpp) without
a GPU: tests/native/finish_mw_layout_check.cpp compiles the header's host code and answers one request per line.

The rule, restated here from its description: never the column layout for sliced line lists or when 65 doubles per coarse item plus
four ABSRB grids per wave exceed 40 KB; `layer` never, `column` wherever it can run; `auto` only for one block of channels (<= 64),
at least 32 layers and at least four column workgroups (profiles x blocks of 64 layers) per compute unit.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (shutil.which(HIPCC) or os.path.exists(HIPCC)), reason="hipcc not found")

AUTO, LAYER, COLUMN = 0, 1, 2
NW = 4
C4 = dict(nprof=1024, nlay_max=64, nwn=50, cus=256, nA=55, NPTABS=40, sliced=0)   # configs[3] whole on an MI355X


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = tmp_path_factory.mktemp("finish_mw_layout") / "finish_mw_layout_check"
    src = os.path.join(ROOT, "tests", "native", "finish_mw_layout_check.cpp")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "c++", src, "-o", str(exe)], check=True, timeout=600)

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), check=True, capture_output=True, text=True, timeout=60)
        rows = [dict(kv.split("=") for kv in ln.split()) for ln in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return [{k: int(v) for k, v in r.items()} for r in rows]

    return run


def rule(ask, opt, **kw):
    r = {**C4, **kw}
    return ask([f"rule {r['nprof']} {r['nlay_max']} {r['nwn']} {r['cus']} {r['nA']} {r['NPTABS']} {r['sliced']} {opt}"])[0]


def lds_bytes(nA, NPTABS, nw=NW):
    return 8 * (nA * 65 + nw * 4 * (NPTABS + 4))


def test_option_values_parse_strictly(ask):
    good = {"": AUTO, "auto": AUTO, "layer": LAYER, "column": COLUMN}
    got = ask(["parse" + (" " + v if v else "") for v in good])
    assert [g["ok"] for g in got] == [1] * len(good) and [g["opt"] for g in got] == list(good.values())
    bad = ["Layer", "COLUMN", "col", "columns", "1", "0", "on", "off", "auto ", " layer", "layer,column"]
    assert all(g["ok"] == 0 for g in ask(["parse " + v for v in bad]))


def test_lds_budget(ask):
    assert rule(ask, COLUMN)["lds"] == lds_bytes(55, 40) <= 40960
    # the widest range that fits at NPTABS = 40, and the first that does not
    fit = max(n for n in range(1, 200) if lds_bytes(n, 40) <= 40960)
    assert lds_bytes(fit + 1, 40) > 40960
    assert rule(ask, COLUMN, nA=fit)["waves"] == NW and rule(ask, COLUMN, nA=fit + 1)["waves"] == 0
    assert rule(ask, AUTO, nA=fit)["waves"] == NW and rule(ask, AUTO, nA=fit + 1)["waves"] == 0


def test_forced_layouts(ask):
    for kw in (dict(), dict(nprof=1), dict(nwn=130), dict(nlay_max=1), dict(nlay_max=603)):
        assert rule(ask, LAYER, **kw)["waves"] == 0
        assert rule(ask, COLUMN, **kw)["waves"] == NW
    for opt in (AUTO, LAYER, COLUMN):
        assert rule(ask, opt, sliced=1)["waves"] == 0


def test_auto_at_its_boundaries(ask):
    assert rule(ask, AUTO)["waves"] == NW                                   # configs[3] whole: 1024 workgroups on 256 compute units
    assert rule(ask, AUTO, nprof=1023)["waves"] == 0
    assert rule(ask, AUTO, nprof=128)["waves"] == 0                          # the 128-profile shard
    assert rule(ask, AUTO, nprof=1)["waves"] == 0                            # single profiles
    assert rule(ask, AUTO, nprof=512, nlay_max=65)["waves"] == NW            # two blocks of layers per profile
    assert rule(ask, AUTO, nprof=511, nlay_max=65)["waves"] == 0
    assert rule(ask, AUTO, cus=257)["waves"] == 0 and rule(ask, AUTO, nprof=416, cus=104)["waves"] == NW
    assert rule(ask, AUTO, nwn=64)["waves"] == NW and rule(ask, AUTO, nwn=65)["waves"] == 0
    assert rule(ask, AUTO, nlay_max=32)["waves"] == NW and rule(ask, AUTO, nlay_max=31)["waves"] == 0
