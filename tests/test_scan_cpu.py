"""Path scans (monortm_hip_rtm_scan), the part that needs no GPU: the two entry points are declared, bound
and exported; plane_parallel_path; and the premise of the feature on the CPU oracle - scaling every amount of a layer by s, with the
layer's P and T untouched, scales the layer's optical depth by s."""
import copy
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from common import ROOT
from monortm_amd import _build, api, synth, tape3

SCAN_SYMBOLS = ("monortm_hip_rtm_scan", "monortm_hip_rtm_scan_dev")


def test_scan_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "monortm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_build.build_hip())
    for name in SCAN_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/monortm_hip.h"
        assert name in api.SYMBOLS, f"{name} is not bound in api.SYMBOLS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    # host entry: 23 arguments, device entry: the same plus the stream
    assert len(api.SYMBOLS["monortm_hip_rtm_scan"][1]) == 23
    assert len(api.SYMBOLS["monortm_hip_rtm_scan_dev"][1]) == 24


def test_plane_parallel_path_values():
    f = api.plane_parallel_path([0.0, 60.0, 75.0], 7)
    assert f.shape == (3, 7) and f.dtype == np.float64 and f.flags.c_contiguous
    np.testing.assert_allclose(f[0], 1.0, rtol=0, atol=0)
    np.testing.assert_allclose(f[1], 2.0, rtol=1e-15)
    np.testing.assert_allclose(f[2], 1.0 / np.cos(np.deg2rad(75.0)), rtol=1e-15)
    assert api.plane_parallel_path(30.0, 2).shape == (1, 2)   # a scalar is one path


@pytest.mark.parametrize("bad", [[90.0], [-1.0], [10.0, 120.0], [float("nan")], [float("inf")], []])
def test_plane_parallel_path_refuses(bad):
    with pytest.raises(ValueError):
        api.plane_parallel_path(bad, 4)


def test_plane_parallel_path_refuses_shapes():
    with pytest.raises(ValueError):
        api.plane_parallel_path([[10.0, 20.0]], 4)
    with pytest.raises(ValueError):
        api.plane_parallel_path([10.0], 0)


@pytest.fixture(scope="module")
def oracle_case(workdir):
    """The line list and channels of tests/test_jacobian.py::case."""
    from oracle.pyoracle import Oracle

    t3 = f"{workdir}/TAPE3_scan_cpu"
    tape3.write_tape3(t3, synth.synthetic_lines(300, seed=777, lc_frac=0.5, sdep_frac=0.2))
    wn = np.unique(np.concatenate([synth.c2_channels(12, seed=11), synth.sounder_channels()]))
    orc = Oracle(t3, wn[0], wn[-1])
    yield wn, orc
    orc.close()


def scaled(pr, s):
    """The profile with every amount of layer l multiplied by s[l]; P, T, TZ as they were."""
    q = copy.deepcopy(pr)
    s = np.asarray(s, np.float64)
    q.wkl = pr.wkl * s[:, None]
    q.wbrodl = pr.wbrodl * s
    q.clw = pr.clw * s
    if getattr(pr, "xamnt", None) is not None:
        q.xamnt = pr.xamnt * s[:, None]
    return q


@pytest.mark.parametrize("kind", ["uniform", "per_layer"])
def test_premise_modm_is_linear_in_layer_amounts(oracle_case, kind):
    """MODM of amounts scaled per layer = s x O of the unscaled run at rtol 1e-13 (number density and mixing ratios depend on P, T
    and amount ratios only; every term of O is proportional to an amount).  Observed: 8.9e-16."""
    wn, orc = oracle_case
    rng = np.random.default_rng(4)
    worst = 0.0
    for i, irt in zip((500, 501, 502), (1, 3, 2)):
        pr = synth.perturbed_profile(i, wn, nlay=20, cloud=True, irt=irt)
        s = np.full(20, 2.0) if kind == "uniform" else rng.uniform(1.0, 6.0, 20)
        base, got = orc.run(pr), orc.run(scaled(pr, s))
        want = base.o * s[:, None]
        assert np.all(want > 0)
        worst = max(worst, float(np.max(np.abs(got.o - want) / want)))
        np.testing.assert_allclose(got.o, want, rtol=1e-13, atol=0)
        np.testing.assert_allclose(got.o_clw, base.o_clw * s[:, None], rtol=1e-13, atol=0)
    print(f"premise ({kind}): worst relative difference {worst:.2e}")


def test_scan_bench_builds_its_workload():
    """tools/scan_bench.py imports, and its workload is the headline batch of bench.py (configs[3]: 1024 profiles x 64 layers x 50
    channels x 500 lines): everything the tool does before it needs the GPU."""
    spec = importlib.util.spec_from_file_location("scan_bench", os.path.join(ROOT, "tools", "scan_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec, profs, desc = mod.workload()
    assert len(profs) == 1024 and profs[0].nlay == 64 and profs[0].nwn == 50 and rec.n_physical == 500
    assert "configs[3]" in desc
    s = mod.stats([1.0, 2.0, 3.0, 4.0, 10.0])
    assert s == dict(median=3.0, min=1.0, max=10.0, iqr=2.0, n=5)
