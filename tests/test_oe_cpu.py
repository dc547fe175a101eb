"""The optimal-estimation step without a GPU: the long-double truth of tests/oe_truth.py against itself - m-form
against n-form, the identities the diagnostics obey -, the state map of api.oe_state_map, and the two entries of the C ABI in the header
and in the binding."""
import os
import re

import numpy as np
import pytest

import oe_truth as ot
from common import ROOT
from monortm_amd import api

SIZES = [(14, 40), (64, 130)]


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"m{s[0]}-n{s[1]}")
def solved(request):
    m, n = request.param
    c = ot.make_case(m, n, seed=1)
    a = {k: v[0] for k, v in c.items()}
    return a, {g: (ot.step(gamma=g, **a), ot.step_nform(gamma=g, **a)) for g in (0.0, 10.0)}


@pytest.mark.parametrize("gamma", [0.0, 10.0])
def test_m_form_equals_n_form(solved, gamma):
    a, res = solved
    mf, nf = res[gamma]
    scale = np.max(np.abs(mf["x_new"] - a["x"]))
    e = float(np.max(np.abs(mf["x_new"] - nf["x_new"])) / scale)
    print(f"gamma {gamma}: m-form against n-form, x_new {e:.2e} of max |x_new - x|")
    assert e <= 1e-12
    smax = float(np.max(np.diag(a["Sa"])))
    assert float(np.max(np.abs(mf["post_var"] - nf["post_var"]))) <= 1e-12 * smax
    assert float(np.max(np.abs(mf["avk_diag"] - nf["avk_diag"]))) <= 1e-12


@pytest.mark.parametrize("gamma", [0.0, 10.0])
def test_degrees_of_freedom_identity(solved, gamma):
    """sum avk_diag = tr(W M^-1 K) = tr(M^-1 (M - diag se)) = m - tr(M^-1 diag se)."""
    a, res = solved
    mf = res[gamma][0]
    m = len(a["se"])
    Li = ot.solve_lower(mf["L"], np.eye(m, dtype=ot.LD))
    minv_diag = np.sum(Li * Li, axis=0)
    dfs = np.sum(mf["avk_diag"])
    assert abs(dfs - (m - np.sum(minv_diag * a["se"].astype(ot.LD)))) <= 1e-12 * m
    assert 0 < dfs < m


@pytest.mark.parametrize("gamma", [0.0, 10.0])
def test_posterior_variance_is_bounded_by_the_prior(solved, gamma):
    a, res = solved
    pv = res[gamma][0]["post_var"]
    assert np.all(pv > 0) and np.all(pv <= np.diag(a["Sa"]).astype(ot.LD) / (1 + ot.LD(gamma)))


def test_float64_restatement_is_close():
    """The same algebra in float64 numpy stays within 1e-12 of the long-double step: the room the GPU bound leaves."""
    a = {k: v[0] for k, v in ot.make_case(64, 130, seed=2).items()}
    t = ot.step(**a)
    W = a["Sa"] @ a["K"].T
    M = a["K"] @ W + np.diag(a["se"])
    xn = a["x"] + (a["xa"] - a["x"]) + W @ np.linalg.solve(M, (a["y"] - a["F"]) - a["K"] @ (a["xa"] - a["x"]))
    assert float(np.max(np.abs(xn - t["x_new"])) / np.max(np.abs(t["x_new"] - a["x"]))) <= 1e-12


def test_only_the_lower_triangle_of_sa_counts():
    a = {k: v[0] for k, v in ot.make_case(14, 40, seed=3).items()}
    t = ot.step(**a)
    a["Sa"] = np.tril(a["Sa"]) + np.triu(np.full_like(a["Sa"], np.nan), 1)
    u = ot.step(**a)
    assert np.array_equal(t["x_new"], u["x_new"])


# ---- the state map ------------------------------------------------------------------------------------------------------------------------
def test_state_map_resolves_names_orders_and_repeats():
    kind, row = api.oe_state_map([("t", range(3)), ("w", "H2O", [0, 2]), ("w", 7, 1), ("clw", 2), ("tmpsfc",), ("emiss",), ("reflc",), ("tz", [3, 0]),
                                  ("t", 1), ("w", "p", [1])], 3, vars=[7, 1, 1001])
    assert kind.dtype == np.int32 and row.dtype == np.int32
    assert kind.tolist() == [0, 0, 0, 2, 2, 2, 3, 4, 4, 4, 1, 1, 0, 2]
    #                        t        H2O: slot 1     O2: slot 0  clw  sfc      tz     t  p: slot 2
    assert row.tolist() == [0, 1, 2, 0 * 3 + 1, 2 * 3 + 1, 1 * 3 + 0, 2, 0, 1, 2, 3, 0, 1, 1 * 3 + 2]
    k2, r2 = api.oe_state_map([("w", "h2o", 4)], 5, vars=np.array([1], np.int32))
    assert (k2.tolist(), r2.tolist()) == ([2], [4])


@pytest.mark.parametrize("spec", [
    [], "t", [("t",)], [("t", 0, 1)], [("x", 0)], [("t", 3)], [("t", -1)], [("tz", 4)], [("w", "H2O")], [("w", "CO2", 0)], [("w", "nosuch", 0)],
    [("tmpsfc", 0)], [("t", 0.5)], ["t"],
])
def test_state_map_refuses_bad_specs(spec):
    with pytest.raises(ValueError):
        api.oe_state_map(spec, 3, vars=[1])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def declared(name):
    hdr = open(os.path.join(ROOT, "include", "monortm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert found, f"{name} is not declared in include/monortm_hip.h"
    return [a.strip() for a in found.group(1).split(",")]


@pytest.mark.parametrize("name,nargs", [("monortm_hip_oe_step", 28), ("monortm_hip_oe_step_dev", 29)])
def test_header_declares_and_binding_matches(name, nargs):
    args = declared(name)
    assert len(args) == nargs
    assert name in api.SYMBOLS, f"{name} is not bound in monortm_amd/api.py"
    res, types = api.SYMBOLS[name]
    assert len(types) == nargs
    for a, ty in zip(args, types):   # ints are ints, pointers are pointers
        assert ("*" in a) == (ty is not api.C.c_int), (a, ty)


def test_null_context_is_refused():
    lib = api.load_library()
    z = [None] * 20
    assert lib.monortm_hip_oe_step(None, 1, 1, 1, 1, 0, 1, *z[:12], 0, None, 0, *z[:6]) == 6
    assert lib.monortm_hip_oe_step_dev(None, 1, 1, 1, 1, 0, 1, *z[:12], 0, None, 0, *z[:7]) == 6
