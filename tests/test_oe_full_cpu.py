"""The full optimal-estimation step without a GPU: the long-double step_full of tests/oe_full_truth.py against
the independent n-form with a full Se, the identities its matrices obey, the generator's condition bounds at every shape the GPU tests
use, and what the Python wrappers decide before any device is touched: the Se dispatch and their ValueErrors."""
import os
import re

import numpy as np
import pytest

import oe_full_truth as oft
import oe_truth as ot
from common import ROOT
from monortm_amd import api
from test_oe_step import MSHAPES

SIZES = [(5, 9), (14, 40), (64, 130)]


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"m{s[0]}-n{s[1]}")
def solved(request):
    m, n = request.param
    c = oft.make_case(m, n, seed=1)
    a = {k: v[0] for k, v in c.items()}
    return a, {g: (oft.step_full(gamma=g, **a), oft.nform_full(gamma=g, **a)) for g in (0.0, 3.0)}


@pytest.mark.parametrize("gamma", [0.0, 3.0])
def test_m_form_equals_n_form_with_a_full_se(solved, gamma):
    """G, A and S_hat - and x_new - under the bounds tests/test_oe_cpu.py holds the diagonal case to: 1e-12 of the largest step, of
    max Sa_ii and absolute for the averaging kernel; the gain within 1e-12 of its largest element."""
    a, res = solved
    mf, nf = res[gamma]
    e = float(np.max(np.abs(mf["x_new"] - nf["x_new"])) / np.max(np.abs(mf["x_new"] - a["x"])))
    eg = float(np.max(np.abs(mf["gain_t"].T - nf["gain"])) / np.max(np.abs(nf["gain"])))
    ea = float(np.max(np.abs(mf["avk"] - nf["avk"])))
    es = float(np.max(np.abs(mf["post_cov"] - nf["post_cov"])) / np.max(np.diag(a["Sa"])))
    print(f"gamma {gamma}: m-form against n-form, x_new {e:.2e}, gain {eg:.2e}, avk {ea:.2e}, post_cov {es:.2e}")
    assert e <= 1e-12 and eg <= 1e-12 and ea <= 1e-12 and es <= 1e-12
    assert abs(mf["dofs"] - np.trace(nf["avk"])) <= 1e-12 * len(a["x"])


@pytest.mark.parametrize("gamma", [0.0, 3.0])
def test_posterior_covariance_is_symmetric_and_its_diagonals_are_the_vectors(solved, gamma):
    mf = solved[1][gamma][0]
    assert np.array_equal(mf["post_cov"], mf["post_cov"].T)
    assert np.array_equal(np.diag(mf["post_cov"]), mf["post_var"]) and np.array_equal(np.diag(mf["avk"]), mf["avk_diag"])
    ev = np.linalg.eigvalsh(np.asarray(mf["post_cov"], np.float64))
    assert ev[0] > -1e-12 * ev[-1]                 # positive semi-definite up to the rounding of the float64 eigensolver


@pytest.mark.parametrize("gamma", [0.0, 10.0])
def test_diagonal_se_gives_the_diagonals_of_the_diagonal_step(gamma):
    """With a diagonal Se - as variances and as a matrix - diag(avk), diag(post_cov), x_new and chi2 are those of oe_truth.step."""
    a = {k: v[0] for k, v in ot.make_case(14, 40, seed=4).items()}
    t = ot.step(gamma=gamma, **a)
    se = a.pop("se")
    smax = np.max(np.diag(a["Sa"]))
    for Se in (se, np.diag(se)):
        f = oft.step_full(Se=Se, gamma=gamma, **a)
        assert float(np.max(np.abs(np.diag(f["post_cov"]) - t["post_var"]))) <= 1e-16 * smax
        assert float(np.max(np.abs(np.diag(f["avk"]) - t["avk_diag"]))) <= 1e-16
        assert float(np.max(np.abs(f["x_new"] - t["x_new"]))) <= 1e-16 * float(np.max(np.abs(t["x_new"] - a["x"])))
        assert abs(f["chi2"] - t["chi2"]) <= 1e-16 * t["chi2"]
        assert abs(f["dofs"] - np.sum(t["avk_diag"])) <= 1e-16 * len(se)


def test_only_the_lower_triangles_count():
    a = {k: v[0] for k, v in oft.make_case(14, 40, seed=3).items()}
    t = oft.step_full(**a)
    for k in ("Sa", "Se"):
        a[k] = np.tril(a[k]) + np.triu(np.full_like(a[k], np.nan), 1)
    u = oft.step_full(**a)
    for k in ("x_new", "gain_t", "avk", "post_cov", "chi2"):
        assert np.array_equal(t[k], u[k]), k


def test_an_indefinite_se_is_an_error_of_the_truth():
    a = {k: v[0] for k, v in oft.make_case(5, 9, seed=2).items()}
    a["Se"][3, 1] = a["Se"][1, 3] = 10.0 * np.max(np.diag(a["Se"]))
    with pytest.raises(ArithmeticError):
        oft.step_full(**a)


@pytest.mark.parametrize("n", oft.NFULL)
@pytest.mark.parametrize("nview,nchan", MSHAPES)
def test_generator_keeps_its_condition_bounds_at_the_gpu_shapes(nview, nchan, n):
    """full_se asserts cond(M) < 1e4 and cond(Se) < 1e3 itself; here for the two cases of the truth test at every shape."""
    worst = [0.0, 0.0]
    for kw in (dict(seed=0), dict(seed=1, shared_sa=True, shared_se=True)):
        c = oft.make_gpu_case(nview, nchan, n, **kw)
        for p in range(3):
            M = c["K"][p] @ c["Sa"][p] @ c["K"][p].T + c["Se"][p]
            worst = [max(worst[0], np.linalg.cond(M)), max(worst[1], np.linalg.cond(c["Se"][p]))]
    print(f"m {nview * nchan} n {n}: worst cond(M) {worst[0]:.3g}, cond(Se) {worst[1]:.3g}")
    assert worst[0] < 1e4 and worst[1] < 1e3


# ---- the Python wrappers, before any device ---------------------------------------------------------------------------------------------
def test_se_shape_selects_kind_and_sharing():
    assert api.oe_se_kind((30,), 3, 30) == (0, 0)
    assert api.oe_se_kind((3, 30), 3, 30) == (0, 1)
    assert api.oe_se_kind((30, 30), 3, 30) == (1, 0)
    assert api.oe_se_kind((3, 30, 30), 3, 30) == (1, 1)
    assert api.oe_se_kind((1,), 1, 1) == (0, 0) and api.oe_se_kind((1, 1, 1), 1, 1) == (1, 1)
    assert api.oe_se_kind((4, 4, 4), 4, 4) == (1, 1) and api.oe_se_kind((4,), 4, 4) == (0, 0)
    assert api.oe_se_kind((4, 4), 4, 4, se_kind=0) == (0, 1) and api.oe_se_kind((4, 4), 4, 4, se_kind=1) == (1, 0)      # said, not guessed
    assert api.oe_se_kind((30, 30), 3, 30, se_kind=1) == (1, 0)
    for shape, kind in (((30, 30), 0), ((30,), 1), ((3, 30), 1), ((30,), 2)):
        with pytest.raises(ValueError):
            api.oe_se_kind(shape, 3, 30, se_kind=kind)


@pytest.mark.parametrize("shape,nprof,m", [((4, 4), 4, 4), ((1, 1), 1, 1), ((29,), 3, 30), ((30, 3), 3, 30), ((3, 30, 29), 3, 30), ((2, 30, 30), 3, 30),
                                           ((), 3, 30), ((3, 3, 30, 30), 3, 30)])
def test_se_shapes_that_are_refused(shape, nprof, m):
    """[m, m] with nprof = m is both a matrix and per-profile variances: ambiguous; the others fit nothing."""
    with pytest.raises(ValueError):
        api.oe_se_kind(shape, nprof, m)


def test_unknown_diagnostics_are_refused():
    assert api._oe_want(("dofs", "avk")) == ("avk", "dofs") and api._oe_want("gain_t") == ("gain_t",) and api._oe_want(()) == ()
    with pytest.raises(ValueError):
        api._oe_want(("avk", "gain"))


def test_wrappers_refuse_before_any_device():
    """MonoRTM.oe_step_full checks Se's shape and `want` before it touches its context; DeviceBatch.retrieve wants one of se and Se."""
    rt = object.__new__(api.MonoRTM)               # no context: whatever reached the library would fail on the missing attributes
    jac = dict(k_t=np.zeros((2, 1, 3, 4)), k_tz=np.zeros((2, 1, 4, 4)), k_clw=np.zeros((2, 1, 3, 4)), k_sfc=np.zeros((2, 1, 3, 4)), y=np.zeros((2, 1, 4)))
    args = (jac, [("t", range(3))], np.zeros((2, 1, 4)), np.zeros((2, 3)), np.zeros((2, 3)), np.eye(3))
    with pytest.raises(ValueError, match="Se must be"):
        api.MonoRTM.oe_step_full(rt, *args, np.ones(5))
    with pytest.raises(ValueError, match="Se must be"):
        api.MonoRTM.oe_step_full(rt, *args, np.ones((4, 4, 4)))
    with pytest.raises(ValueError, match="unknown diagnostics"):
        api.MonoRTM.oe_step_full(rt, *args, np.ones(4), want=("avk", "cov"))
    db = object.__new__(api.DeviceBatch)
    for kw in (dict(), dict(se=np.ones(4), Se=np.eye(4))):
        with pytest.raises(ValueError, match="se .* or Se"):
            api.DeviceBatch.retrieve(db, None, None, 0, [("t", range(3))], None, None, **kw)
    with pytest.raises(ValueError, match="unknown diagnostics"):
        api.DeviceBatch.retrieve(db, None, None, 0, [("t", range(3))], None, None, np.ones(4), diagnostics=("avk_diag",))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def declared(name):
    hdr = open(os.path.join(ROOT, "include", "monortm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert found, f"{name} is not declared in include/monortm_hip.h"
    return [a.strip() for a in found.group(1).split(",")]


@pytest.mark.parametrize("name,nargs", [("monortm_hip_oe_step_full", 33), ("monortm_hip_oe_step_full_dev", 34)])
def test_header_declares_and_binding_matches(name, nargs):
    args = declared(name)
    assert len(args) == nargs
    assert name in api.SYMBOLS, f"{name} is not bound in monortm_amd/api.py"
    _, types = api.SYMBOLS[name]
    assert len(types) == nargs
    for a, ty in zip(args, types):   # ints are ints, pointers are pointers
        assert ("*" in a) == (ty is not api.C.c_int), (a, ty)
    old = declared(name.replace("_full", ""))      # the arguments of the step's entry, with Se, se_kind in place of se
    i = old.index("const monortm_real *se")
    assert args[:i] == old[:i] and args[i: i + 2] == ["const monortm_real *Se", "int se_kind"] and args[i + 2: i + 9] == old[i + 1: i + 8]


def test_null_context_is_refused():
    lib = api.load_library()
    z = [None] * 20
    assert lib.monortm_hip_oe_step_full(None, 1, 1, 1, 1, 0, 1, *z[:12], 0, None, 0, 0, *z[:10]) == 6
    assert lib.monortm_hip_oe_step_full_dev(None, 1, 1, 1, 1, 0, 1, *z[:12], 0, None, 1, 0, *z[:11]) == 6
