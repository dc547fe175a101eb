"""The adaptive retrieval loop without a GPU: the long-double functions of tests/oe_lm_truth.py - the
specification of the step's dual vector, the scatter and the decision - checked against Sa^-1 formed explicitly, the n-form cost, a whole
loop on a toy nonlinear forward model, every branch of the decision, and what the Python layer decides before any device."""
import os
import re

import numpy as np
import pytest

import oe_full_truth as oft
import oe_lm_truth as lt
import oe_truth as ot
from common import ROOT
from monortm_amd import api
from test_oe_full_cpu import SIZES

LD = ot.LD


# ---- the dual vector and the cost ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["diag", "full"])
@pytest.mark.parametrize("gamma", [0.0, 3.0])
@pytest.mark.parametrize("m,n", SIZES)
def test_dual_vector_follows_the_iterate_and_cost_is_the_n_form_cost(m, n, gamma, full):
    """c = Sa^-1 (x - xa)  =>  c_new = Sa^-1 (x_new - xa), against inverse_spd(Sa): within 1e-12 of max |c_new| (long double, cond(Sa)
    below 1e3 for these priors); cost = chi2 + (x - xa)^T Sa^-1 (x - xa) within 1e-12 relative."""
    a = {k: v[0] for k, v in (oft.make_case(m, n, seed=2) if full else ot.make_case(m, n, seed=2)).items()}
    Se = a.pop("Se") if full else a.pop("se")
    Sai = ot.inverse_spd(oft.sym_lower(a["Sa"]))
    d = np.asarray(a["x"], LD) - np.asarray(a["xa"], LD)
    c = Sai @ d
    t = lt.step_lm(a["K"], a["Sa"], Se, a["xa"], a["x"], a["y"], a["F"], gamma, c)
    want = Sai @ (t["x_new"] - np.asarray(a["xa"], LD))
    e = float(np.max(np.abs(t["c_new"] - want)) / np.max(np.abs(want)))
    J = lt.chi2_of(a["F"], a["y"], Se) + d @ Sai @ d
    ej = float(abs(t["cost"] - J) / J)
    print(f"m {m} n {n} gamma {gamma} {'full' if full else 'diag'}: c_new {e:.2e}, cost {ej:.2e}")
    assert e <= 1e-12 and ej <= 1e-12
    f = oft.step_full(a["K"], a["Sa"], Se, a["xa"], a["x"], a["y"], a["F"], gamma)
    for k in ("x_new", "post_var", "avk_diag", "chi2"):
        assert np.array_equal(t[k], f[k]), k


def test_starting_at_the_prior_the_dual_vector_is_zero_and_absent_is_zero():
    a = {k: v[0] for k, v in ot.make_case(14, 40, seed=5).items()}
    se = a.pop("se")
    a["x"] = a["xa"].copy()
    t0 = lt.step_lm(a["K"], a["Sa"], se, a["xa"], a["x"], a["y"], a["F"], 2.0, None)
    t1 = lt.step_lm(a["K"], a["Sa"], se, a["xa"], a["x"], a["y"], a["F"], 2.0, np.zeros(40))
    assert np.array_equal(t0["c_new"], t1["c_new"]) and t0["cost"] == t0["chi2"] == t1["cost"]


# ---- a whole loop on a toy nonlinear forward model ------------------------------------------------------------------------------------------
def toy(beta, seed=3, m=8, n=6):
    """F(x) = l + beta l^2 with l = A x: linear plus a quadratic term; y is F at a draw from the prior, noise-free."""
    rng = np.random.default_rng(seed)
    A = np.asarray(ot.smooth_k(m, n, rng), LD)
    Sa = ot.blocks_cov(n, rng)
    xa = rng.normal(0.0, 1.0, n)
    xt = xa + np.linalg.cholesky(Sa) @ rng.normal(size=n)

    def forward(x):
        lin = A @ np.asarray(x, LD)
        return lin + beta * lin * lin, (1 + 2 * beta * lin)[:, None] * A

    return forward, forward(xt)[0], Sa, np.full(m, 1e-2), xa


def test_loop_on_a_toy_model_accepts_rejects_converges_and_stalls():
    """beta = 0.2 from gamma 0: the undamped first steps overshoot (rejected, gamma 1, 10, 100), the damped ones descend (accepted, gamma
    halved each time) until J falls by less than conv x m (converged).  The same problem in a box of 1e-9 around the prior with
    gamma_max = 1e3: every trial leaves the box, gamma climbs 1, 10, .. 1e4 and the profile stalls."""
    f, y, Sa, se, xa = toy(0.2)
    st, tr = lt.loop(f, y, Sa, se, xa, 12)
    marks = "".join("A" if t["accepted"] else "R" if t["rejected"] else "-" for t in tr)
    print(marks, [float(t["state"]["J"]) for t in tr])
    assert marks.startswith("RRRA") and st["n_rej"] == 3 and st["n_acc"] >= 5 and st["done"] == 1
    assert [float(t["state"]["gamma"]) for t in tr[:4]] == [1.0, 10.0, 100.0, 50.0]
    J = [float(tr[0]["J_before"])] + [float(t["state"]["J"]) for t in tr]
    assert all(b <= a for a, b in zip(J, J[1:])) and J[-1] < 1e-3 * J[0]          # J_history never rises
    k = next(i for i, t in enumerate(tr) if t["state"]["done"])
    assert tr[k]["accepted"] and tr[k]["J_before"] - tr[k]["J_trial"] <= 0.01 * len(y)
    for t in tr[k + 1:]:                                                          # a finished profile does not move
        assert not t["accepted"] and not t["rejected"] and np.array_equal(t["state"]["x"], tr[k]["state"]["x"])
    for t in tr:                                                                  # a rejected trial raised J (or left the box)
        if t["rejected"]:
            assert not (t["trial_ok"] and t["J_trial"] <= t["J_before"])
    st, tr = lt.loop(f, y, Sa, se, xa, 12, lo=xa - 1e-9, hi=xa + 1e-9, gamma_max=1e3)
    assert st["done"] == 4 and st["n_acc"] == 0 and st["n_rej"] == 5 and float(st["gamma"]) == 1e4 and np.array_equal(st["x"], np.asarray(xa, LD))
    assert not any(t["trial_ok"] for t in tr[:5])
    # out of iterations
    st, _ = lt.loop(f, y, Sa, se, xa, 5)
    assert st["done"] == 3


# ---- the decision, branch by branch -----------------------------------------------------------------------------------------------------------
def test_every_branch_of_the_decision():
    st = dict(x=np.zeros(2), c=np.zeros(2), J=100.0, gamma=4.0, done=0, n_acc=1, n_rej=2)
    xt, ct = np.ones(2), np.full(2, 3.0)
    a = lt.accept(st, xt, ct, 50.0, True, 0, 10)
    assert (a["J"], a["gamma"], a["n_acc"], a["n_rej"], a["done"]) == (50.0, 2.0, 2, 2, 0) and np.array_equal(a["x"], xt) and np.array_equal(a["c"], ct)
    assert lt.accept(st, xt, ct, 99.95, True, 0, 10)["done"] == 1                                  # fell by 0.05 <= 0.01 x 10
    assert lt.accept(dict(st, gamma=1.5e-3), xt, ct, 50.0, True, 0, 10)["gamma"] == 0.0            # through the floor
    r = lt.accept(dict(st, gamma=0.0), xt, ct, 150.0, True, 0, 10)
    assert (r["gamma"], r["n_rej"], r["n_acc"], r["J"], r["done"]) == (1.0, 3, 1, 100.0, 0) and np.array_equal(r["x"], st["x"])
    assert lt.accept(st, xt, ct, 50.0, False, 0, 10)["gamma"] == 40.0                              # outside the box
    assert lt.accept(st, xt, ct, np.nan, True, 0, 10)["n_rej"] == 3
    assert lt.accept(dict(st, gamma=5e7), xt, ct, 150.0, True, 0, 10)["done"] == 4
    f = lt.accept(st, xt, ct, 50.0, True, 1, 10)
    assert f["done"] == 2 and f["n_acc"] == 1 and f["n_rej"] == 2 and f["gamma"] == 4.0
    assert lt.accept(st, xt, ct, 50.0, True, 0, 10, se_bad=True)["done"] == 2
    d = lt.accept(dict(st, done=1), xt, ct, 50.0, True, 0, 10, last=True)
    assert d == dict(st, done=1)
    assert lt.accept(st, xt, ct, 50.0, True, 0, 10, last=True)["done"] == 3 and lt.accept(st, xt, ct, 99.95, True, 0, 10, last=True)["done"] == 1
    assert lt.accept(st, xt, ct, 100.0, True, 0, 10)["n_acc"] == 2                                 # J_trial = J_cur is accepted


# ---- the write map and the scatter ----------------------------------------------------------------------------------------------------------
def test_write_map_and_scatter():
    spec = [("t", range(4)), ("w", "H2O", [0, 1]), ("tz", [2, 4]), ("tmpsfc",), ("t", [1]), ("tz", [4]), ("clw", [3]), ("tmpsfc",)]
    kind, index, mol = wmap = api.oe_write_map(spec, 4, 7)
    assert kind.tolist() == [0, -1, 0, 0, 2, 2, 1, -1, -1, 0, 1, 3, 4]
    assert index.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, -1, 1, 4, 3, 0] and mol.tolist() == [0] * 13
    assert api.oe_write_map([("w", "O3", [1])], 4, 7)[2].tolist() == [2]
    for bad in ([("emiss",)], [("reflc",)], [("w", "p", [0])], [("w", "SO2", [0])]):
        with pytest.raises(ValueError):
            api.oe_write_map(bad, 4, 7)
    nlay = np.array([4, 3])
    rng = np.random.default_rng(1)
    arr = dict(T=rng.normal(size=(2, 4)), TZ=rng.normal(size=(2, 5)), WKL=rng.uniform(1, 2, (2, 4, 7)), CLW=rng.normal(size=(2, 4)), tmpsfc=rng.normal(size=2))
    old = {k: v.copy() for k, v in arr.items()}
    x = rng.normal(size=(2, 13))
    assert lt.scatter(wmap, nlay, arr, x).tolist() == [1, 1]
    assert np.array_equal(arr["T"][0], [x[0, 0], x[0, 9], x[0, 2], x[0, 3]])               # layer 1 from the last column that names it
    assert np.array_equal(arr["T"][1], [x[1, 0], x[1, 9], x[1, 2], old["T"][1, 3]])        # layer 3 of a 3-layer profile is padding
    assert np.array_equal(arr["TZ"][:, 4], [x[0, 10], old["TZ"][1, 4]]) and np.array_equal(arr["TZ"][:, 2], x[:, 6])
    assert np.array_equal(arr["tmpsfc"], x[:, 12]) and arr["CLW"][0, 3] == x[0, 11] and arr["CLW"][1, 3] == old["CLW"][1, 3]
    assert np.array_equal(arr["WKL"][:, :2, 0], np.exp(x[:, 4:6])) and np.array_equal(arr["WKL"][:, :, 1:], old["WKL"][:, :, 1:])
    # the box: a violation in a shadowed column counts where it is live, one in padding does not; the fallback is written
    lo = np.full((2, 13), -np.inf)
    lo[0, 8], lo[1, 3] = x[0, 8] + 1.0, x[1, 3] + 1.0      # profile 0: the first TMPSFC column; profile 1: its padded layer 3
    now = {k: v.copy() for k, v in arr.items()}
    fb = rng.normal(size=(2, 13))
    assert lt.scatter(wmap, nlay, arr, x, fb, None, lo, None).tolist() == [0, 1]
    assert arr["T"][0, 0] == fb[0, 0] and arr["tmpsfc"][0] == fb[0, 12] and all(np.array_equal(arr[k][1], now[k][1]) for k in arr)
    x[1, 5] = np.nan
    assert lt.scatter(wmap, nlay, arr, x, fb, np.array([0, 0])).tolist() == [1, 0]
    assert lt.scatter(wmap, nlay, arr, fb, x, np.array([1, 0])).tolist() == [1, 1] and arr["T"][0, 0] == x[0, 0] and arr["T"][1, 0] == fb[1, 0]


# ---- the Python layer, before any device ------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_before_any_device():
    db = object.__new__(api.DeviceBatch)               # no context: whatever reached the library would fail on the missing attributes
    args = (None, None, 0, [("t", range(3))], None, None)
    for kw in (dict(), dict(se=np.ones(4), Se=np.eye(4))):
        with pytest.raises(ValueError, match="se .* or Se"):
            api.DeviceBatch.retrieve_lm(db, *args, **kw)
    with pytest.raises(ValueError, match="x0 needs c0"):
        api.DeviceBatch.retrieve_lm(db, *args, se=np.ones(4), x0=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="unknown diagnostics"):
        api.DeviceBatch.retrieve_lm(db, *args, se=np.ones(4), diagnostics=("avk_diag",))
    with pytest.raises(ValueError, match="maxit"):
        api.DeviceBatch.retrieve_lm(db, *args, se=np.ones(4), maxit=0)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def declared(name):
    hdr = open(os.path.join(ROOT, "include", "monortm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert found, f"{name} is not declared in include/monortm_hip.h"
    return [a.strip() for a in found.group(1).split(",")]


@pytest.mark.parametrize("name,nargs", [("monortm_hip_oe_step_lm", 36), ("monortm_hip_oe_step_lm_dev", 37), ("monortm_hip_oe_scatter_dev", 27),
                                        ("monortm_hip_oe_accept_dev", 29)])
def test_header_declares_and_binding_matches(name, nargs):
    args = declared(name)
    assert len(args) == nargs
    assert name in api.SYMBOLS, f"{name} is not bound in monortm_amd/api.py"
    _, types = api.SYMBOLS[name]
    assert len(types) == nargs
    for a, ty in zip(args, types):   # scalars are scalars, pointers are pointers
        assert ("*" in a) == (ty not in (api.C.c_int, api.C.c_longlong, api.C.c_double)), (a, ty)
    if "step_lm" in name:            # the arguments of the full step's entry, then c, c_new, cost
        old = declared(name.replace("_lm", "_full"))
        k = len(old) - (1 if name.endswith("_dev") else 0)
        assert args[:k] == old[:k] and args[k: k + 3] == ["const monortm_real *c", "monortm_real *c_new", "monortm_real *cost"] and args[k + 3:] == old[k:]


def test_null_context_is_refused():
    lib = api.load_library()
    z = [None] * 20
    assert lib.monortm_hip_oe_step_lm(None, 1, 1, 1, 1, 0, 1, *z[:12], 0, None, 0, 0, *z[:13]) == 6
    assert lib.monortm_hip_oe_step_lm_dev(None, 1, 1, 1, 1, 0, 1, *z[:12], 0, None, 1, 0, *z[:14]) == 6
    assert lib.monortm_hip_oe_scatter_dev(None, 1, 1, *z[:8], 0, None, 1, 7, None, 1, None, 2, None, 7, None, 1, *z[:4]) == 6
    assert lib.monortm_hip_oe_accept_dev(None, 1, 1, 1, *z[:3], 0, 0, *z[:5], 10.0, 0.5, 1.0, 1e-3, 1e8, 0.01, 0, *z[:8]) == 6
