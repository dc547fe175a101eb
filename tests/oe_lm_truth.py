"""The adaptive retrieval loop of DESIGN.md section 3.15 restated in numpy long double: the specification of monortm_hip_oe_step_lm,
monortm_hip_oe_scatter_dev and monortm_hip_oe_accept_dev, built on oe_truth and oe_full_truth.

step_lm()   step_full plus the dual vector: with c = Sa^-1 (x - xa), u = L^-1 r and b = L^-1 K,
              q = b^T u = K^T M^-1 r,   c_new = (gamma c + q) / (1 + gamma) = Sa^-1 (x_new - xa),   cost = chi2 + c . (x - xa).
            (x_new - xa = g [(x - xa) gamma + Sa K^T M^-1 r]: multiply by Sa^-1.)  Sa^-1 is never formed.
cost_of()   J of a trial: chi2(Y_trial) + c_trial . (x_trial - xa), chi2 as step_full forms it.
accept()    the decision on one profile's trial, on a dict of x, c, J, gamma, done, n_acc, n_rej: returns the new dict.
scatter()   a state vector into resident arrays through a write map (monortm_amd.api.oe_write_map), with the box test.
loop()      the six steps of DeviceBatch.lm_iterate on a forward model given as a function, one profile."""
import numpy as np

import oe_full_truth as oft
import oe_truth as ot

LD = ot.LD
KNOBS = dict(up=10.0, down=0.5, gamma_first=1.0, gamma_floor=1e-3, gamma_max=1e8, conv=0.01)


def step_lm(K, Sa, Se, xa, x, y, F, gamma=0.0, c=None):
    """One profile in long double: the dict of oe_full_truth.step_full plus c_new [n] and cost."""
    t = oft.step_full(K, Sa, Se, xa, x, y, F, gamma)
    K, xa, x, y, F = (np.asarray(a, LD) for a in (K, xa, x, y, F))
    c = np.zeros(len(x), LD) if c is None else np.asarray(c, LD)
    g = LD(1) + LD(gamma)
    r = (y - F) - K @ ((xa - x) / g)
    q = ot.solve_lower(t["L"], K).T @ ot.solve_lower(t["L"], r)
    t.update(c_new=(LD(gamma) * c + q) / g, cost=t["chi2"] + np.sum(c * (x - xa)))
    return t


def chi2_of(Y, y, Se):
    """(y - Y)^T Se^-1 (y - Y): Se [m] variances or [m][m] (lower triangle read); ArithmeticError for an Se that is not positive definite."""
    dy = np.asarray(y, LD) - np.asarray(Y, LD)
    if np.ndim(Se) == 1:
        return np.sum(dy * dy / np.asarray(Se, LD))
    ue = ot.solve_lower(ot.cholesky(oft.sym_lower(Se)), dy)
    return np.sum(ue * ue)


def cost_of(Y_trial, y, Se, c_trial, x_trial, xa):
    return chi2_of(Y_trial, y, Se) + np.sum(np.asarray(c_trial, LD) * (np.asarray(x_trial, LD) - np.asarray(xa, LD)))


def accept(st, x_trial, c_trial, J_trial, trial_ok, step_status, nmeas, last=False, se_bad=False, up=10.0, down=0.5, gamma_first=1.0,
           gamma_floor=1e-3, gamma_max=1e8, conv=0.01):
    """The decision on one profile.  st: dict of x, c, J, gamma, done, n_acc, n_rej - returned as a new dict, st itself unchanged.
    se_bad: the Cholesky of a full Se met a bad pivot."""
    st = dict(st)
    if st["done"] != 0:
        return st
    if step_status == 1 or se_bad:
        st["done"] = 2
        return st
    if trial_ok and np.isfinite(J_trial) and J_trial <= st["J"]:
        dJ = st["J"] - J_trial
        g = st["gamma"] * down
        st.update(x=np.array(x_trial), c=np.array(c_trial), J=J_trial, gamma=g if g >= gamma_floor else 0.0 * g, n_acc=st["n_acc"] + 1)
        if dJ <= conv * nmeas:
            st["done"] = 1
    else:
        g = max(st["gamma"] * up, gamma_first)
        st.update(gamma=g, n_rej=st["n_rej"] + 1)
        if g > gamma_max:
            st["done"] = 4
    if last and st["done"] == 0:
        st["done"] = 3
    return st


def live_columns(wmap, nlay):
    kind, index, _ = wmap
    return (kind == 4) | np.where(kind == 1, index <= nlay, index < nlay)


def scatter(wmap, nlay, arrays, x_src, x_fallback=None, done=None, lo=None, hi=None):
    """One call of the scatter on numpy arrays: arrays is a dict of T [nprof][lm], TZ [nprof][lm + 1], WKL [nprof][lm][nmol], CLW and
    tmpsfc [nprof], changed in place; lo, hi [n] or [nprof][n] or None.  Returns trial_ok int [nprof]."""
    kind, index, mol = wmap
    nprof, n = x_src.shape
    ok = np.ones(nprof, np.int32)
    for p in range(nprof):
        live = live_columns(wmap, nlay[p])
        v = x_src[p]
        inside = np.isfinite(v)
        for b, cmp in ((lo, np.greater_equal), (hi, np.less_equal)):
            if b is not None:
                inside &= cmp(v, b[p] if np.ndim(b) == 2 else b)
        ok[p] = int(np.all(inside[live]))
        src = x_fallback[p] if x_fallback is not None and (not ok[p] or (done is not None and done[p] != 0)) else v
        for i in np.nonzero(live & (kind >= 0))[0]:
            k, ix = kind[i], index[i]
            if k == 0:
                arrays["T"][p, ix] = src[i]
            elif k == 1:
                arrays["TZ"][p, ix] = src[i]
            elif k == 2:
                arrays["WKL"][p, ix, mol[i]] = np.exp(src[i])
            elif k == 3:
                arrays["CLW"][p, ix] = src[i]
            else:
                arrays["tmpsfc"][p] = src[i]
    return ok


def loop(forward, y, Sa, Se, xa, maxit, gamma0=0.0, lo=None, hi=None, **knobs):
    """The loop of one profile on forward(x) -> (F, K), in long double, from x = xa and c = 0.  Returns the final state dict and the
    trace: per iteration a dict of accepted, trial_ok, J_trial, and the state after it."""
    kn = dict(KNOBS, **knobs)
    xa = np.asarray(xa, LD)
    m = len(y)
    st = dict(x=xa.copy(), c=np.zeros(len(xa), LD), J=None, gamma=LD(gamma0), done=0, n_acc=0, n_rej=0)
    trace = []
    for it in range(maxit):
        F, K = forward(st["x"])
        try:
            t, status = step_lm(K, Sa, Se, xa, st["x"], y, F, st["gamma"], st["c"]), 0
        except ArithmeticError:
            t, status = dict(x_new=st["x"], c_new=st["c"], cost=LD(0)), 1
        if it == 0:
            st["J"] = t["cost"]
        ok = bool(np.all(np.isfinite(t["x_new"])) and (lo is None or np.all(t["x_new"] >= lo)) and (hi is None or np.all(t["x_new"] <= hi)))
        Ft, _ = forward(t["x_new"] if ok and st["done"] == 0 else st["x"])
        Jt = cost_of(Ft, y, Se, t["c_new"], t["x_new"], xa)
        new = accept(st, t["x_new"], t["c_new"], Jt, ok, status, m, last=it + 1 == maxit, **kn)
        trace.append(dict(accepted=new["n_acc"] > st["n_acc"], rejected=new["n_rej"] > st["n_rej"], trial_ok=ok, J_trial=Jt, J_before=st["J"],
                          state=new))
        st = new
    return st, trace
