"""The cases and the reference of tests/test_jacobian_vars_truth_cpu.py and tests/test_jacobian_vars_truth.py: every Jacobian variable
of DESIGN.md section 3.11 (ln P, ln WBRODL, the seven continuum factors, SCLCPL, SCLHW, Y0RES) and the molecule slots, from the
infrared to the ultraviolet, where each of them is live, against the CPU oracle chained with the closed-form adjoint of the truth.

A helper module like tests/rtm_truth.py and tests/continuum_cases.py (no fixture, no test).  Nothing here runs on a GPU or loads the
product's library: monortm_amd.api is imported for its table of codes and its default step only.

The reference.  MODM is layer-diagonal, so Oracle.run on a profile whose input theta is changed in ALL layers gives every layer's
dO_k/dtheta at once (the CPU tests hold that bit for bit), and rtm_truth.truth_adjoint gives dq/dO_k in closed form, in long double.
A slot [nlay, nwn] of the reference is their product.  dO/dtheta:
  continuum factor i   O is exactly linear in a factor, so dO/dfac_i is a difference of two oracle runs with no step and no truncation:
                       (O(fac) - O(fac with fac_i = 0)) / fac_i, and O(fac_i := 1) - O(fac_i := 0) at fac_i <= eps (the one-sided
                       rule of DESIGN 3.11, eps = api.JAC_DLNW).  Taken literally that differences two TOTALS, each rounded to
                       1.1e-16 O, and resolves a term that is the share c of O to ~1e-16 / c only: Rayleigh in the infrared
                       fixtures (1e-11 .. 1e-10 of O) to 2.3e-6 in the tests' measure, XSELF at 17000 cm-1 to 1.7e-6 - more than
                       the bound.  The reference therefore takes the same difference at fac_i := GAIN = 1e8,
                       (O(fac_i := GAIN) - O(fac_i := 0)) / GAIN: the same number by the same linearity, resolved on the term's
                       own scale.  d_factor(gain=None) is the literal rule; the CPU tests print how far the two are apart.
  ln P, ln WBRODL,     central differences over theta x exp(+-h), h = 1e-3 and 2e-3, Richardson-extrapolated ((4 D(h) - D(2h)) / 3,
  ln WKL of a molecule truncation O(h^4)).
  SCLCPL, SCLHW, Y0RES the same over theta +- h s with the parameter's natural scale s: 1 for the two factors; Y0_SCALE = 0.1 for
                       Y0RES, which is 0 by default - it is added to the coupling coefficient Y (AIP SCLCPL + Y0RES), and |Y(296 K)|
                       of the O2 60 GHz complex of the real_like list is 0.02 .. 0.25.
Every finite-difference reference comes with its SELF-SPREAD: the same slot from h = 5e-4 and 1e-3 against it, in the measure of the
tests (rel_err with w_floor of tests/test_jacobian.py).  A difference of optical depths resolves a term that is the share c of O_k to
~1e-13 / c; the spread shows where that, not the kernel, limits a comparison.

Bound of a (case, variable, profile): the project's 1e-6, or 10 x the reference's self-spread where that is larger (bound()).  The
exact-linear references have no spread: 1e-6 flat.
"""
from __future__ import annotations

import dataclasses
import os

import numpy as np

import rtm_truth
from common import Golden
from monortm_amd import api, synth, tape3
from test_jacobian import rel_err, w_floor   # the measure every k_w slot of the project is held in, unchanged (loads nothing at import)

FIXTURES = ("ir_o2_fundamental", "ir_n2_fundamental_co2", "ir_n2_overtone", "nir_o2_bands", "vis_o2_aband_chappuis",
            "vis_grid_chappuis", "uv_hartley_huggins", "uv_40800_seam", "fuv_schumann_runge")
MW = "mw_real_like"
NAMES = FIXTURES + (MW,)
FACTORS = ("xself", "xfrgn", "xco2c", "xo3cn", "xo2cn", "xn2cn", "xrayl")
MOLS = (1, 2, 3, 7)
IR_VARS = MOLS + ("p", "wbrod") + FACTORS                        # 6 per-layer variables: 3 profiles x (3 + 2 x 6) = 45 states <= 64
MW_VARS = ("p", "wbrod", "sclcpl", "sclhw", "y0res", 1, 7)
ALL_VARS = IR_VARS + ("sclcpl", "sclhw", "y0res")
EPS = api.JAC_DLNW
H = 1e-3
Y0_SCALE = 0.1
SCALE = {"sclcpl": 1.0, "sclhw": 1.0, "y0res": Y0_SCALE}
NLAYS = (None, 5, 1)                                             # profile 0: the fixture's own (8 layers); two synthetic ones
EDGE_CASES = ("vis_o2_aband_chappuis", "ir_n2_fundamental_co2")
EDGE_FACTORS = {"zero": 0.0, "inside": 5e-5}                     # 5e-5 lies inside (0, eps]: both take the one-sided rule
TOL = 1e-6
GAIN = 1e8
# (case, variable) left out of a case's list because the finite-difference reference does not settle there (its self-spread on a strong
# slot exceeds 1e-7 at every step; tests/test_jacobian_vars_truth_cpu.py::test_self_spreads).  ln P on the DVSET grid: in the lowest
# layer at 17100 cm-1 H2O's O(P) is not smooth at the 1e-6 level (a switch of the line shape, by the look of it) - D(h) of that cell
# runs 2.1e-6, 2.0e-6, 1.1e-6, 0, -5.2e-6 of the column's peak from D(1e-3) at h = 1.25e-4 .. 2e-3, no h^2 law below 5e-4 - and the
# slot's spread is 1.5e-7 - 3.6e-7 on a slot of 3.3 K; a smaller step does not mend a difference that does not converge.
# ln P is asserted in the other nine cases.
DROPPED = {("vis_grid_chappuis", "p")}


def var_name(v) -> str:
    return v if isinstance(v, str) else f"mol{v}"


@dataclasses.dataclass
class Case:
    name: str
    seed: int
    tape3: str
    wn: np.ndarray
    profiles: list               # three profiles; MODM takes the factors and scalars of profiles[0], all carry the same
    variables: tuple

    def extra_profiles(self, n: int) -> list:
        """n more profiles of 2 .. 7 layers behind the three (the call of more than 64 per-layer states)."""
        return [self._synthetic(3 + i, 2 + (3 * i) % 6, irt=(1, 3)[i % 2]) for i in range(n)]

    def _synthetic(self, i, nlay, irt):
        p0 = self.profiles[0]
        pr = synth.perturbed_profile(self.seed * 1000 + i, self.wn, nlay=nlay, cloud=(i % 2 == 1), irt=irt)
        return dataclasses.replace(pr, dvset=p0.dvset, cntnm=p0.cntnm.copy(), sclcpl=p0.sclcpl, sclhw=p0.sclhw, y0res=p0.y0res)


def scalars_of(seed: int) -> dict:
    """The seeded factors in (0.3, 1.7) and the scalars a few percent off their defaults (Y0RES: of its scale)."""
    rng = np.random.default_rng(seed)
    fac = rng.uniform(0.3, 1.7, 7)
    off = rng.uniform(0.02, 0.05, 3) * rng.choice([-1.0, 1.0], 3)
    return dict(cntnm=fac, sclcpl=1.0 + off[0], sclhw=1.0 + off[1], y0res=off[2] * Y0_SCALE)


def build_case(name: str, tmpdir: str) -> Case:
    seed = 9100 + NAMES.index(name)
    sc = scalars_of(seed)
    if name == MW:
        rec, kw, _ = synth.real_like_file()
        t3 = os.path.join(tmpdir, "TAPE3_jvar_real_like")
        if not os.path.exists(t3):
            tape3.write_tape3(t3, rec, **kw)
        wn = synth.sounder_channels()[[4, 6, 10, 16, 21, 27, 35]]
        p0 = dataclasses.replace(synth.perturbed_profile(seed * 1000, wn, nlay=8, cloud=True, irt=3), **sc)
        variables = MW_VARS
    else:
        g = Golden(name, tmpdir)
        t3 = g.tape3
        p0 = dataclasses.replace(g.profiles[0], **sc)            # its wavenumbers and its dvset are kept
        wn = p0.wn
        variables = tuple(v for v in IR_VARS if (name, v) not in DROPPED)
    case = Case(name, seed, t3, wn, [p0], variables)
    irt = (1, 3) if p0.irt == 3 else (3, 1)                       # the three profiles carry irt 1 and 3 between them
    for i, n in enumerate(NLAYS[1:]):
        case.profiles.append(case._synthetic(1 + i, n, irt[i]))
    return case


def with_factors(prs: list, value: float) -> list:
    """The batch with all seven factors at `value` (the edge inputs)."""
    return [dataclasses.replace(p, cntnm=np.full(7, value)) for p in prs]


# ---- dO / dtheta from the oracle ----------------------------------------------------------------------------------------------------
def perturbed(pr, var, u: float, layers=None):
    """The profile with variable `var` moved by u: ln P, ln WBRODL, ln WKL of a molecule in `layers` (default: all - the oracle is
    layer-diagonal); SCLCPL, SCLHW, Y0RES by u times the parameter's scale; a continuum factor by u."""
    sel = slice(None) if layers is None else layers
    if var in SCALE:
        return dataclasses.replace(pr, **{var: getattr(pr, var) + u * SCALE[var]})
    if var in FACTORS:
        fac = pr.cntnm.copy()
        fac[FACTORS.index(var)] += u
        return dataclasses.replace(pr, cntnm=fac)
    name = {"p": "p", "wbrod": "wbrodl"}.get(var, "wkl")
    a = getattr(pr, name).copy()
    if name == "wkl":
        a[sel, var - 1] *= np.exp(u)
    else:
        a[sel] *= np.exp(u)
    return dataclasses.replace(pr, **{name: a})


def central(f, pr, var, h: float, layers=None):
    """(f(theta + h) - f(theta - h)) / 2h in the units of perturbed(); f: profile -> array."""
    return (f(perturbed(pr, var, h, layers)) - f(perturbed(pr, var, -h, layers))) / (2 * h * SCALE.get(var, 1.0))


def richardson(f, pr, var, h: float = H, layers=None):
    """-> (the derivative from h and 2h, the same from h / 2 and h): (4 D(h) - D(2h)) / 3, truncation O(h^4)."""
    d = {hh: central(f, pr, var, hh, layers) for hh in (0.5 * h, h, 2 * h)}
    return (4 * d[h] - d[2 * h]) / 3, (4 * d[0.5 * h] - d[h]) / 3


def d_factor(orc, pr, i: int, base_o=None, gain=GAIN) -> np.ndarray:
    """dO/dfac_i [nlay, nwn]: (O(fac_i := gain) - O(fac_i := 0)) / gain; with gain = None the literal rule of the module's docstring
    (differences of the totals at the profile's own factor, one-sided over 1 at fac_i <= eps)."""
    f = float(pr.cntnm[i])
    fac = pr.cntnm.copy()
    fac[i] = 0.0
    off = orc.run(dataclasses.replace(pr, cntnm=fac)).o
    if gain is not None or f <= EPS:
        g = 1.0 if gain is None else float(gain)
        on = fac.copy()
        on[i] = g
        return (orc.run(dataclasses.replace(pr, cntnm=on)).o - off) / g
    return ((orc.run(pr).o if base_o is None else base_o) - off) / f


def d_o(orc, pr, var, base_o=None):
    """-> (dO/dtheta [nlay, nwn], the same from the half steps or None for an exact-linear reference)."""
    if var in FACTORS:
        return d_factor(orc, pr, FACTORS.index(var)), None
    return richardson(lambda p: orc.run(p).o, pr, var)


def k_o(pr, o, quantity: str, path=None) -> np.ndarray:
    """dq/dtau of the truth in closed form at the optical depths o [nlay, nwn] (longdouble): [nlay, nwn], or along the slant paths
    path [npath, nlay] (tau = path x o): [npath, nlay, nwn]."""
    f = np.ones((1, pr.nlay)) if path is None else np.asarray(path, np.float64)
    n = len(f)
    rep = lambda a: np.repeat(np.asarray(a)[None], n, axis=0)  # noqa: E731
    res = rtm_truth.truth_adjoint(pr.wn, [pr.nlay] * n, [pr.irt] * n, rep(pr.t), rep(pr.tz), f[:, :, None] * o[None], [pr.tmpsfc] * n,
                                  rep(pr.emiss), rep(pr.reflc), quantities=(quantity,))[quantity]["k_o"]
    return res[0] if path is None else res


@dataclasses.dataclass
class Ref:
    slots: dict                  # variable -> float64 [nlay, nwn] ([npath, nlay, nwn] with a path)
    spread: dict                 # variable -> the self-spread of a finite-difference reference, None for an exact-linear one
    o: np.ndarray                # the oracle's base O [nlay, nwn]
    q: np.ndarray                # the truth's quantity at that O

    def peak(self, var) -> float:
        return float(np.abs(self.slots[var]).max())

    def bound(self, var) -> float:
        s = self.spread[var]
        return TOL if s is None else max(TOL, 10.0 * s)


def reference(orc, pr, variables, quantity: str = "tb", path=None) -> Ref:
    """Per variable the slot = truth_adjoint(...)[quantity]["k_o"] x dO/dtheta, truth_adjoint evaluated at the oracle's base O; with
    path [npath, nlay]: truth_adjoint at path x O, times path x dO/dtheta (what scan_jacobian's k_w holds)."""
    base = orc.run(pr)
    assert np.isfinite(base.o).all() and np.isfinite(getattr(base, quantity)).all(), "the oracle's base state is not finite"
    ko = k_o(pr, base.o, quantity, path)
    w = ko if path is None else ko * np.asarray(path, np.float64)[:, :, None]
    slots, spread = {}, {}
    for v in variables:
        do, half = d_o(orc, pr, v, base.o)
        slots[v] = np.asarray(w * do, np.float64)
        spread[v] = None
        if half is not None:
            s2 = np.asarray(w * half, np.float64)
            spread[v] = rel_err(s2, slots[v], axis=-2, floor=w_floor(slots[v])) if np.abs(slots[v]).max() > 0 else float(np.abs(s2).max())
    q = rtm_truth.truth(pr.wn, [pr.nlay], [pr.irt], pr.t[None], pr.tz[None], base.o[None], [pr.tmpsfc], pr.emiss[None], pr.reflc[None])[quantity][0]
    return Ref(slots, spread, base.o, np.asarray(q, np.float64))


def check_slot(got, ref: Ref, var, what: str) -> float:
    """A kernel's slot against the reference's: exactly 0 where the reference is identically 0 (a variable that reaches nothing gives
    O+ = O- bit for bit), else rel_err with w_floor within the bound.  -> the error, after printing it."""
    r = ref.slots[var]
    if ref.peak(var) == 0.0:
        assert np.all(got == 0), f"{what} {var_name(var)}: the reference is identically 0, the slot is not (peak {np.abs(got).max():.3e})"
        print(f"{what} {var_name(var)}: dead, exactly 0")
        return 0.0
    e = rel_err(got, r, axis=-2, floor=w_floor(r))
    print(f"{what} {var_name(var)}: peak {ref.peak(var):.3e} error {e:.2e} bound {ref.bound(var):.1e}"
          + ("" if ref.spread[var] is None else f" (self-spread {ref.spread[var]:.1e})"))
    assert e <= ref.bound(var), f"{what} {var_name(var)}: {e:.3e} > {ref.bound(var):.1e}"
    return e


# ---- the cases and their references, computed once per session ------------------------------------------------------------------------
_CASES: dict = {}
_ORACLES: dict = {}
_REFS: dict = {}


def case(name: str, tmpdir: str) -> Case:
    if name not in _CASES:
        _CASES[name] = build_case(name, tmpdir)
    return _CASES[name]


def oracle_of(c: Case):
    from oracle.pyoracle import Oracle

    if c.name not in _ORACLES:
        _ORACLES[c.name] = Oracle(c.tape3, c.wn[0], c.wn[-1])
    return _ORACLES[c.name]


def case_reference(name: str, tmpdir: str, quantity: str = "tb", edge: str | None = None) -> list:
    """[Ref per profile] of a case's three profiles: every variable of the case, or with edge = "zero" / "inside" the seven factors on
    the batch whose factors are all 0 / all 5e-5."""
    key = (name, quantity, edge)
    if key not in _REFS:
        c = case(name, tmpdir)
        prs = c.profiles if edge is None else with_factors(c.profiles, EDGE_FACTORS[edge])
        _REFS[key] = [reference(oracle_of(c), p, c.variables if edge is None else FACTORS, quantity) for p in prs]
    return _REFS[key]
