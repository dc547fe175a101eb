"""Python binding of the C ABI (include/monortm_hip.h) - the same entry points the Fortran shim binds.

Two layers:
  * :class:`MonoRTM` - host-buffer calls (numpy in, numpy out) = exactly what
    ``ModmMod::MODM`` / ``RTMmono::RTM`` / ``RTMmono::CALCTMR`` of the Fortran shim do;
  * :class:`DeviceBatch` - a batch of profiles resident in HBM (torch tensors are only the owners of
    the device memory / stream), used by bench.py and the multi-GPU driver.

There is NO CPU fallback: if the HIP library is missing or no GPU is visible every call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build
from .caseio import Dump
from .synth import Profile

NCONT = 5
ERRORS = {1: "EIO", 2: "EFORMAT", 3: "EUNSUPPORTED", 4: "ETEMP", 5: "ESDV", 6: "EARG", 7: "EHIP"}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

# every symbol include/monortm_hip.h declares: (restype, argtypes)
SYMBOLS = {
    "monortm_hip_init": (C.c_int, [C.c_char_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "monortm_hip_init_multi": (C.c_int, [C.c_char_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "monortm_hip_device_count": (C.c_int, [_vp]),
    "monortm_hip_finalize": (None, [_vp]),
    "monortm_hip_last_error": (C.c_char_p, [_vp]),
    "monortm_hip_line_count": (C.c_longlong, [_vp, C.c_int]),
    "monortm_hip_has_lines": (C.c_int, [_vp]),
    "monortm_hip_xsec_regions": (C.c_int, [_vp]),
    "monortm_hip_counter": (C.c_longlong, [_vp, C.c_int]),
    "monortm_hip_kat": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "monortm_hip_tape3_probe": (C.c_int, [C.c_char_p, C.c_double, C.c_double, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                          C.POINTER(C.c_longlong)]),
    "monortm_hip_modm": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                   C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "monortm_hip_set_option": (C.c_int, [_vp, C.c_char_p, C.c_char_p]),
    "monortm_hip_comm_unique_id": (C.c_int, [_vp]),
    "monortm_hip_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "monortm_hip_gather_dev": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_int, _vp]),
    "monortm_hip_xsec_tables": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_longlong]),
    "monortm_hip_modm_xs": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                      C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "monortm_hip_modm_xs_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp,
                                          _vp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp]),
    "monortm_hip_rtm": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp]),
    "monortm_hip_modm_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp,
                                       _vp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "monortm_hip_rtm_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "monortm_hip_rtm_scan": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int]
                             + [_vp] * 8),
    "monortm_hip_rtm_scan_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int]
                                 + [_vp] * 9),
    "monortm_hip_rtm_jac": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int] + [_vp] * 12),
    "monortm_hip_rtm_jac_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int] + [_vp] * 13),
    "monortm_hip_jacobian": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                       C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp]
                             + [_vp] * 9),
    "monortm_hip_jacobian_xs": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                          C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                              C.c_int, _vp]
                                + [_vp] * 9),
    "monortm_hip_jacobian_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                           C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp]
                                 + [_vp] * 11),
    "monortm_hip_jacobian_xs_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                              C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                              C.c_int, _vp]
                                    + [_vp] * 11),
    "monortm_hip_rtm_scan_jac": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int]
                                 + [_vp] * 9),
    "monortm_hip_rtm_scan_jac_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp,
                                               C.c_int] + [_vp] * 10),
    "monortm_hip_scan_jacobian": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                            C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp,
                                            C.c_int, _vp, C.c_int] + [_vp] * 10),
    "monortm_hip_scan_jacobian_xs": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                               C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                              C.c_int, _vp,
                                               C.c_int, _vp, C.c_int] + [_vp] * 10),
    "monortm_hip_scan_jacobian_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                                C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp,
                                                C.c_int, _vp, C.c_int] + [_vp] * 12),
    "monortm_hip_scan_jacobian_xs_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                                   C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                              C.c_int, _vp,
                                                   C.c_int, _vp, C.c_int] + [_vp] * 12),
    "monortm_hip_obs_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _ip]),
    "monortm_hip_obs_destroy": (C.c_int, [_vp, C.c_int]),
    "monortm_hip_rtm_obs_jac": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                          _vp, _vp, C.c_int] + [_vp] * 4),
    "monortm_hip_rtm_obs_jac_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp,
                                              C.c_int, _vp, _vp, C.c_int] + [_vp] * 5),
    "monortm_hip_obs_jacobian": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                           C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp,
                                           C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 7),
    "monortm_hip_obs_jacobian_xs": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                              C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                              C.c_int, _vp,
                                              C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 7),
    "monortm_hip_obs_jacobian_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                               C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp,
                                               C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 9),
    "monortm_hip_obs_jacobian_xs_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                              C.c_int, _vp,
                                                  C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 9),
    "monortm_hip_rtm_obs": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                      _vp, _vp, C.c_int, _vp, _vp]),
    "monortm_hip_rtm_obs_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                          _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "monortm_hip_obs": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                  C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int,
                                  C.c_int, _vp, _vp, _vp]),
    "monortm_hip_obs_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                      C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int,
                                      C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "monortm_hip_oe_step": (C.c_int, [_vp] + [C.c_int] * 6 + [_vp] * 12 + [C.c_int, _vp, C.c_int] + [_vp] * 6),
    "monortm_hip_oe_step_dev": (C.c_int, [_vp] + [C.c_int] * 6 + [_vp] * 12 + [C.c_int, _vp, C.c_int] + [_vp] * 7),
    "monortm_hip_oe_step_full": (C.c_int, [_vp] + [C.c_int] * 6 + [_vp] * 12 + [C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 10),
    "monortm_hip_oe_step_full_dev": (C.c_int, [_vp] + [C.c_int] * 6 + [_vp] * 12 + [C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 11),
    "monortm_hip_oe_step_lm": (C.c_int, [_vp] + [C.c_int] * 6 + [_vp] * 12 + [C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 13),
    "monortm_hip_oe_step_lm_dev": (C.c_int, [_vp] + [C.c_int] * 6 + [_vp] * 12 + [C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 14),
    "monortm_hip_oe_scatter_dev": (C.c_int, [_vp, C.c_int, C.c_int] + [_vp] * 8 + [C.c_int, _vp, C.c_int, C.c_int] + [_vp, C.c_longlong] * 4 + [_vp] * 4),
    "monortm_hip_oe_accept_dev": (C.c_int, [_vp] + [C.c_int] * 3 + [_vp] * 3 + [C.c_int] * 2 + [_vp] * 5 + [C.c_double] * 6 + [C.c_int] + [_vp] * 8),
    "monortm_hip_check": (C.c_int, [_vp, _vp]),
    "monortm_hip_profile": (C.c_int, [_vp, C.c_int]),
    "monortm_hip_kernel_time": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(C.c_longlong)]),
}

_LIB = None

# half-steps of the Jacobian's central differences (include/monortm_hip.h MONORTM_JAC_DT / MONORTM_JAC_DLNW; set_option "jac_dt" /
# "jac_dlnw" changes them per context)
JAC_DT = 1e-2
JAC_DLNW = 1e-4
# Jacobian variables besides the 1-based molecules (MONORTM_JVAR_* of include/monortm_hip.h): ln P and
# ln WBRODL per layer, and the scalar arguments of MODM - the seven continuum factors, SCLCPL, SCLHW, Y0RES
JAC_VARS = {"p": 1001, "wbrod": 1002, "xself": 1011, "xfrgn": 1012, "xco2c": 1013, "xo3cn": 1014, "xo2cn": 1015, "xn2cn": 1016,
            "xrayl": 1017, "sclcpl": 1021, "sclhw": 1022, "y0res": 1023}
# ... and the cross-section molecules: JVAR_XS0 + x, x the 0-based position in the cross-section request
# (Profile.xs_names, the second axis of xamnt); "xs:<NAME>" in mols= of the MonoRTM Jacobian calls with ixsect = 1
JVAR_XS0 = 1101


def jac_codes(seq, xs_names=None) -> np.ndarray:
    """The `mols=` argument of the Jacobian calls as the int32 codes of the C ABI: ints (1-based molecules, or codes) pass through,
    names are looked up in JAC_VARS (case-insensitive); an unknown name raises ValueError.  "xs:<NAME>" is the cross-section
    molecule NAME of xs_names (the cross-section request, case-insensitive): JVAR_XS0 + its position."""
    out = []
    for v in ([seq] if isinstance(seq, (str, int, np.integer)) else seq):
        if isinstance(v, str) and v.lower().startswith("xs:"):
            names = [n.strip().upper() for n in (xs_names or [])]
            if v[3:].strip().upper() not in names:
                raise ValueError(f"unknown cross-section molecule {v!r}: the request holds {names}")
            v = JVAR_XS0 + names.index(v[3:].strip().upper())
        elif isinstance(v, str):
            if v.lower() not in JAC_VARS:
                raise ValueError(f"unknown Jacobian variable {v!r}: a 1-based molecule or one of {sorted(JAC_VARS)}")
            v = JAC_VARS[v.lower()]
        out.append(int(v))
    return np.ascontiguousarray(np.array(out, np.int32).reshape(-1))


# ---- the state map of the optimal-estimation step (monortm_hip_oe_step) -----------------------------------
# molecule names in the line file's numbering (1-based), for ("w", name, layers) of a state spec
MOLECULES = ("H2O", "CO2", "O3", "N2O", "CO", "CH4", "O2", "NO", "SO2", "NO2", "NH3", "HNO3", "OH", "HF", "HCL", "HBR", "HI", "CLO", "OCS", "H2CO",
             "HOCL", "N2", "HCN", "CH3CL", "H2O2", "C2H2", "C2H6", "PH3", "COF2", "SF6", "H2S", "HCOOH", "HO2", "O", "CLONO2", "NO+", "HOBR",
             "C2H4", "CH3OH")
OE_KINDS = {"t": 0, "tz": 1, "w": 2, "clw": 3, "tmpsfc": 4, "emiss": 4, "reflc": 4}   # state kind of the C ABI: K_T, K_TZ, K_W, K_CLW, K_SFC
OE_SFC_ROWS = {"tmpsfc": 0, "emiss": 1, "reflc": 2}
OE_MAX_MEAS, OE_MAX_STATE = 128, 2048


def oe_var_code(v) -> int:
    """The Jacobian variable a ("w", v, layers) item names: a molecule name of MOLECULES (case-insensitive) is its 1-based number,
    anything else goes through jac_codes (an int code, or a name of JAC_VARS)."""
    if isinstance(v, str) and v.upper() in MOLECULES:
        return MOLECULES.index(v.upper()) + 1
    return int(jac_codes([v])[0])


def _oe_items(spec, nlay_max: int):
    """A state spec as a flat list of (name, code or None, layer / level / None); ValueError on anything malformed."""
    if isinstance(spec, (str, bytes)) or not hasattr(spec, "__iter__"):
        raise ValueError("state spec: a list of tuples such as ('t', layers), ('w', 'H2O', layers), ('tmpsfc',)")
    out = []
    for item in spec:
        if not isinstance(item, (tuple, list)) or not item or not isinstance(item[0], str) or item[0].lower() not in OE_KINDS:
            raise ValueError(f"state spec item {item!r}: the first entry must be one of {sorted(OE_KINDS)}")
        name = item[0].lower()
        want = {"w": 3, "tmpsfc": 1, "emiss": 1, "reflc": 1}.get(name, 2)
        if len(item) != want:
            raise ValueError(f"state spec item {item!r}: {name!r} takes {want - 1} argument(s)")
        if want == 1:
            out.append((name, None, None))
            continue
        code = oe_var_code(item[1]) if name == "w" else None
        idx = item[-1]
        idx = list(idx) if hasattr(idx, "__iter__") and not isinstance(idx, str) else [idx]
        top = nlay_max + 1 if name == "tz" else nlay_max
        for k in idx:
            if not isinstance(k, (int, np.integer)) or not 0 <= int(k) < top:
                raise ValueError(f"state spec item {item!r}: index {k!r} outside 0..{top - 1}")
            out.append((name, code, int(k)))
    if not out:
        raise ValueError("state spec: no state element")
    return out


def oe_state_map(spec, nlay_max: int, vars=()):
    """(state_kind, state_row) of monortm_hip_oe_step, int32 [nstate], from a readable spec: a list of
      ("t", layers)  ("tz", levels)  ("w", "H2O" | code | JAC_VARS name, layers)  ("clw", layers)  ("tmpsfc",)  ("emiss",)  ("reflc",)
    in the order the state vector has them; layers / levels are 0-based ints or sequences of them, repeats are allowed.  ("w", v, ...) is
    resolved against `vars`, the codes in slot order that an obs_jacobian result carries under "vars": row = layer x len(vars) + slot."""
    vars = [int(v) for v in np.asarray(vars).reshape(-1)]
    kind, row = [], []
    for name, code, k in _oe_items(spec, nlay_max):
        kind.append(OE_KINDS[name])
        if name == "w":
            if code not in vars:
                raise ValueError(f"state spec: variable {code} is not among the Jacobian's vars {vars}")
            row.append(k * len(vars) + vars.index(code))
        else:
            row.append(OE_SFC_ROWS[name] if k is None else k)
    return np.ascontiguousarray(kind, np.int32), np.ascontiguousarray(row, np.int32)


OE_FULL_WANT = ("gain_t", "avk", "post_cov", "dofs")


def oe_se_kind(shape, nprof: int, nmeas: int, se_kind=None):
    """(se_kind, se_per_profile) of monortm_hip_oe_step_full for an Se of this shape: [nmeas] variances (0, 0), [nprof, nmeas] (0, 1),
    [nmeas, nmeas] a covariance matrix (1, 0), [nprof, nmeas, nmeas] (1, 1).  ValueError for any other shape, and for [nmeas, nmeas]
    when nprof = nmeas - both a matrix and per-profile variances - unless se_kind (0 or 1) says which; a se_kind that is given must fit."""
    shape, m = tuple(int(v) for v in shape), int(nmeas)
    if se_kind not in (None, 0, 1):
        raise ValueError(f"se_kind must be None, 0 (variances) or 1 (covariance matrix), got {se_kind!r}")
    fits = [k for k, s in (((0, 0), (m,)), ((0, 1), (nprof, m)), ((1, 0), (m, m)), ((1, 1), (nprof, m, m))) if s == shape and se_kind in (None, k[0])]
    if not fits:
        raise ValueError(f"Se must be [{m}] or [{nprof}, {m}] (se_kind 0), [{m}, {m}] or [{nprof}, {m}, {m}] (se_kind 1), got {list(shape)}"
                         + ("" if se_kind is None else f" with se_kind = {se_kind}"))
    if len(fits) > 1:
        raise ValueError(f"Se {list(shape)} is ambiguous with nprof = nmeas = {m}: per-profile variances or one covariance matrix; "
                         f"say se_kind = 0 or 1")
    return fits[0]


def _oe_want(want):
    """The requested diagnostics of oe_step_full in the order of OE_FULL_WANT; ValueError for an unknown name."""
    want = (want,) if isinstance(want, str) else tuple(want)
    bad = [w for w in want if w not in OE_FULL_WANT]
    if bad:
        raise ValueError(f"unknown diagnostics {bad}: choose from {list(OE_FULL_WANT)}")
    return tuple(w for w in OE_FULL_WANT if w in want)


def _oe_map_of(state, nlay_max: int, vars):
    """A (state_kind, state_row) pair as it is, a spec through oe_state_map."""
    if isinstance(state, tuple) and len(state) == 2 and all(isinstance(a, np.ndarray) for a in state):
        kind, row = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in state)
        if kind.shape != row.shape or not len(kind):
            raise ValueError("state map: state_kind and state_row must be two int arrays of one length >= 1")
        return kind, row
    return oe_state_map(state, nlay_max, vars)


def _lm_check(se, Se, x0, c0):
    """What retrieve_lm and lm_start refuse before they touch the batch."""
    if (se is None) == (Se is None):
        raise ValueError("retrieve_lm: give se (variances) or Se (any shape of oe_step_full), not both")
    if x0 is not None and c0 is None:
        raise ValueError("retrieve_lm: x0 needs c0, the caller's own Sa^-1 (x0 - xa) (the loop never forms Sa^-1)")
    if x0 is None and c0 is not None:
        raise ValueError("retrieve_lm: c0 without x0")


OE_WRITE_KINDS = {"t": 0, "tz": 1, "w": 2, "clw": 3, "tmpsfc": 4}
OE_DONE = {0: "running", 1: "converged", 2: "failed step", 3: "out of iterations", 4: "stalled at gamma_max"}


def oe_write_map(spec, nlay_max: int, nmol: int):
    """(map_kind, map_index, map_mol) of monortm_hip_oe_scatter_dev, int32 [nstate], from a state spec over ("t", layers), ("tz",
    levels), ("w", molecule, layers), ("clw", layers) and ("tmpsfc",).  A variable named twice is written from its last column: the
    earlier ones get kind -1 (checked against the box, not written) and an index under which `index < nlay` says whether they are
    live - the layer, level - 1, or -1 for TMPSFC.  ValueError for what has no resident input ("emiss", "reflc", a Jacobian variable
    that is no molecule of the batch)."""
    items = _oe_items(spec, nlay_max)
    kind, index, mol = (np.zeros(len(items), np.int32) for _ in range(3))
    last = {}
    for col, (name, code, k) in enumerate(items):
        if name not in OE_WRITE_KINDS:
            raise ValueError(f"a state element {name!r} has no resident scalar to write back (oe_step itself takes it)")
        if name == "w" and not 1 <= code <= nmol:
            raise ValueError(f"Jacobian variable {code} is not a molecule of the batch (oe_step itself takes it)")
        last[(name, code, k)] = col
    for col, (name, code, k) in enumerate(items):
        if last[(name, code, k)] == col:
            kind[col], index[col], mol[col] = OE_WRITE_KINDS[name], 0 if k is None else k, code - 1 if name == "w" else 0
        else:
            kind[col], index[col] = -1, -1 if k is None else k - 1 if name == "tz" else k
    return kind, index, mol


JAC_FIELDS = ("o", "rad", "tb", "k_t", "k_tz", "k_w", "k_clw", "k_o", "k_sfc")
SCAN_JAC_RTM_FIELDS = ("rad", "tb", "k_o", "k_path", "k_t", "k_tz", "k_sfc")                 # output order of monortm_hip_rtm_scan_jac
SCAN_JAC_FIELDS = ("o", "rad", "tb", "k_t", "k_tz", "k_w", "k_clw", "k_o", "k_path", "k_sfc")   # ... of monortm_hip_scan_jacobian
OBS_JAC_RTM_FIELDS = ("y", "k_t", "k_tz", "k_sfc")                                           # output order of monortm_hip_rtm_obs_jac
OBS_JAC_FIELDS = ("o", "y", "k_t", "k_tz", "k_w", "k_clw", "k_sfc")                           # ... of monortm_hip_obs_jacobian
OBS_RTM_FIELDS = ("y",)                                                                      # ... of monortm_hip_rtm_obs
OBS_FIELDS = ("o", "y")                                                                      # ... of monortm_hip_obs
OBS_MAX_PATHS, OBS_MAX_WN, OBS_MAX_VIEWS, OBS_MAX_CHAN = 16384, 80000, 65535, 65536           # the bounds of monortm_hip_obs_create


class ObsOperator:
    """A measurement operator (monortm_hip_obs_create): views = beams sampled by adjacent paths of a scan,
    channels = passbands sampled by wavenumbers,
        y[p, v, c] = sum_{j in view v} wpath[j] sum_{i: chan[i] = c} wchan[i] q[p, j, i].
    view_start [nview + 1] is CSR (view v holds the paths view_start[v] .. view_start[v + 1] - 1; starts at 0, never decreases, ends at
    npath; empty views are allowed), chan [nwn] maps every wavenumber to its channel or to -1 (unused), the weights are finite and of
    any sign; nchan defaults to max(chan) + 1.  The same checks as the C entry, raised as ValueError."""

    def __init__(self, view_start, wpath, chan, wchan, nchan=None):
        def arr(x, dt, name):
            a = np.asarray(x)
            if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) if dt == np.int32 else np.issubdtype(a.dtype, np.number)
                                   and not np.issubdtype(a.dtype, np.complexfloating)):
                raise ValueError(f"{name}: a 1-D array of {'integers' if dt == np.int32 else 'real numbers'}")
            if dt == np.int32 and a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError(f"{name}: out of range")
            return np.ascontiguousarray(a, dt)

        vs, wp = arr(view_start, np.int32, "view_start"), arr(wpath, np.float64, "wpath")
        ch, wc = arr(chan, np.int32, "chan"), arr(wchan, np.float64, "wchan")
        npath, nwn, nview = len(wp), len(ch), len(vs) - 1
        if not 1 <= npath <= OBS_MAX_PATHS:
            raise ValueError(f"npath = len(wpath) outside 1..{OBS_MAX_PATHS}")
        if not 1 <= nwn <= OBS_MAX_WN or len(wc) != nwn:
            raise ValueError(f"chan and wchan must have the same length nwn in 1..{OBS_MAX_WN}")
        if not 1 <= nview <= OBS_MAX_VIEWS:
            raise ValueError(f"view_start must have nview + 1 entries, nview in 1..{OBS_MAX_VIEWS}")
        if vs[0] != 0 or vs[-1] != npath or np.any(np.diff(vs) < 0):
            raise ValueError("view_start must start at 0, never decrease and end at npath")
        if nchan is None:
            nchan = int(ch.max()) + 1
        nchan = int(nchan)
        if not 1 <= nchan <= OBS_MAX_CHAN:
            raise ValueError(f"nchan outside 1..{OBS_MAX_CHAN}")
        if ch.min() < -1 or ch.max() >= nchan:
            raise ValueError("chan must lie in -1..nchan-1")
        if ((nwn + 63) // 64) * (nchan + 1) > 1 << 26:
            raise ValueError("nwn / 64 x nchan exceeds the membership table's bound (2^26 entries)")
        if not (np.all(np.isfinite(wp)) and np.all(np.isfinite(wc))):
            raise ValueError("the weights must be finite")
        self.view_start, self.wpath, self.chan, self.wchan = vs, wp, ch, wc
        self.npath, self.nwn, self.nview, self.nchan = npath, nwn, nview, nchan
        for a in (vs, wp, ch, wc):
            a.setflags(write=False)

    def dense(self) -> np.ndarray:
        """The [nview * nchan, npath * nwn] weight matrix W: y[p].ravel() = W @ q[p].ravel() for q [npath, nwn]."""
        vw = np.zeros((self.nview, self.npath))
        for v in range(self.nview):
            j = slice(self.view_start[v], self.view_start[v + 1])
            vw[v, j] = self.wpath[j]
        cw = np.zeros((self.nchan, self.nwn))
        used = self.chan >= 0
        cw[self.chan[used], np.nonzero(used)[0]] = self.wchan[used]
        return np.einsum("vj,ci->vcji", vw, cw).reshape(self.nview * self.nchan, self.npath * self.nwn)

    @classmethod
    def from_sets(cls, views, channels, npath=None, nwn=None):
        """Uniform normalised weights from index sets: views = [[paths of view 0], ...] (every path in at most one view), channels =
        [[wavenumbers of channel 0], ...] (every wavenumber in at most one channel).  Path j of a view of n paths gets 1 / n, sample i
        of a channel of m samples 1 / m.  The paths are reordered into CSR: returns (operator, perm) with perm[k] = the caller's index
        of the operator's path k - hand path[..., perm, :] (and emiss / reflc per path likewise) to the calls.  The operator holds the
        paths of the views only (its npath is len(perm)): a path in no view is not handed over at all, so whatever lies along it - a
        non-finite radiance included - cannot reach a measurement.  npath, where given, is the caller's number of paths (the bound
        of the indices)."""
        views = [[int(j) for j in v] for v in views]
        channels = [[int(i) for i in c] for c in channels]
        if not views or not channels:
            raise ValueError("at least one view and one channel")
        flat = [j for v in views for j in v]
        npath = (max(flat) + 1 if flat else 1) if npath is None else int(npath)
        fl = [i for c in channels for i in c]
        nwn = (max(fl) + 1 if fl else 1) if nwn is None else int(nwn)
        if len(set(flat)) != len(flat) or any(not 0 <= j < npath for j in flat):
            raise ValueError("views: every path index in 0..npath-1 and in at most one view")
        if len(set(fl)) != len(fl) or any(not 0 <= i < nwn for i in fl):
            raise ValueError("channels: every wavenumber index in 0..nwn-1 and in at most one channel")
        if not flat:
            raise ValueError("views: at least one view must hold a path")
        perm = np.array(flat, np.int64)
        vs = np.concatenate([[0], np.cumsum([len(v) for v in views])]).astype(np.int32)
        wp = np.concatenate([np.full(len(v), 1.0 / len(v)) for v in views if v])
        ch, wc = np.full(nwn, -1, np.int32), np.zeros(nwn)
        for c, members in enumerate(channels):
            ch[members] = c
            wc[members] = 1.0 / max(len(members), 1)
        return cls(vs, wp, ch, wc, nchan=len(channels)), perm


class _BadQuantity(KeyError, ValueError):
    """An unknown quantity name: the KeyError it has always been, and a ValueError for callers that catch bad arguments."""


def _quantity(q, band: bool = False) -> int:
    """'tb' -> 1, 'rad' -> 0 and, for the forward measurement operator only (band=True), 'band_tb' -> 2; an int is passed through
    unchanged (the C ABI checks it)."""
    if isinstance(q, str):
        names = {"tb": 1, "rad": 0, "band_tb": 2} if band else {"tb": 1, "rad": 0}
        if q.lower() not in names:
            raise _BadQuantity(q)
        return names[q.lower()]
    return int(q)


# the radiation constants as the kernels hold them (K_RADCN1, K_RADCN2 of device_common.hpp; src/PhysConstants.f90)
RADCN1 = 1.191042722E-12
RADCN2 = 1.4387752


def _band_args(vcen, rad):
    v, r = np.asarray(vcen, np.float64), np.asarray(rad, np.float64)
    if v.ndim != 1 or r.ndim < 1 or r.shape[-1] != len(v):
        raise ValueError(f"vcen must be [nchan] and rad [..., nchan], got {v.shape} and {r.shape}")
    if not np.all(np.isfinite(v) & (v > 0.)):
        raise ValueError("vcen: every value finite and > 0")
    return v, r


def band_tb(vcen, rad) -> np.ndarray:
    """The band brightness temperature of contracted radiances rad [..., nchan] at the channels' nominal wavenumbers vcen [nchan]
    (quantity "band_tb" of MonoRTM.obs / rtm_obs, evaluated on the host in float64):
        TB = RADCN2 vcen / log(RADCN1 vcen^3 / rad + 1).
    An element that is exactly 0 (no sample: an empty view or channel) stays 0; one that is negative or not finite is NaN."""
    v, r = _band_args(vcen, rad)
    ok = np.isfinite(r) & (r > 0.)
    out = np.where(r == 0., 0., np.nan)
    c3 = np.broadcast_to(RADCN1 * (v * v * v), r.shape)
    vv = np.broadcast_to(v, r.shape)
    out[ok] = RADCN2 * vv[ok] / np.log(c3[ok] / r[ok] + 1.)
    return out


def band_tb_slope(vcen, rad) -> np.ndarray:
    """dTB/dRAD of band_tb: RADCN2 v RADCN1 v^3 / (log(X)^2 X rad^2) with X = RADCN1 v^3 / rad + 1 (the factor of DESIGN.md section
    3.6).  Band-TB Jacobians from the radiance Jacobians of obs_jacobian(quantity="rad"):
        K_band = band_tb_slope(vcen, y_rad)[..., None, :] * K_rad.
    Elements without a temperature (rad <= 0 or not finite) are NaN, those without a sample (rad == 0) are 0."""
    v, r = _band_args(vcen, rad)
    ok = np.isfinite(r) & (r > 0.)
    out = np.where(r == 0., 0., np.nan)
    c3 = np.broadcast_to(RADCN1 * (v * v * v), r.shape)[ok]
    vv = np.broadcast_to(v, r.shape)[ok]
    x = c3 / r[ok] + 1.
    lx = np.log(x)
    out[ok] = (RADCN2 * vv) * ((c3 / r[ok]) / x) / ((lx * lx) * r[ok])   # rad enters once per factor: rad^2 underflows for a cold band
    return out


def _vcen(vcen, quantity: int, nchan: int):
    """The vcen argument of the forward entries: required, [nchan], finite and > 0 for quantity 2; ignored otherwise."""
    if quantity != 2:
        return None
    if vcen is None:
        raise ValueError("quantity 'band_tb' needs vcen [nchan], the channels' nominal wavenumbers")
    v = np.ascontiguousarray(vcen, np.float64)
    if v.shape != (nchan,):
        raise ValueError(f"vcen must be [{nchan}], got {v.shape}")
    if not np.all(np.isfinite(v) & (v > 0.)):
        raise ValueError("vcen: every value finite and > 0")
    return v


# selectors 2 .. 7 of MonoRTM.counter(): launches of the continuum / cloud / total kernel by variant
FINISH_VARIANTS = ("mw", "high", "par", "q4", "plain64", "plain256")
FINISH_COUNTER0 = 2
# selectors 16 .. 19: launches of far_kernel by waves per workgroup
FAR_WAVES = (1, 2, 4, 8)
FAR_COUNTER0 = 16

SCAN_FIELDS = ("rup", "rdn", "trtot", "rad", "tb", "tmr")   # output order of monortm_hip_rtm_scan


def plane_parallel_path(zenith_deg, nlay_max: int) -> np.ndarray:
    """Path factors of a plane-parallel atmosphere for rtm_scan / scan: [npath, nlay_max] of 1 / cos(zenith), the same in every
    layer.  Angles outside [0, 90) degrees (and NaN) are refused."""
    z = np.atleast_1d(np.asarray(zenith_deg, np.float64))
    if z.ndim != 1 or z.size < 1 or int(nlay_max) < 1:
        raise ValueError("zenith_deg: a scalar or a 1-D sequence of angles; nlay_max >= 1")
    if not np.all((z >= 0.) & (z < 90.)):
        raise ValueError("zenith angles must lie in [0, 90) degrees")
    return np.ascontiguousarray(np.repeat((1. / np.cos(np.deg2rad(z)))[:, None], int(nlay_max), axis=1))


class MonoRTMError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"monortm_hip error {code} ({ERRORS.get(code, '?')}): {msg}")
        self.code = code


def load_library(path: str | None = None):
    """dlopen the in-tree HIP library and bind every declared symbol (fails loudly if absent)."""
    global _LIB
    if _LIB is None or path:
        p = path or os.environ.get("MONORTM_HIP_LIB") or _build.LIB  # env override: A/B builds of the same ABI
        if not os.path.exists(p):
            raise MonoRTMError(7, f"{p} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        # torch ships its own HIP runtime (same SONAME as /opt/rocm's).  Whichever copy enters the process first serves
        # both torch and this library; if ours pulled in /opt/rocm's first, torch later reports "No HIP GPUs are
        # available".  So let torch load its runtime before we dlopen.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(p)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the ABI symbol is missing
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def _np(a, dt=np.float64):
    return np.ascontiguousarray(a, dt)


def _ptr(a):
    return a.ctypes.data_as(_vp) if a is not None else None


def pack_layers(profiles, lm: int, get, width=None, dtype=np.float64) -> np.ndarray:
    """get(p) [nlay] (or [nlay, width]) of every profile, zero-padded to lm layers: [nprof, lm] (or [nprof, lm, width])."""
    out = np.zeros((len(profiles), lm) if width is None else (len(profiles), lm, width), dtype)
    for i, p in enumerate(profiles):
        out[i, : p.nlay] = get(p)
    return out


def tape3_probe(path: str, v1: float, v2: float):
    """Host-only TAPE3 parse (no GPU): -> (n_physical[40], n_entries[40], n_coupled[40]) numpy int64 arrays."""
    lib = load_library()
    a, b, c = (np.zeros(40, np.int64) for _ in range(3))
    ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_longlong))  # noqa: E731
    rc = lib.monortm_hip_tape3_probe(path.encode(), float(v1), float(v2), ptr(a), ptr(b), ptr(c))
    if rc:
        raise MonoRTMError(rc, lib.monortm_hip_last_error(None).decode())
    return a, b, c


class MonoRTM:
    """One GPU context = one loaded TAPE3 (the reference loads it once per process, with the first
    call's v1,v2: src/modm.f90:187-190).  real_kind 8 = the reference's "dbl" build, 4 = its "sgl" build
    (REAL arrays are float32; wavenumbers stay float64)."""

    def __init__(self, tape3: str, v1: float, v2: float, device: int = -1, icp: int = 1, real_kind: int = 8, ngpu: int | None = None):
        """ngpu = None: one context on `device`; ngpu = N (0 = all visible): a multi-device context whose host-buffer calls
        shard the batch over N devices (monortm_hip_init_multi)."""
        self.lib = load_library()
        self.ctx = _vp()
        self.real_kind = real_kind
        self.dtype = np.float32 if real_kind == 4 else np.float64
        if ngpu is None:
            rc = self.lib.monortm_hip_init(tape3.encode(), float(v1), float(v2), icp, real_kind, device, C.byref(self.ctx))
        else:
            rc = self.lib.monortm_hip_init_multi(tape3.encode(), float(v1), float(v2), icp, real_kind, ngpu, C.byref(self.ctx))
        if rc:
            raise MonoRTMError(rc, self.lib.monortm_hip_last_error(None).decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.monortm_hip_finalize(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise MonoRTMError(rc, self.lib.monortm_hip_last_error(self.ctx).decode())

    def line_count(self, mol: int = 0) -> int:
        return int(self.lib.monortm_hip_line_count(self.ctx, mol))

    # ---- host-buffer calls (mirror MODM / CALCTMR+RTM of the Fortran boundary) -------------------
    def set_xsec(self, tabs) -> None:
        """Hand the parsed cross-section tables (monortm_amd.xsec.XsTables) to the context (monortm_hip_xsec_tables)."""
        reg, temps, pres, offs, pool = tabs.flatten()
        nreg = len(reg)
        pad = lambda a, dt: np.ascontiguousarray(a if nreg else np.zeros((1, 6)), dt)  # noqa: E731
        reg, temps, pres, offs = pad(reg, np.float64), pad(temps, np.float64), pad(pres, np.float64), pad(offs, np.int64)
        pool = _np(pool if len(pool) else np.zeros(1))
        self._chk(self.lib.monortm_hip_xsec_tables(self.ctx, len(tabs.names), nreg, _ptr(reg), _ptr(temps), _ptr(pres), _ptr(offs),
                                                   _ptr(pool), len(pool) if nreg else 0))
        self._xs_key = (tuple(tabs.names), nreg)

    def modm(self, profiles: list[Profile], ixsect: int | None = None):
        """Batched MODM over profiles sharing wn/nmol and the scalar options of profiles[0].  With cross-section molecules
        (profiles[0].xs_names, IXSECT = 1) the tables are parsed from profiles[0].xs_dir for the call's wavenumber range - the
        reference's XSREAD does that per run with min / max of the wavenumbers, src/monortm.f90:494-497 - and a fifth array,
        ODXSEC, is returned."""
        p0 = profiles[0]
        if ixsect is None:
            ixsect = p0.ixsect
        if ixsect == 1 and p0.xs_names and p0.xs_dir:
            from . import xsec

            self.set_xsec(xsec.load_tables(p0.xs_dir, p0.xs_names, float(p0.wn.min()), float(p0.wn.max())))
        nprof, nwn = len(profiles), p0.nwn
        nlay = np.array([p.nlay for p in profiles], np.int32)
        lm = int(nlay.max())
        nmol, P, T, CLW, WKL, WB, fac = self._pack_atm(profiles, lm)
        O = np.empty((nprof, lm, nwn), self.dtype)
        OBM = np.empty((nprof, lm, nmol, nwn), self.dtype)
        OC = np.empty((nprof, lm, NCONT, nwn), self.dtype)
        OCLW = np.empty((nprof, lm, nwn), self.dtype)
        lead = (self.ctx, nprof, nwn, _ptr(_np(p0.wn)), p0.dvset, _ptr(nlay), lm, nmol, _ptr(P), _ptr(T), _ptr(CLW), _ptr(WKL), _ptr(WB), _ptr(fac),
                p0.sclcpl, p0.sclhw, p0.y0res, p0.ibrd)
        if ixsect == 1 and p0.xs_names:
            XA = pack_layers(profiles, lm, lambda p: p.xamnt, len(p0.xs_names), self.dtype)
            ODX = np.empty((nprof, lm, nwn), self.dtype)
            self._chk(self.lib.monortm_hip_modm_xs(*lead, 1, _ptr(XA), _ptr(ODX), _ptr(O), _ptr(OBM), _ptr(OC), _ptr(OCLW)))
            return O, OBM, OC, OCLW, ODX
        self._chk(self.lib.monortm_hip_modm(*lead, ixsect, _ptr(O), _ptr(OBM), _ptr(OC), _ptr(OCLW)))
        return O, OBM, OC, OCLW

    def rtm(self, profiles: list[Profile], O: np.ndarray):
        p0 = profiles[0]
        nprof, nwn = len(profiles), p0.nwn
        nlay = np.array([p.nlay for p in profiles], np.int32)
        lm = int(nlay.max())
        irt = np.array([p.irt for p in profiles], np.int32)
        dt = self.dtype
        T = np.zeros((nprof, lm), dt)
        TZ = np.zeros((nprof, lm + 1), dt)
        for i, p in enumerate(profiles):
            T[i, : p.nlay] = p.t
            TZ[i, : p.nlay + 1] = p.tz
        ts = np.array([p.tmpsfc for p in profiles], dt)
        em = _np(np.stack([p.emiss for p in profiles]), dt)
        rf = _np(np.stack([p.reflc for p in profiles]), dt)
        outs = [np.zeros((nprof, nwn), dt) for _ in range(6)]
        wn = _np(p0.wn)
        O = _np(O, dt)
        self._chk(self.lib.monortm_hip_rtm(self.ctx, nprof, nwn, _ptr(wn), _ptr(nlay), lm, _ptr(irt), p0.iout, _ptr(T), _ptr(TZ),
                                           _ptr(O), _ptr(ts), _ptr(em), _ptr(rf), *[_ptr(o) for o in outs]))
        return (*outs, ts)

    # ---- path scans (monortm_hip_rtm_scan) ------------------------------------------------------------
    def _path(self, path, nprof: int, lm: int) -> np.ndarray:
        """[npath, nlay_max] (the same paths for every profile) or [nprof, npath, nlay_max] -> the latter, contiguous."""
        f = np.asarray(path, self.dtype)
        if f.ndim == 2:
            f = np.broadcast_to(f[None], (nprof,) + f.shape)
        if f.ndim != 3 or f.shape[0] != nprof or f.shape[1] < 1 or f.shape[2] != lm:
            raise ValueError(f"path must be [npath, {lm}] or [{nprof}, npath, {lm}], got {f.shape}")
        return np.ascontiguousarray(f)

    def rtm_scan(self, profiles: list[Profile], O: np.ndarray, path, emiss=None, reflc=None) -> dict:
        """CALCTMR + RTM along npath paths per profile from one O [nprof, nlay_max, nwn]: path [npath, nlay_max] or
        [nprof, npath, nlay_max] holds the factor of every layer's amounts along the path (plane_parallel_path for secants).
        emiss / reflc default to the profiles' own; given as [nprof, npath, nwn] they differ per path (sfc_per_path = 1).
        Returns a dict of rup, rdn, trtot, rad, tb, tmr [nprof, npath, nwn] and tmpsfc [nprof]."""
        nprof, nwn, nlay, lm, irt, T, TZ, ts, em, rf = self._pack_rtm(profiles)
        dt = self.dtype
        f = self._path(path, nprof, lm)
        npath = f.shape[1]
        em = em if emiss is None else _np(emiss, dt)
        rf = rf if reflc is None else _np(reflc, dt)
        if em.shape != rf.shape or em.shape not in ((nprof, nwn), (nprof, npath, nwn)):
            raise ValueError(f"emiss / reflc must both be [{nprof}, {nwn}] or [{nprof}, {npath}, {nwn}]")
        O = _np(O, dt)
        if O.shape != (nprof, lm, nwn):
            raise ValueError(f"O must be [{nprof}, {lm}, {nwn}], got {O.shape}")
        out = {k: np.zeros((nprof, npath, nwn), dt) for k in SCAN_FIELDS}
        wn = _np(profiles[0].wn)
        self._chk(self.lib.monortm_hip_rtm_scan(self.ctx, nprof, npath, nwn, _ptr(wn), _ptr(nlay), lm, _ptr(irt), profiles[0].iout,
                                                _ptr(T), _ptr(TZ), _ptr(O), _ptr(f), _ptr(ts), int(em.ndim == 3), _ptr(em), _ptr(rf),
                                                *[_ptr(out[k]) for k in SCAN_FIELDS]))
        out["tmpsfc"] = ts
        return out

    def scan(self, profiles: list[Profile], path, emiss=None, reflc=None) -> dict:
        """MODM once, then the radiances along every path (rtm_scan)."""
        return self.rtm_scan(profiles, self.modm(profiles)[0], path, emiss, reflc)

    def counter(self, which: int = 0) -> int:
        """monortm_hip_counter: 0 = rtm calls, 1 = rtm_scan calls that found O resident on the device; 2 .. 7 = launches of the
        continuum / cloud / total kernel by variant (FINISH_VARIANTS: finish_mw_kernel, finish_kernel<HIGH>, <PAR>, <Q4>, plain with
        64 threads, plain with 256), one per MODM evaluation; 9 = those of variant 0 that took the column layout
        (finish_mw_kernel_col); 16 .. 19 = launches of far_kernel with 1, 2, 4, 8 waves per workgroup
        (FAR_WAVES), one per level of intervals and MODM evaluation."""
        return int(self.lib.monortm_hip_counter(self.ctx, which))

    def run(self, profiles: list[Profile]) -> list[Dump]:
        """MODM + CALCTMR + RTM for a batch, as PROGRAM MONORTM chains them (src/monortm.f90:557-574)."""
        res = self.modm(profiles)
        O, OBM, OC, OCLW = res[:4]
        ODX = res[4] if len(res) > 4 else None
        rup, rdn, trtot, rad, tb, tmr, ts = self.rtm(profiles, O)
        out = []
        for i, p in enumerate(profiles):
            n = p.nlay
            out.append(Dump(O[i, :n], OBM[i, :n], OC[i, :n], OCLW[i, :n], rup[i], rdn[i], trtot[i], rad[i], tb[i], tmr[i],
                            float(ts[i]), None if ODX is None else ODX[i, :n]))
        return out

    # ---- Jacobians (monortm_hip_rtm_jac / monortm_hip_jacobian) --------------------------------------
    def _pack_rtm(self, profiles: list[Profile]):
        nprof, nwn = len(profiles), profiles[0].nwn
        nlay = np.array([p.nlay for p in profiles], np.int32)
        lm = int(nlay.max())
        dt = self.dtype
        T = np.zeros((nprof, lm), dt)
        TZ = np.zeros((nprof, lm + 1), dt)
        for i, p in enumerate(profiles):
            T[i, : p.nlay] = p.t
            TZ[i, : p.nlay + 1] = p.tz
        irt = np.array([p.irt for p in profiles], np.int32)
        ts = np.array([p.tmpsfc for p in profiles], dt)
        em = _np(np.stack([p.emiss for p in profiles]), dt)
        rf = _np(np.stack([p.reflc for p in profiles]), dt)
        return nprof, nwn, nlay, lm, irt, T, TZ, ts, em, rf

    def _pack_atm(self, profiles: list[Profile], lm: int):
        """The MODM inputs of a batch, zero-padded to lm layers, and the continuum factors of profiles[0]: nmol, P, T, CLW, WKL, WB, fac."""
        nmol = profiles[0].nmol
        P, T, CLW, WB = (pack_layers(profiles, lm, g, None, self.dtype) for g in (lambda p: p.p, lambda p: p.t, lambda p: p.clw, lambda p: p.wbrodl))
        return nmol, P, T, CLW, pack_layers(profiles, lm, lambda p: p.wkl, nmol, self.dtype), WB, _np(profiles[0].cntnm)

    def _full_args(self, profiles: list[Profile], rtm, atm, em, rf, xargs=()):
        """The leading arguments of the entries that run MODM and RTM in one call (monortm_hip_jacobian*, _scan_jacobian*, _obs_jacobian*,
        _obs): ctx, nprof ... ibrd, xargs (what ixsect adds), irt, TZ, tmpsfc, emiss, reflc - from _pack_rtm, _pack_atm and the call's
        emissivities.  The pointers keep their arrays alive."""
        nprof, nwn, nlay, lm, irt, _, TZ, ts, _, _ = rtm
        nmol, P, T, CLW, WKL, WB, fac = atm
        p0 = profiles[0]
        return (self.ctx, nprof, nwn, _ptr(_np(p0.wn)), p0.dvset, _ptr(nlay), lm, nmol, _ptr(P), _ptr(T), _ptr(CLW), _ptr(WKL), _ptr(WB), _ptr(fac),
                p0.sclcpl, p0.sclhw, p0.y0res, p0.ibrd, *xargs, _ptr(irt), _ptr(TZ), _ptr(ts), _ptr(em), _ptr(rf))

    def rtm_jacobian(self, profiles: list[Profile], O: np.ndarray, quantity="tb") -> dict:
        """The adjoint of RTM alone, given the optical depths O [nprof, nlay_max, nwn]: dict of rad, tb [nprof, nwn], k_o, k_t (Planck
        term only) [nprof, nlay_max, nwn], k_tz [nprof, nlay_max + 1, nwn], k_sfc [nprof, 3, nwn] (d/dTMPSFC, d/dEMISS, d/dREFLC).
        quantity: "tb" or "rad" (what q is)."""
        nprof, nwn, nlay, lm, irt, T, TZ, ts, em, rf = self._pack_rtm(profiles)
        dt = self.dtype
        O = _np(O, dt)
        out = dict(rad=np.zeros((nprof, nwn), dt), tb=np.zeros((nprof, nwn), dt), k_o=np.zeros((nprof, lm, nwn), dt),
                   k_t=np.zeros((nprof, lm, nwn), dt), k_tz=np.zeros((nprof, lm + 1, nwn), dt), k_sfc=np.zeros((nprof, 3, nwn), dt))
        wn = _np(profiles[0].wn)
        self._chk(self.lib.monortm_hip_rtm_jac(self.ctx, nprof, nwn, _ptr(wn), _ptr(nlay), lm, _ptr(irt), _quantity(quantity), _ptr(T),
                                               _ptr(TZ), _ptr(O), _ptr(ts), _ptr(em), _ptr(rf), *[_ptr(out[k]) for k in
                                                                                                  ("rad", "tb", "k_o", "k_t", "k_tz", "k_sfc")]))
        return out

    def _jac_xs(self, profiles: list[Profile], ixsect: int, xs_entry: bool, lm: int):
        """What ixsect adds to a full Jacobian call: (suffix of the entry's name, the arguments behind ibrd, the packed xamnt).
        ixsect = 1 packs xamnt as modm() does and takes the *_xs entry; ixsect = 0 takes the entry without cross sections, or -
        xs_entry - the *_xs entry with ixsect = 0, which is the same computation."""
        if ixsect not in (0, 1):
            raise ValueError("ixsect must be 0 or 1")
        if ixsect == 0:
            return ("_xs", (0, None), None) if xs_entry else ("", (), None)
        p0 = profiles[0]
        if p0.xs_names and p0.xs_dir:   # (as modm(): the tables of the call's wavenumber range)
            from . import xsec

            self.set_xsec(xsec.load_tables(p0.xs_dir, p0.xs_names, float(p0.wn.min()), float(p0.wn.max())))
        XA = pack_layers(profiles, lm, lambda p: p.xamnt, len(p0.xs_names or []), self.dtype)
        return "_xs", (1, _ptr(XA)), XA

    def jacobian(self, profiles: list[Profile], mols=(1,), quantity="tb", ixsect: int = 0, xs_entry: bool = False) -> dict:
        """MODM + RTM with Jacobians for a batch (real_kind 8): dict of o [nprof, nlay_max, nwn], rad, tb [nprof, nwn], k_t, k_clw, k_o
        [nprof, nlay_max, nwn], k_tz [nprof, nlay_max + 1, nwn], k_w [nprof, nlay_max, len(mols), nwn] (d/d ln WKL of mols, 1-based)
        and k_sfc [nprof, 3, nwn].  Partial derivatives with respect to the MODM / RTM inputs (see include/monortm_hip.h).
        mols may mix molecules with the names (or codes) of JAC_VARS: "p", "wbrod" (d/d ln P_k, d/d ln WBRODL_k) and the scalars
        "xself" .. "xrayl", "sclcpl", "sclhw", "y0res", whose k_w slot summed over the layers is dq/dtheta;
        vars holds the codes in slot order.  The same holds for scan_jacobian, obs_jacobian and the DeviceBatch calls.
        ixsect = 1 (the tables are those of set_xsec): o, k_o and every slot include the cross-section
        molecules, k_t and the "p" slot their own T and P dependence, and mols accepts "xs:<NAME>" (a name of profiles[0].xs_names)
        or JVAR_XS0 + x: d/d ln XAMNT of that molecule.  Likewise for scan_jacobian and obs_jacobian; not for DeviceBatch."""
        rtm = self._pack_rtm(profiles)
        nprof, nwn, _, lm, _, _, _, _, em, rf = rtm
        dt = self.dtype
        jm = jac_codes(mols, profiles[0].xs_names)
        sfx, xargs, _xa = self._jac_xs(profiles, ixsect, xs_entry, lm)   # (_xa: xamnt, alive during the call)
        nj = len(jm)
        out = dict(o=np.zeros((nprof, lm, nwn), dt), rad=np.zeros((nprof, nwn), dt), tb=np.zeros((nprof, nwn), dt),
                   k_t=np.zeros((nprof, lm, nwn), dt), k_tz=np.zeros((nprof, lm + 1, nwn), dt), k_w=np.zeros((nprof, lm, nj, nwn), dt),
                   k_clw=np.zeros((nprof, lm, nwn), dt), k_o=np.zeros((nprof, lm, nwn), dt), k_sfc=np.zeros((nprof, 3, nwn), dt))
        self._chk(getattr(self.lib, "monortm_hip_jacobian" + sfx)(*self._full_args(profiles, rtm, self._pack_atm(profiles, lm), em, rf, xargs),
                                                                  _quantity(quantity), nj, _ptr(jm) if nj else None,
                                                                  *[_ptr(out[k]) if (k != "k_w" or nj) else None for k in JAC_FIELDS]))
        out["vars"] = jm
        return out

    # ---- Jacobians of path scans (monortm_hip_rtm_scan_jac / monortm_hip_scan_jacobian) ----------------------
    def _scan_sfc(self, em, rf, emiss, reflc, nprof, npath, nwn):
        em = em if emiss is None else _np(emiss, self.dtype)
        rf = rf if reflc is None else _np(reflc, self.dtype)
        if em.shape != rf.shape or em.shape not in ((nprof, nwn), (nprof, npath, nwn)):
            raise ValueError(f"emiss / reflc must both be [{nprof}, {nwn}] or [{nprof}, {npath}, {nwn}]")
        return em, rf

    def rtm_scan_jacobian(self, profiles: list[Profile], O: np.ndarray, path, quantity="tb", emiss=None, reflc=None) -> dict:
        """The adjoint of RTM along npath paths per profile from one O [nprof, nlay_max, nwn]; path, emiss, reflc as rtm_scan,
        quantity as rtm_jacobian.  Dict of rad, tb [nprof, npath, nwn], k_o (= factor x dq/dtau: with respect to the vertical O),
        k_path (= O x dq/dtau: with respect to the factor), k_t (Planck term only) [nprof, npath, nlay_max, nwn],
        k_tz [nprof, npath, nlay_max + 1, nwn], k_sfc [nprof, npath, 3, nwn]."""
        nprof, nwn, nlay, lm, irt, T, TZ, ts, em, rf = self._pack_rtm(profiles)
        dt = self.dtype
        f = self._path(path, nprof, lm)
        npath = f.shape[1]
        em, rf = self._scan_sfc(em, rf, emiss, reflc, nprof, npath, nwn)
        O = _np(O, dt)
        if O.shape != (nprof, lm, nwn):
            raise ValueError(f"O must be [{nprof}, {lm}, {nwn}], got {O.shape}")
        z = lambda *s: np.zeros((nprof, npath) + s, dt)  # noqa: E731
        out = dict(rad=z(nwn), tb=z(nwn), k_o=z(lm, nwn), k_path=z(lm, nwn), k_t=z(lm, nwn), k_tz=z(lm + 1, nwn), k_sfc=z(3, nwn))
        wn = _np(profiles[0].wn)
        self._chk(self.lib.monortm_hip_rtm_scan_jac(self.ctx, nprof, npath, nwn, _ptr(wn), _ptr(nlay), lm, _ptr(irt), _quantity(quantity),
                                                    _ptr(T), _ptr(TZ), _ptr(O), _ptr(f), _ptr(ts), int(em.ndim == 3), _ptr(em), _ptr(rf),
                                                    *[_ptr(out[k]) for k in SCAN_JAC_RTM_FIELDS]))
        return out

    def scan_jacobian(self, profiles: list[Profile], path, mols=(1,), quantity="tb", emiss=None, reflc=None, ixsect: int = 0,
                      xs_entry: bool = False) -> dict:
        """MODM (the base and the perturbed states of jacobian(), ONCE) + RTM with Jacobians along npath paths per profile (real_kind
        8): the fields of rtm_scan_jacobian with the optical-depth term in k_t, plus o [nprof, nlay_max, nwn] (the vertical optical
        depths), k_w [nprof, npath, nlay_max, len(mols), nwn] and k_clw [nprof, npath, nlay_max, nwn] - derivatives with respect to
        the batch's own (vertical) ln WKL and CLW."""
        rtm = self._pack_rtm(profiles)
        nprof, nwn, _, lm, _, _, _, _, em, rf = rtm
        dt = self.dtype
        f = self._path(path, nprof, lm)
        npath = f.shape[1]
        em, rf = self._scan_sfc(em, rf, emiss, reflc, nprof, npath, nwn)
        jm = jac_codes(mols, profiles[0].xs_names)
        sfx, xargs, _xa = self._jac_xs(profiles, ixsect, xs_entry, lm)   # (_xa: xamnt, alive during the call)
        nj = len(jm)
        z = lambda *s: np.zeros((nprof, npath) + s, dt)  # noqa: E731
        out = dict(o=np.zeros((nprof, lm, nwn), dt), rad=z(nwn), tb=z(nwn), k_t=z(lm, nwn), k_tz=z(lm + 1, nwn), k_w=z(lm, nj, nwn),
                   k_clw=z(lm, nwn), k_o=z(lm, nwn), k_path=z(lm, nwn), k_sfc=z(3, nwn))
        self._chk(getattr(self.lib, "monortm_hip_scan_jacobian" + sfx)(*self._full_args(profiles, rtm, self._pack_atm(profiles, lm), em, rf, xargs),
                                                                       _quantity(quantity), nj, _ptr(jm) if nj else None, npath, _ptr(f),
                                                                       int(em.ndim == 3),
                                                                       *[_ptr(out[k]) if (k != "k_w" or nj) else None for k in SCAN_JAC_FIELDS]))
        out["vars"] = jm
        return out

    # ---- channel- and beam-averaged Jacobians (monortm_hip_obs_create / _rtm_obs_jac / _obs_jacobian) ------------
    def obs_create(self, op: ObsOperator) -> int:
        """The operator's tables go to the device(s) once; returns the handle the calls below take (up to 16 per context)."""
        h = C.c_int(0)
        self._chk(self.lib.monortm_hip_obs_create(self.ctx, op.npath, op.nwn, op.nview, op.nchan, _ptr(op.view_start), _ptr(op.wpath),
                                                  _ptr(op.chan), _ptr(op.wchan), C.byref(h)))
        self.__dict__.setdefault("_obs", {})[h.value] = op
        return h.value

    def obs_destroy(self, handle: int) -> None:
        self._chk(self.lib.monortm_hip_obs_destroy(self.ctx, int(handle)))
        self.__dict__.get("_obs", {}).pop(int(handle), None)

    def _obs_shape(self, handle: int):
        op = self.__dict__.get("_obs", {}).get(int(handle))
        if op is None:
            raise MonoRTMError(6, "obs: not a handle of this context (never created here, or destroyed)")
        return op.nview, op.nchan

    def rtm_obs_jacobian(self, profiles: list[Profile], O: np.ndarray, path, obs: int, quantity="tb", emiss=None, reflc=None) -> dict:
        """The adjoint of RTM per measurement from one O [nprof, nlay_max, nwn]: the terms of rtm_scan_jacobian contracted with the
        operator `obs` (a handle of obs_create) inside the kernel.  Dict of y [nprof, nview, nchan], k_t (Planck term only)
        [nprof, nview, nlay_max, nchan], k_tz [nprof, nview, nlay_max + 1, nchan], k_sfc [nprof, nview, 3, nchan] (the emissivity and
        reflectivity rows: with respect to a common shift of all samples of the measurement)."""
        nprof, nwn, nlay, lm, irt, T, TZ, ts, em, rf = self._pack_rtm(profiles)
        dt = self.dtype
        f = self._path(path, nprof, lm)
        npath = f.shape[1]
        em, rf = self._scan_sfc(em, rf, emiss, reflc, nprof, npath, nwn)
        O = _np(O, dt)
        if O.shape != (nprof, lm, nwn):
            raise ValueError(f"O must be [{nprof}, {lm}, {nwn}], got {O.shape}")
        nv, nc = self._obs_shape(obs)
        z = lambda *s: np.zeros((nprof, nv) + s + (nc,), dt)  # noqa: E731
        out = dict(y=z(), k_t=z(lm), k_tz=z(lm + 1), k_sfc=z(3))
        wn = _np(profiles[0].wn)
        self._chk(self.lib.monortm_hip_rtm_obs_jac(self.ctx, nprof, npath, nwn, _ptr(wn), _ptr(nlay), lm, _ptr(irt), _quantity(quantity),
                                                   _ptr(T), _ptr(TZ), _ptr(O), _ptr(f), _ptr(ts), int(em.ndim == 3), _ptr(em), _ptr(rf),
                                                   int(obs), *[_ptr(out[k]) for k in OBS_JAC_RTM_FIELDS]))
        return out

    def obs_jacobian(self, profiles: list[Profile], path, obs: int, mols=(1,), quantity="tb", emiss=None, reflc=None, ixsect: int = 0,
                     xs_entry: bool = False) -> dict:
        """MODM (the base and the perturbed states of jacobian(), ONCE) + RTM with Jacobians per measurement (real_kind 8): the fields
        of rtm_obs_jacobian with the optical-depth term in k_t, plus o [nprof, nlay_max, nwn] (the vertical optical depths, as
        scan_jacobian returns them), k_w [nprof, nview, nlay_max, len(mols), nchan] and k_clw [nprof, nview, nlay_max, nchan]."""
        rtm = self._pack_rtm(profiles)
        nprof, nwn, _, lm, _, _, _, _, em, rf = rtm
        dt = self.dtype
        f = self._path(path, nprof, lm)
        npath = f.shape[1]
        em, rf = self._scan_sfc(em, rf, emiss, reflc, nprof, npath, nwn)
        jm = jac_codes(mols, profiles[0].xs_names)
        sfx, xargs, _xa = self._jac_xs(profiles, ixsect, xs_entry, lm)   # (_xa: xamnt, alive during the call)
        nj = len(jm)
        nv, nc = self._obs_shape(obs)
        z = lambda *s: np.zeros((nprof, nv) + s + (nc,), dt)  # noqa: E731
        out = dict(o=np.zeros((nprof, lm, nwn), dt), y=z(), k_t=z(lm), k_tz=z(lm + 1), k_w=z(lm, nj), k_clw=z(lm), k_sfc=z(3))
        self._chk(getattr(self.lib, "monortm_hip_obs_jacobian" + sfx)(*self._full_args(profiles, rtm, self._pack_atm(profiles, lm), em, rf, xargs),
                                                                      _quantity(quantity), nj, _ptr(jm) if nj else None, npath, _ptr(f),
                                                                      int(em.ndim == 3), int(obs),
                                                                      *[_ptr(out[k]) if (k != "k_w" or nj) else None for k in OBS_JAC_FIELDS]))
        out["vars"] = jm
        return out

    # ---- the optimal-estimation step (monortm_hip_oe_step) --------------------------------------------------------
    def oe_step(self, jac: dict, state, y_obs, x, xa, Sa, se, gamma=None) -> dict:
        """One Gauss-Newton / Levenberg-Marquardt update from the dict obs_jacobian (or rtm_obs_jacobian) returned: K is read in place
        through `state`, a spec of oe_state_map or the (state_kind, state_row) pair it makes.  y_obs [nprof, nview, nchan]; x, xa
        [nprof, nstate]; Sa [nstate, nstate] or [nprof, nstate, nstate] (lower triangle read); se [nmeas] or [nprof, nmeas]; gamma
        None (0) or [nprof].  Dict of x_new, post_var, avk_diag [nprof, nstate], dfs (the sum of avk_diag), chi2 [nprof] and status
        (int32 [nprof]; 1: the profile's step failed and x_new = x)."""
        kt = jac["k_t"]
        nprof, nv, lm, nc = kt.shape
        kw = jac.get("k_w")
        nj = 0 if kw is None else kw.shape[3]
        kind, row = _oe_map_of(state, lm, jac.get("vars", ()))
        n, m = len(kind), nv * nc
        f = lambda a: None if a is None else _np(a)  # noqa: E731
        K = [f(jac.get(k)) for k in ("k_t", "k_tz", "k_w", "k_clw", "k_sfc")]
        if nj == 0:
            K[2] = None
        Y, yo, x, xa, Sa, se, gamma = (f(a) for a in (jac["y"], y_obs, x, xa, Sa, se, gamma))
        for name, a, shapes in (("y_obs", yo, [(nprof, nv, nc)]), ("x", x, [(nprof, n)]), ("xa", xa, [(nprof, n)]), ("Sa", Sa, [(n, n), (nprof, n, n)]),
                                ("se", se, [(m,), (nprof, m)]), ("gamma", gamma, [(nprof,)])):
            if a is not None and a.shape not in shapes:
                raise ValueError(f"{name} must be {' or '.join(str(list(s)) for s in shapes)}, got {list(a.shape)}")
        out = dict(x_new=np.zeros((nprof, n)), post_var=np.zeros((nprof, n)), avk_diag=np.zeros((nprof, n)), chi2=np.zeros(nprof),
                   status=np.zeros(nprof, np.int32))
        self._chk(self.lib.monortm_hip_oe_step(self.ctx, nprof, nv, nc, lm, nj, n, _ptr(kind), _ptr(row), *[_ptr(k) for k in K], _ptr(Y), _ptr(yo),
                                               _ptr(x), _ptr(xa), _ptr(Sa), int(Sa.ndim == 3), _ptr(se), int(se.ndim == 2), _ptr(gamma),
                                               *[_ptr(out[k]) for k in ("x_new", "post_var", "avk_diag", "chi2", "status")]))
        out["dfs"] = out["avk_diag"].sum(axis=1)
        return out

    # ---- the step with a full Se and the full diagnostics (monortm_hip_oe_step_full) ---------------------------------
    def oe_step_full(self, jac: dict, state, y_obs, x, xa, Sa, Se, gamma=None, want=("avk", "post_cov", "dofs"), se_kind=None) -> dict:
        """oe_step with Se [nmeas] / [nprof, nmeas] (variances) or [nmeas, nmeas] / [nprof, nmeas, nmeas] (a covariance matrix, lower
        triangle read; oe_se_kind decides, se_kind settles nprof = nmeas), and the diagnostics named in `want`: "gain_t" [nprof, nmeas, nstate] (G^T), "avk" and "post_cov"
        [nprof, nstate, nstate], "dofs" [nprof] (tr A).  Dict of x_new, post_var, avk_diag, chi2, status and what was wanted; a failed
        profile (status 1) has x_new = x and zeros everywhere else."""
        want = _oe_want(want)
        kt = jac["k_t"]
        nprof, nv, lm, nc = kt.shape
        kw = jac.get("k_w")
        nj = 0 if kw is None else kw.shape[3]
        kind, row = _oe_map_of(state, lm, jac.get("vars", ()))
        n, m = len(kind), nv * nc
        f = lambda a: None if a is None else _np(a)  # noqa: E731
        K = [f(jac.get(k)) for k in ("k_t", "k_tz", "k_w", "k_clw", "k_sfc")]
        if nj == 0:
            K[2] = None
        Y, yo, x, xa, Sa, Se, gamma = (f(a) for a in (jac["y"], y_obs, x, xa, Sa, Se, gamma))
        se_kind, se_pp = oe_se_kind(Se.shape, nprof, m, se_kind)
        for name, a, shapes in (("y_obs", yo, [(nprof, nv, nc)]), ("x", x, [(nprof, n)]), ("xa", xa, [(nprof, n)]), ("Sa", Sa, [(n, n), (nprof, n, n)]),
                                ("gamma", gamma, [(nprof,)])):
            if a is not None and a.shape not in shapes:
                raise ValueError(f"{name} must be {' or '.join(str(list(s)) for s in shapes)}, got {list(a.shape)}")
        out = dict(x_new=np.zeros((nprof, n)), post_var=np.zeros((nprof, n)), avk_diag=np.zeros((nprof, n)), chi2=np.zeros(nprof),
                   status=np.zeros(nprof, np.int32))
        shapes = dict(gain_t=(nprof, m, n), avk=(nprof, n, n), post_cov=(nprof, n, n), dofs=(nprof,))
        out.update({w: np.zeros(shapes[w]) for w in want})
        self._chk(self.lib.monortm_hip_oe_step_full(self.ctx, nprof, nv, nc, lm, nj, n, _ptr(kind), _ptr(row), *[_ptr(k) for k in K], _ptr(Y),
                                                    _ptr(yo), _ptr(x), _ptr(xa), _ptr(Sa), int(Sa.ndim == 3), _ptr(Se), se_kind, se_pp, _ptr(gamma),
                                                    *[_ptr(out[k]) for k in ("x_new", "post_var", "avk_diag", "chi2", "status")],
                                                    *[_ptr(out[w]) if w in want else None for w in OE_FULL_WANT]))
        return out

    # ---- the step that carries the dual vector of the adaptive loop (monortm_hip_oe_step_lm) -------------------------
    def oe_step_lm(self, jac: dict, state, y_obs, x, xa, Sa, Se, gamma=None, c=None, want=(), se_kind=None) -> dict:
        """oe_step_full plus the dual vector of the iterate: c [nprof, nstate] = Sa^-1 (x - xa), None for 0 (x = xa).  The dict of
        oe_step_full and c_new [nprof, nstate] = Sa^-1 (x_new - xa) and cost [nprof] = chi2 + c . (x - xa), the cost at x; a failed
        profile has c_new = c and cost = 0."""
        want = _oe_want(want)
        kt = jac["k_t"]
        nprof, nv, lm, nc = kt.shape
        kw = jac.get("k_w")
        nj = 0 if kw is None else kw.shape[3]
        kind, row = _oe_map_of(state, lm, jac.get("vars", ()))
        n, m = len(kind), nv * nc
        f = lambda a: None if a is None else _np(a)  # noqa: E731
        K = [f(jac.get(k)) for k in ("k_t", "k_tz", "k_w", "k_clw", "k_sfc")]
        if nj == 0:
            K[2] = None
        Y, yo, x, xa, Sa, Se, gamma, c = (f(a) for a in (jac["y"], y_obs, x, xa, Sa, Se, gamma, c))
        se_kind, se_pp = oe_se_kind(Se.shape, nprof, m, se_kind)
        for name, a, shapes in (("y_obs", yo, [(nprof, nv, nc)]), ("x", x, [(nprof, n)]), ("xa", xa, [(nprof, n)]), ("Sa", Sa, [(n, n), (nprof, n, n)]),
                                ("gamma", gamma, [(nprof,)]), ("c", c, [(nprof, n)])):
            if a is not None and a.shape not in shapes:
                raise ValueError(f"{name} must be {' or '.join(str(list(s)) for s in shapes)}, got {list(a.shape)}")
        out = dict(x_new=np.zeros((nprof, n)), post_var=np.zeros((nprof, n)), avk_diag=np.zeros((nprof, n)), chi2=np.zeros(nprof),
                   status=np.zeros(nprof, np.int32), c_new=np.zeros((nprof, n)), cost=np.zeros(nprof))
        shapes = dict(gain_t=(nprof, m, n), avk=(nprof, n, n), post_cov=(nprof, n, n), dofs=(nprof,))
        out.update({w: np.zeros(shapes[w]) for w in want})
        self._chk(self.lib.monortm_hip_oe_step_lm(self.ctx, nprof, nv, nc, lm, nj, n, _ptr(kind), _ptr(row), *[_ptr(k) for k in K], _ptr(Y),
                                                  _ptr(yo), _ptr(x), _ptr(xa), _ptr(Sa), int(Sa.ndim == 3), _ptr(Se), se_kind, se_pp, _ptr(gamma),
                                                  *[_ptr(out[k]) for k in ("x_new", "post_var", "avk_diag", "chi2", "status")],
                                                  *[_ptr(out[w]) if w in want else None for w in OE_FULL_WANT], _ptr(c), _ptr(out["c_new"]),
                                                  _ptr(out["cost"])))
        return out

    # ---- the forward measurement operator (monortm_hip_rtm_obs / monortm_hip_obs) ------------------------------
    def rtm_obs(self, profiles: list[Profile], O: np.ndarray, path, obs: int, quantity="tb", emiss=None, reflc=None, vcen=None) -> dict:
        """y = F(x) per measurement from one O [nprof, nlay_max, nwn]: the radiances of rtm_scan contracted with the operator `obs`
        (a handle of obs_create) inside the kernel, in the fixed order of rtm_obs_jacobian's y.  quantity: "rad", "tb" (the mean of the
        monochromatic brightness temperatures) or "band_tb" (the contracted radiance converted at the channels' nominal wavenumbers
        vcen [nchan]: see band_tb; the weights must be normalised per measurement).  Works for both real kinds and for an O of
        modm() with cross-section molecules.  Dict of y [nprof, nview, nchan]."""
        q = _quantity(quantity, band=True)
        nv, nc = self._obs_shape(obs)
        vc = _vcen(vcen, q, nc)
        nprof, nwn, nlay, lm, irt, T, TZ, ts, em, rf = self._pack_rtm(profiles)
        dt = self.dtype
        f = self._path(path, nprof, lm)
        npath = f.shape[1]
        em, rf = self._scan_sfc(em, rf, emiss, reflc, nprof, npath, nwn)
        O = _np(O, dt)
        if O.shape != (nprof, lm, nwn):
            raise ValueError(f"O must be [{nprof}, {lm}, {nwn}], got {O.shape}")
        out = dict(y=np.zeros((nprof, nv, nc), dt))
        wn = _np(profiles[0].wn)
        self._chk(self.lib.monortm_hip_rtm_obs(self.ctx, nprof, npath, nwn, _ptr(wn), _ptr(nlay), lm, _ptr(irt), q, _ptr(T), _ptr(TZ), _ptr(O),
                                               _ptr(f), _ptr(ts), int(em.ndim == 3), _ptr(em), _ptr(rf), int(obs), _ptr(vc),
                                               *[_ptr(out[k]) for k in OBS_RTM_FIELDS]))
        return out

    def obs(self, profiles: list[Profile], path, obs: int, quantity="tb", emiss=None, reflc=None, vcen=None) -> dict:
        """MODM ONCE + the forward measurement operator (both real kinds): dict of o [nprof, nlay_max, nwn] (the vertical optical
        depths, as modm() returns them) and y [nprof, nview, nchan]; the arguments of rtm_obs."""
        q = _quantity(quantity, band=True)
        nv, nc = self._obs_shape(obs)
        vc = _vcen(vcen, q, nc)
        rtm = self._pack_rtm(profiles)
        nprof, nwn, _, lm, _, _, _, _, em, rf = rtm
        dt = self.dtype
        f = self._path(path, nprof, lm)
        npath = f.shape[1]
        em, rf = self._scan_sfc(em, rf, emiss, reflc, nprof, npath, nwn)
        out = dict(o=np.zeros((nprof, lm, nwn), dt), y=np.zeros((nprof, nv, nc), dt))
        self._chk(self.lib.monortm_hip_obs(*self._full_args(profiles, rtm, self._pack_atm(profiles, lm), em, rf), q, npath, _ptr(f),
                                           int(em.ndim == 3), int(obs), _ptr(vc), *[_ptr(out[k]) for k in OBS_FIELDS]))
        return out

    # ---- the C-ABI gather of a profile-sharded job (RCCL; what a C / Fortran caller uses instead of torch.distributed) ------
    @staticmethod
    def comm_unique_id() -> bytes:
        """128-byte ncclUniqueId generated by this process (rank 0 of the job)."""
        buf = C.create_string_buffer(128)
        if load_library().monortm_hip_comm_unique_id(buf) != 0:
            raise MonoRTMError(7, "RCCL cannot be loaded or ncclGetUniqueId failed")
        return buf.raw

    def comm_init(self, world: int, rank: int, uid: bytes) -> None:
        self._chk(self.lib.monortm_hip_comm_init(self.ctx, world, rank, C.create_string_buffer(uid, 128)))

    def gather_dev(self, send, recv, root: int = 0, stream: int = 0) -> None:
        """send / recv: torch tensors on this context's device; recv (root only) holds world x send.numel() elements."""
        nbytes = send.numel() * send.element_size()
        self._chk(self.lib.monortm_hip_gather_dev(self.ctx, C.c_void_p(send.data_ptr()), nbytes,
                                                  C.c_void_p(recv.data_ptr()) if recv is not None else None, root, C.c_void_p(stream)))

    def set_option(self, name: str, value) -> None:
        """Measurement switches of the context (monortm_hip_set_option): nslice, fair, tile_waves, far_levels, lines_kernel = auto | wn |
        ms, ms_items, ms_prepare = auto | fused | passes, ms_plan = auto | on | off, finish_mw = auto | layer | column, jac_dt, jac_dlnw, and finish = auto | generic (generic: finish_kernel also below 820 cm-1, where finish_mw_kernel
        serves by default; the environment variable MONORTM_FINISH_GENERIC makes it the default of a new context)."""
        self._chk(self.lib.monortm_hip_set_option(self.ctx, name.encode(), str(value).encode()))

    def kat(self, which: int, args: np.ndarray, tab: np.ndarray | None = None) -> np.ndarray:
        """Known-answer hook: device versions of W4 / SD_Humlicek / SDVOIGT / RADFN / AtoB / ODCLW_TKC / TIPS / HALFWHM_D / bb_fn and
        (which = 10, 11) the radiance kernels' exp_cw / rcp2, args [n,4] -> [n,2]."""
        a = _np(args)
        t = _np(tab) if tab is not None else None
        out = np.zeros((len(a), 2))
        self._chk(self.lib.monortm_hip_kat(self.ctx, which, len(a), _ptr(a), _ptr(t), _ptr(out)))
        return out

    # ---- timing of the kernels on the launch stream ----------------------------------------------
    def profile(self, mask: int = 7, stride: int = 1):
        """bit 0 lines kernel, bit 1 continuum/cloud/total kernel, bit 2 rtm kernel; 0 = off.  stride n: only every n-th
        launch of a selected kernel is bracketed by events"""
        self._chk(self.lib.monortm_hip_profile(self.ctx, int(mask) | (max(1, int(stride)) << 8)))

    def kernel_time(self, kernel: int):
        ms = C.c_double()
        n = C.c_longlong()
        self._chk(self.lib.monortm_hip_kernel_time(self.ctx, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class DeviceBatch:
    """A batch of profiles resident in HBM; ``step()`` is one pass of the hot path (MODM + CALCTMR + RTM)
    with no host<->device traffic.  torch owns the buffers and the stream - nothing else."""

    def __init__(self, rt: MonoRTM, profiles: list[Profile], device: str = "cuda:0"):
        import torch

        self.torch = torch
        self.rt = rt
        self.dev = torch.device(device)
        p0 = profiles[0]
        self.p0 = p0
        self.nprof, self.nwn, self.nmol = len(profiles), p0.nwn, p0.nmol
        nlay = np.array([p.nlay for p in profiles], np.int32)
        self.lm = lm = int(nlay.max())
        f64 = torch.float32 if rt.real_kind == 4 else torch.float64  # dtype of the REAL arrays

        def up(a, dt=f64):
            return torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(self.dev)

        def pack(get, width=None):
            return pack_layers(profiles, lm, get, width)

        self.wn = up(p0.wn, torch.float64)
        self.nlay = up(nlay, torch.int32)
        self.irt = up(np.array([p.irt for p in profiles], np.int32), torch.int32)
        self.P, self.T, self.CLW, self.WB = (up(pack(g)) for g in (lambda p: p.p, lambda p: p.t, lambda p: p.clw,
                                                                  lambda p: p.wbrodl))
        self.WKL = up(pack(lambda p: p.wkl, self.nmol))
        tz = np.zeros((self.nprof, lm + 1))
        for i, p in enumerate(profiles):
            tz[i, : p.nlay + 1] = p.tz
        self.TZ = up(tz)
        self.tmpsfc0 = up(np.array([p.tmpsfc for p in profiles]))
        self.tmpsfc = self.tmpsfc0.clone()
        self.emiss = up(np.stack([p.emiss for p in profiles]))
        self.reflc = up(np.stack([p.reflc for p in profiles]))
        z = lambda *s: torch.zeros(*s, dtype=f64, device=self.dev)  # noqa: E731
        self.O = z(self.nprof, lm, self.nwn)
        self.OBM = z(self.nprof, lm, self.nmol, self.nwn)
        self.OC = z(self.nprof, lm, NCONT, self.nwn)
        self.OCLW = z(self.nprof, lm, self.nwn)
        # the six spectral outputs of a step live in ONE block [6, nprof, nwn] (RAD, TB, TRTOT, TMR, RUP, RDN: the order of
        # spectral_outputs()), so that a profile-sharded job can hand the block to its gather as it is - no stack, no copy on the
        # compute stream.  Two blocks: with `pingpong` a step writes the block the step before did NOT write, so the gather of step k
        # reads its block while step k + 1 runs (distributed.GatherPlan, field_major=True).
        self._spec = [z(6, self.nprof, self.nwn), z(6, self.nprof, self.nwn)]
        self._cur = 0
        self.pingpong = False
        self._bind_spectral()
        self.fac = _np(p0.cntnm)
        self.wn_ends = _np([p0.wn[0], p0.wn[-1]])  # host copy: keeps step() free of device->host traffic
        self.nlay_total = int(nlay.sum())
        self._scan = {}  # npath -> (output block, device copy of the factors) of scan()

    def _bind_spectral(self):
        b = self._spec[self._cur]
        self.RAD, self.TB, self.TRTOT, self.TMR, self.RUP, self.RDN = (b[k] for k in range(6))

    def spectral_block(self):
        """The [6, nprof, nwn] block the last step wrote (RAD, TB, TRTOT, TMR, RUP, RDN), contiguous, no copy."""
        return self._spec[self._cur]

    def _modm_args(self):
        """The leading arguments of the *_dev entries that run MODM on the resident batch: ctx, nprof ... ibrd."""
        p0 = self.p0
        d = lambda x: _vp(x.data_ptr())  # noqa: E731
        return (self.rt.ctx, self.nprof, self.nwn, d(self.wn), p0.dvset, d(self.nlay), self.lm, self.nmol, d(self.P), d(self.T), d(self.CLW),
                d(self.WKL), d(self.WB), _ptr(self.fac), p0.sclcpl, p0.sclhw, p0.y0res, p0.ibrd)

    def _sfc_args(self):
        """... and what follows ibrd in the full Jacobian entries: irt, TZ, the profiles' own TMPSFC (input only), emiss, reflc."""
        return tuple(_vp(x.data_ptr()) for x in (self.irt, self.TZ, self.tmpsfc0, self.emiss, self.reflc))

    def _modm(self, sp):
        """MODM of the resident batch into its O, OBM, OC, OCLW, on the stream sp."""
        d = lambda x: _vp(x.data_ptr())  # noqa: E731
        self.rt._chk(self.rt.lib.monortm_hip_modm_dev(*self._modm_args(), 0, d(self.O), d(self.OBM), d(self.OC), d(self.OCLW), _ptr(self.wn_ends),
                                                      sp))

    def _path(self, path):
        """The factors of a scan as a tensor [nprof, npath, nlay_max] (a view where [npath, nlay_max] was given): ValueError otherwise."""
        f = self.torch.as_tensor(path)
        if f.dim() == 2:
            f = f.unsqueeze(0).expand(self.nprof, -1, -1)
        if f.dim() != 3 or f.shape[0] != self.nprof or f.shape[1] < 1 or f.shape[2] != self.lm:
            raise ValueError(f"path must be [npath, {self.lm}] or [{self.nprof}, npath, {self.lm}], got {tuple(f.shape)}")
        return f

    def step(self, stream=None):
        t = self.torch
        if self.pingpong:   # (not under graph capture: a captured step keeps the block it was recorded with)
            self._cur ^= 1
            self._bind_spectral()
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        sp = _vp(s.cuda_stream)
        p0, lib, rt = self.p0, self.rt.lib, self.rt
        d = lambda x: _vp(x.data_ptr())  # noqa: E731
        self._modm(sp)
        rt._chk(lib.monortm_hip_rtm_dev(rt.ctx, self.nprof, self.nwn, d(self.wn), d(self.nlay), self.lm, d(self.irt), p0.iout,
                                        d(self.T), d(self.TZ), d(self.O), d(self.tmpsfc), d(self.emiss), d(self.reflc),
                                        d(self.RUP), d(self.RDN), d(self.TRTOT), d(self.RAD), d(self.TB), d(self.TMR), sp))

    # ---- Jacobians on the resident batch (monortm_hip_jacobian_dev) ---------------------------------------------------------------
    def jacobian(self, mols=(1,), quantity="tb", stream=None) -> dict:
        """K of the batch's profiles on the current (or the given) stream, asynchronously: a dict of torch tensors with the fields and
        shapes of MonoRTM.jacobian, allocated at the first call for (mols, quantity) and overwritten by every later one (so that a
        graph capture of the call replays into the same tensors).  TMPSFC is the profiles' own (input only)."""
        t = self.torch
        key = (tuple(int(m) for m in jac_codes(mols)), _quantity(quantity))
        cache = self.__dict__.setdefault("_jac", {})
        if key not in cache:
            f64 = t.float32 if self.rt.real_kind == 4 else t.float64
            z = lambda *s: t.zeros(*s, dtype=f64, device=self.dev)  # noqa: E731
            n, lm, nw, nj = self.nprof, self.lm, self.nwn, len(key[0])
            cache[key] = (dict(o=z(n, lm, nw), rad=z(n, nw), tb=z(n, nw), k_t=z(n, lm, nw), k_tz=z(n, lm + 1, nw), k_w=z(n, lm, nj, nw),
                               k_clw=z(n, lm, nw), k_o=z(n, lm, nw), k_sfc=z(n, 3, nw)), np.ascontiguousarray(key[0], np.int32))
        out, jm = cache[key]
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        rt = self.rt
        d = lambda x: _vp(x.data_ptr())  # noqa: E731
        nj = len(jm)
        rt._chk(rt.lib.monortm_hip_jacobian_dev(*self._modm_args(), *self._sfc_args(), key[1], nj, _ptr(jm) if nj else None,
                                                *[d(out[k]) if (k != "k_w" or nj) else None for k in JAC_FIELDS],
                                                _ptr(self.wn_ends), _vp(s.cuda_stream)))
        out["vars"] = t.from_numpy(jm.copy())   # (a host tensor: the codes in slot order)
        return out

    # ---- path scans on the resident batch (monortm_hip_modm_dev + monortm_hip_rtm_scan_dev) ---------------------------------------
    def scan(self, path, stream=None):
        """MODM once and the radiances along npath paths per profile, on the current (or the given) stream, asynchronously.
        path: [npath, nlay_max] or [nprof, npath, nlay_max] (numpy or a torch tensor).  Returns one [6, nprof, npath, nwn] block in
        the order of spectral_block() (RAD, TB, TRTOT, TMR, RUP, RDN), allocated at the first call for that npath and overwritten
        by every later one, as is the device copy of the factors (so that a graph capture of the call replays into the same
        tensors).  A torch tensor on the batch's device is copied on the stream: only then is the call asynchronous and fit for
        a graph capture.  A numpy array or a host tensor is uploaded from pageable memory, which blocks the host on every call
        and cannot be captured.  Bad factors surface through check()."""
        t = self.torch
        real = t.float32 if self.rt.real_kind == 4 else t.float64  # dtype of the REAL arrays
        f = self._path(path)
        npath = int(f.shape[1])
        if npath not in self._scan:
            self._scan[npath] = (t.zeros(6, self.nprof, npath, self.nwn, dtype=real, device=self.dev),
                                 t.zeros(self.nprof, npath, self.lm, dtype=real, device=self.dev))
        blk, fd = self._scan[npath]
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        with t.cuda.stream(s):
            fd.copy_(f, non_blocking=True)
        sp = _vp(s.cuda_stream)
        p0, lib, rt = self.p0, self.rt.lib, self.rt
        d = lambda x: _vp(x.data_ptr())  # noqa: E731
        rad, tb, trtot, tmr, rup, rdn = (blk[k] for k in range(6))
        self._modm(sp)
        rt._chk(lib.monortm_hip_rtm_scan_dev(rt.ctx, self.nprof, npath, self.nwn, d(self.wn), d(self.nlay), self.lm, d(self.irt), p0.iout,
                                             d(self.T), d(self.TZ), d(self.O), d(fd), d(self.tmpsfc), 0, d(self.emiss), d(self.reflc),
                                             d(rup), d(rdn), d(trtot), d(rad), d(tb), d(tmr), sp))
        return blk

    # ---- Jacobians of path scans on the resident batch (monortm_hip_scan_jacobian_dev) ----------------------------------------------
    def scan_jacobian(self, path, mols=(1,), quantity="tb", stream=None) -> dict:
        """K along npath paths per profile on the current (or the given) stream, asynchronously: a dict of torch tensors with the
        fields and shapes of MonoRTM.scan_jacobian.  The outputs and the device copy of the factors are allocated at the first call
        for (npath, mols, quantity) and overwritten by every later one, so that a graph capture of the call (after one warm call, with
        the factors in a tensor on the batch's device) replays into the same tensors.  path as DeviceBatch.scan; TMPSFC is the
        profiles' own (input only).  Bad factors surface through check()."""
        t = self.torch
        real = t.float32 if self.rt.real_kind == 4 else t.float64  # dtype of the REAL arrays
        f = self._path(path)
        npath = int(f.shape[1])
        key = (npath, tuple(int(m) for m in jac_codes(mols)), _quantity(quantity))
        cache = self.__dict__.setdefault("_scan_jac", {})
        if key not in cache:
            n, lm, nw, nj = self.nprof, self.lm, self.nwn, len(key[1])
            z = lambda *s: t.zeros(*s, dtype=real, device=self.dev)  # noqa: E731
            zp = lambda *s: z(n, npath, *s)  # noqa: E731
            cache[key] = (dict(o=z(n, lm, nw), rad=zp(nw), tb=zp(nw), k_t=zp(lm, nw), k_tz=zp(lm + 1, nw), k_w=zp(lm, nj, nw), k_clw=zp(lm, nw),
                               k_o=zp(lm, nw), k_path=zp(lm, nw), k_sfc=zp(3, nw)), np.ascontiguousarray(key[1], np.int32), z(n, npath, lm))
        out, jm, fd = cache[key]
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        with t.cuda.stream(s):
            fd.copy_(f, non_blocking=True)
        rt = self.rt
        d = lambda x: _vp(x.data_ptr())  # noqa: E731
        nj = len(jm)
        rt._chk(rt.lib.monortm_hip_scan_jacobian_dev(*self._modm_args(), *self._sfc_args(), key[2], nj, _ptr(jm) if nj else None, npath, d(fd), 0,
                                                     *[d(out[k]) if (k != "k_w" or nj) else None for k in SCAN_JAC_FIELDS],
                                                     _ptr(self.wn_ends), _vp(s.cuda_stream)))
        out["vars"] = t.from_numpy(jm.copy())   # (a host tensor: the codes in slot order)
        return out

    # ---- channel- and beam-averaged Jacobians on the resident batch (monortm_hip_obs_jacobian_dev) --------------------------------------
    def obs_jacobian(self, path, obs: int, mols=(1,), quantity="tb", stream=None) -> dict:
        """K per measurement on the current (or the given) stream, asynchronously: a dict of torch tensors with the fields and shapes
        of MonoRTM.obs_jacobian; obs is a handle of rt.obs_create.  The outputs and the device copy of the factors are allocated at
        the first call for (obs, npath, mols, quantity), overwritten by every later one and dropped at the first call after
        rt.obs_destroy(obs), so that a graph capture of the call (after
        one warm call, with the factors in a tensor on the batch's device) replays into the same tensors.  path as DeviceBatch.scan;
        no monochromatic or per-path K is allocated anywhere.  Bad factors surface through check()."""
        t = self.torch
        real = t.float32 if self.rt.real_kind == 4 else t.float64  # dtype of the REAL arrays
        f = self._path(path)
        npath = int(f.shape[1])
        key = (int(obs), npath, tuple(int(m) for m in jac_codes(mols)), _quantity(quantity))
        cache = self.__dict__.setdefault("_obs_jac", {})
        live = self.rt.__dict__.get("_obs", {})
        for k in [k for k in cache if k[0] not in live]:   # operators destroyed since: handles are never reused, let their tensors go
            del cache[k]
        if key not in cache:
            nv, nc = self.rt._obs_shape(obs)
            n, lm, nw, nj = self.nprof, self.lm, self.nwn, len(key[2])
            z = lambda *s: t.zeros(*s, dtype=real, device=self.dev)  # noqa: E731
            zv = lambda *s: z(n, nv, *s, nc)  # noqa: E731
            cache[key] = (dict(o=z(n, lm, nw), y=zv(), k_t=zv(lm), k_tz=zv(lm + 1), k_w=zv(lm, nj), k_clw=zv(lm), k_sfc=zv(3)),
                          np.ascontiguousarray(key[2], np.int32), z(n, npath, lm))
        out, jm, fd = cache[key]
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        with t.cuda.stream(s):
            fd.copy_(f, non_blocking=True)
        rt = self.rt
        d = lambda x: _vp(x.data_ptr())  # noqa: E731
        nj = len(jm)
        rt._chk(rt.lib.monortm_hip_obs_jacobian_dev(*self._modm_args(), *self._sfc_args(), key[3], nj, _ptr(jm) if nj else None, npath, d(fd), 0,
                                                    int(obs), *[d(out[k]) if (k != "k_w" or nj) else None for k in OBS_JAC_FIELDS],
                                                    _ptr(self.wn_ends), _vp(s.cuda_stream)))
        out["vars"] = t.from_numpy(jm.copy())   # (a host tensor: the codes in slot order)
        return out

    # ---- the forward measurement operator on the resident batch (monortm_hip_modm_dev + monortm_hip_rtm_obs_dev) ------------------------
    def obs(self, path, obs: int, quantity="tb", vcen=None, stream=None):
        """y = F(x) per measurement on the current (or the given) stream, asynchronously: the batch's MODM step (into its resident O,
        as step() and scan() run it), then the forward kernel on that O.  Returns y [nprof, nview, nchan], a torch tensor; obs is a
        handle of rt.obs_create, quantity and vcen as MonoRTM.obs.  The output, the device copy of the factors and of vcen are
        allocated at the first call for (obs, npath, quantity), overwritten by every later one and dropped at the first call after
        rt.obs_destroy(obs), so that a graph capture of the call (after one warm call, with the factors in a tensor on the batch's
        device) replays into the same tensor.  path as DeviceBatch.scan; TMPSFC is the profiles' own (input only).  Bad factors and a
        bad vcen surface through check()."""
        t = self.torch
        real = t.float32 if self.rt.real_kind == 4 else t.float64  # dtype of the REAL arrays
        q = _quantity(quantity, band=True)
        f = self._path(path)
        npath = int(f.shape[1])
        key = (int(obs), npath, q)
        cache = self.__dict__.setdefault("_obs_fwd", {})
        live = self.rt.__dict__.get("_obs", {})
        for k in [k for k in cache if k[0] not in live]:   # operators destroyed since: handles are never reused, let their tensors go
            del cache[k]
        nv, nc = self.rt._obs_shape(obs)
        if key not in cache:
            cache[key] = (t.zeros(self.nprof, nv, nc, dtype=real, device=self.dev), t.zeros(self.nprof, npath, self.lm, dtype=real, device=self.dev),
                          t.ones(nc, dtype=t.float64, device=self.dev) if q == 2 else None)
        y, fd, vd = cache[key]
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        with t.cuda.stream(s):
            fd.copy_(f, non_blocking=True)
            if q == 2:
                if vcen is None:
                    raise ValueError("quantity 'band_tb' needs vcen [nchan], the channels' nominal wavenumbers")
                v = t.as_tensor(vcen)
                if tuple(v.shape) != (nc,):
                    raise ValueError(f"vcen must be [{nc}], got {tuple(v.shape)}")
                vd.copy_(v, non_blocking=True)
        sp = _vp(s.cuda_stream)
        p0, lib, rt = self.p0, self.rt.lib, self.rt
        d = lambda x: _vp(x.data_ptr())  # noqa: E731
        self._modm(sp)
        rt._chk(lib.monortm_hip_rtm_obs_dev(rt.ctx, self.nprof, npath, self.nwn, d(self.wn), d(self.nlay), self.lm, d(self.irt), q,
                                            d(self.T), d(self.TZ), d(self.O), d(fd), d(self.tmpsfc0), 0, d(self.emiss), d(self.reflc),
                                            int(obs), d(vd) if q == 2 else None, d(y), sp))
        return y

    # ---- the optimal-estimation step on device tensors (monortm_hip_oe_step_dev) --------------------------------
    def oe_step(self, jac: dict, state, y_obs, x, xa, Sa, se, gamma=None, stream=None) -> dict:
        """MonoRTM.oe_step on torch tensors, on the current (or the given) stream, asynchronously: jac is the dict obs_jacobian returned,
        every other array a contiguous float64 tensor on the batch's device (nothing is copied or converted: ValueError otherwise).
        The outputs - x_new, post_var, avk_diag, dfs, chi2, status - are allocated at the first call for (nprof, nview, nchan, nstate)
        and overwritten by every later one, so that a graph capture of the call (after one warm call with the same state map) replays
        into the same tensors.  A failed profile is status 1, never an error of check()."""
        t = self.torch
        kt = jac["k_t"]
        nprof, nv, lm, nc = (int(v) for v in kt.shape)
        kw = jac.get("k_w")
        nj = 0 if kw is None else int(kw.shape[3])
        vars = jac.get("vars", ())
        kind, row = _oe_map_of(state, lm, vars.numpy() if isinstance(vars, t.Tensor) else vars)
        n, m = len(kind), nv * nc
        K = [jac.get(k) for k in ("k_t", "k_tz", "k_w", "k_clw", "k_sfc")]
        if nj == 0:
            K[2] = None
        for name, a, shapes in [("y_obs", y_obs, [(nprof, nv, nc)]), ("x", x, [(nprof, n)]), ("xa", xa, [(nprof, n)]), ("Sa", Sa, [(n, n), (nprof, n, n)]),
                                ("se", se, [(m,), (nprof, m)]), ("gamma", gamma, [(nprof,)]), ("y", jac["y"], [(nprof, nv, nc)])] + \
                               [(f"K[{i}]", k, None) for i, k in enumerate(K)]:
            if a is None and (name == "gamma" or name.startswith("K[")):
                continue
            if not isinstance(a, t.Tensor) or a.dtype != t.float64 or a.device != self.dev or not a.is_contiguous():
                raise ValueError(f"{name} must be a contiguous float64 tensor on {self.dev}")
            if shapes is not None and tuple(a.shape) not in shapes:
                raise ValueError(f"{name} must be {' or '.join(str(list(s)) for s in shapes)}, got {list(a.shape)}")
        cache = self.__dict__.setdefault("_oe", {})
        key = (nprof, nv, nc, n)
        if key not in cache:
            z = lambda *s: t.zeros(*s, dtype=t.float64, device=self.dev)  # noqa: E731
            cache[key] = dict(x_new=z(nprof, n), post_var=z(nprof, n), avk_diag=z(nprof, n), dfs=z(nprof), chi2=z(nprof),
                              status=t.zeros(nprof, dtype=t.int32, device=self.dev))
        out = cache[key]
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        rt = self.rt
        d = lambda a: None if a is None else _vp(a.data_ptr())  # noqa: E731
        rt._chk(rt.lib.monortm_hip_oe_step_dev(rt.ctx, nprof, nv, nc, lm, nj, n, _ptr(kind), _ptr(row), *[d(k) for k in K], d(jac["y"]), d(y_obs),
                                               d(x), d(xa), d(Sa), int(Sa.dim() == 3), d(se), int(se.dim() == 2), d(gamma),
                                               *[d(out[k]) for k in ("x_new", "post_var", "avk_diag", "chi2", "status")], _vp(s.cuda_stream)))
        with t.cuda.stream(s):
            t.sum(out["avk_diag"], dim=1, out=out["dfs"])
        return dict(out)

    def oe_step_full(self, jac: dict, state, y_obs, x, xa, Sa, Se, gamma=None, want=("avk", "post_cov", "dofs"), stream=None, se_kind=None) -> dict:
        """MonoRTM.oe_step_full on torch tensors, asynchronously, under the rules of oe_step: Se [nmeas] or [nprof, nmeas] (variances),
        [nmeas, nmeas] or [nprof, nmeas, nmeas] (covariance, lower triangle read) - oe_se_kind decides, ValueError where it cannot (se_kind).
        The outputs - x_new, post_var, avk_diag, chi2, status and the diagnostics in `want` ("gain_t", "avk", "post_cov", "dofs") - are
        allocated at the first call for (nprof, nview, nchan, nstate, want) and overwritten by every later one: a graph capture of the
        call (after one warm call) replays into the same tensors."""
        return self._oe_step_dev(jac, state, y_obs, x, xa, Sa, Se, gamma, want, stream, se_kind)

    def oe_step_lm(self, jac: dict, state, y_obs, x, xa, Sa, Se, gamma=None, c=None, want=(), stream=None, se_kind=None) -> dict:
        """MonoRTM.oe_step_lm on torch tensors, asynchronously, under the rules of oe_step_full: c [nprof, nstate] or None (0).  The
        outputs of oe_step_full plus c_new [nprof, nstate] and cost [nprof], tensors of this entry's own, allocated at the first call for
        (nprof, nview, nchan, nstate, want) and overwritten by every later one."""
        return self._oe_step_dev(jac, state, y_obs, x, xa, Sa, Se, gamma, want, stream, se_kind, dual=True, c=c)

    def _oe_step_dev(self, jac, state, y_obs, x, xa, Sa, Se, gamma, want, stream, se_kind, dual=False, c=None) -> dict:
        """oe_step_full, or with dual oe_step_lm: one validation, one cache per entry, one call."""
        t = self.torch
        want = _oe_want(want)
        kt = jac["k_t"]
        nprof, nv, lm, nc = (int(v) for v in kt.shape)
        kw = jac.get("k_w")
        nj = 0 if kw is None else int(kw.shape[3])
        vars = jac.get("vars", ())
        kind, row = _oe_map_of(state, lm, vars.numpy() if isinstance(vars, t.Tensor) else vars)
        n, m = len(kind), nv * nc
        K = [jac.get(k) for k in ("k_t", "k_tz", "k_w", "k_clw", "k_sfc")]
        if nj == 0:
            K[2] = None
        for name, a, shapes in [("y_obs", y_obs, [(nprof, nv, nc)]), ("x", x, [(nprof, n)]), ("xa", xa, [(nprof, n)]), ("Sa", Sa, [(n, n), (nprof, n, n)]),
                                ("Se", Se, None), ("gamma", gamma, [(nprof,)]), ("c", c, [(nprof, n)]), ("y", jac["y"], [(nprof, nv, nc)])] + \
                               [(f"K[{i}]", k, None) for i, k in enumerate(K)]:
            if a is None and (name in ("gamma", "c") or name.startswith("K[")):
                continue
            if not isinstance(a, t.Tensor) or a.dtype != t.float64 or a.device != self.dev or not a.is_contiguous():
                raise ValueError(f"{name} must be a contiguous float64 tensor on {self.dev}")
            if shapes is not None and tuple(a.shape) not in shapes:
                raise ValueError(f"{name} must be {' or '.join(str(list(s)) for s in shapes)}, got {list(a.shape)}")
        se_kind, se_pp = oe_se_kind(Se.shape, nprof, m, se_kind)
        cache = self.__dict__.setdefault("_oe_lm" if dual else "_oe_full", {})
        key = (nprof, nv, nc, n, want)
        if key not in cache:
            z = lambda *s: t.zeros(*s, dtype=t.float64, device=self.dev)  # noqa: E731
            shapes = dict(gain_t=(nprof, m, n), avk=(nprof, n, n), post_cov=(nprof, n, n), dofs=(nprof,))
            cache[key] = dict(x_new=z(nprof, n), post_var=z(nprof, n), avk_diag=z(nprof, n), chi2=z(nprof),
                              status=t.zeros(nprof, dtype=t.int32, device=self.dev), **{w: z(*shapes[w]) for w in want})
            if dual:
                cache[key].update(c_new=z(nprof, n), cost=z(nprof))
        out = cache[key]
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        rt = self.rt
        d = lambda a: None if a is None else _vp(a.data_ptr())  # noqa: E731
        entry = rt.lib.monortm_hip_oe_step_lm_dev if dual else rt.lib.monortm_hip_oe_step_full_dev
        rt._chk(entry(rt.ctx, nprof, nv, nc, lm, nj, n, _ptr(kind), _ptr(row), *[d(k) for k in K], d(jac["y"]),
                      d(y_obs), d(x), d(xa), d(Sa), int(Sa.dim() == 3), d(Se), se_kind, se_pp, d(gamma),
                      *[d(out[k]) for k in ("x_new", "post_var", "avk_diag", "chi2", "status")],
                      *[d(out.get(w)) for w in OE_FULL_WANT], *([d(c), d(out["c_new"]), d(out["cost"])] if dual else []), _vp(s.cuda_stream)))
        return dict(out)

    def _oe_resident(self, items):
        """The elements of a retrieval's state by the resident input they live in: [(name, molecule, columns of the state vector, their
        layers / levels, the columns written back, their layers / levels)] - a variable named twice is read into each of its columns and
        written back from the last; ValueError for what retrieve() cannot write back."""
        groups = {}
        for col, (name, code, k) in enumerate(items):
            if name in ("emiss", "reflc"):
                raise ValueError(f"retrieve: a state element {name!r} has no resident scalar to write back (oe_step itself takes it)")
            if name == "w" and not 1 <= code <= self.nmol:
                raise ValueError(f"retrieve: Jacobian variable {code} is not a molecule of the batch (oe_step itself takes it)")
            g = groups.setdefault((name, code), ([], [], {}))
            g[0].append(col)
            g[1].append(0 if k is None else k)
            g[2][0 if k is None else k] = col
        return [(name, code, g[0], g[1], list(g[2].values()), list(g[2].keys())) for (name, code), g in groups.items()]

    def retrieve(self, y_obs, path, obs: int, state, xa, Sa, se=None, gammas=(0,) * 6, mols=None, quantity="tb", keep=False, stream=None,
                 Se=None, diagnostics=()) -> dict:
        """An optimal-estimation retrieval on the resident batch, one iteration per entry of `gammas` (a scalar or [nprof] each):
        obs_jacobian -> oe_step -> x_new written back into the batch's inputs with torch ops; nothing visits the host.  `state` is a spec
        of oe_state_map over ("t", layers), ("tz", levels), ("w", molecule, layers) - ln of the molecule's amounts -, ("clw", layers) and
        ("tmpsfc",); "emiss", "reflc" and Jacobian variables that are no molecule are refused (ValueError).  The first iterate is what the
        batch holds.  Written back: T, TZ, CLW and TMPSFC as they are, WKL[..., mol] = exp(x); only layers < nlay[p] (levels <= nlay[p]).
        mols: the Jacobian's variables (default: the molecules of the spec, in the order it names them).  y_obs, xa, Sa, se as oe_step.
        Returns the dict of the last oe_step, plus x (the iterate that step started from), chi2_history [len(gammas), nprof] and, with
        keep=True, kept: per iteration, clones of y, the k_*, x, x_new and gamma.
        Se (in place of se: any shape oe_step_full takes) and / or diagnostics (names of oe_step_full's `want`) send every iteration
        through oe_step_full; the diagnostics are asked for on the last iteration only and come back in the dict."""
        diagnostics = _oe_want(diagnostics)
        if (se is None) == (Se is None):
            raise ValueError("retrieve: give se (variances) or Se (any shape of oe_step_full), not both")
        full = Se is not None or bool(diagnostics)
        t = self.torch
        items = _oe_items(state, self.lm)
        groups = self._oe_resident(items)
        if mols is None:
            mols = tuple(dict.fromkeys(code for name, code, _ in items if name == "w"))
        if not len(gammas):
            raise ValueError("retrieve: gammas is empty")
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        idx = lambda v: t.as_tensor(v, dtype=t.long, device=self.dev)  # noqa: E731
        n = len(items)
        if not isinstance(xa, t.Tensor) or tuple(xa.shape) != (self.nprof, n):
            raise ValueError(f"xa must be a tensor [{self.nprof}, {n}]")
        with t.cuda.stream(s):
            x = xa.clone()   # (elements of layers >= nlay[p] stay at the prior: K is 0 there)
            gam = t.zeros(self.nprof, dtype=t.float64, device=self.dev)
            resident = lambda name, code, ks: (self.tmpsfc0[:, None] if name == "tmpsfc" else self.WKL[:, ks, code - 1] if name == "w"  # noqa: E731
                                               else {"t": self.T, "tz": self.TZ, "clw": self.CLW}[name][:, ks])
            alive = lambda name, ks: ks[None, :] < self.nlay[:, None] + (2 ** 30 if name == "tmpsfc" else 1 if name == "tz" else 0)  # noqa: E731
            plan = []
            for name, code, cols, ks, wcols, wks in groups:
                cols, ks, wcols, wks = idx(cols), idx(ks), idx(wcols), idx(wks)
                v = resident(name, code, ks)
                x[:, cols] = t.where(alive(name, ks), t.log(v) if name == "w" else v.expand(-1, len(cols)), x[:, cols])
                plan.append((name, code, wcols, wks, alive(name, wks)))
            hist, kept, step = [], [], None
            for it, g in enumerate(gammas):
                if isinstance(g, (int, float)):
                    gam.fill_(float(g))
                else:
                    gam.copy_(t.as_tensor(g, dtype=t.float64).expand(self.nprof))
                jac = self.obs_jacobian(path, obs, mols=mols, quantity=quantity, stream=s)
                if full:
                    step = self.oe_step_full(jac, state, y_obs, x, xa, Sa, se if Se is None else Se, gamma=gam,
                                             want=diagnostics if it + 1 == len(gammas) else (), stream=s)
                else:
                    step = self.oe_step(jac, state, y_obs, x, xa, Sa, se, gamma=gam, stream=s)
                hist.append(step["chi2"].clone())
                if keep:
                    kept.append(dict({k: jac[k].clone() for k in ("y", "k_t", "k_tz", "k_w", "k_clw", "k_sfc")}, x=x.clone(), x_new=step["x_new"].clone(),
                                     gamma=gam.clone()))
                xn = step["x_new"]
                for name, code, wcols, wks, live in plan:
                    if name == "tmpsfc":
                        self.tmpsfc0.copy_(xn[:, wcols[0]])
                        self.tmpsfc.copy_(self.tmpsfc0)
                    elif name == "w":
                        self.WKL[:, wks, code - 1] = t.where(live, t.exp(xn[:, wcols]), self.WKL[:, wks, code - 1])
                    else:
                        dst = {"t": self.T, "tz": self.TZ, "clw": self.CLW}[name]
                        dst[:, wks] = t.where(live, xn[:, wcols], dst[:, wks])
                if it + 1 < len(gammas):
                    x.copy_(xn)
        out = dict(step, x=x, chi2_history=t.stack(hist))
        if keep:
            out["kept"] = kept
        return out

    # ---- the adaptive retrieval loop: LM step acceptance per profile, on the device -------------------------------
    def oe_scatter(self, wmap, x_src, x_fallback=None, done=None, lo=None, hi=None, trial_ok=None, stream=None) -> None:
        """monortm_hip_oe_scatter_dev on the batch's resident T, TZ, WKL, CLW and both TMPSFC copies, asynchronously: wmap is the
        triple of oe_write_map; x_src, x_fallback [nprof, nstate] float64, done, trial_ok [nprof] int32, lo, hi [nstate] or [nprof, nstate],
        all contiguous tensors on the batch's device (ValueError otherwise)."""
        t = self.torch
        kind, index, mol = (np.ascontiguousarray(a, np.int32) for a in wmap)
        n = len(kind)
        for name, a, dt, shapes in (("x_src", x_src, t.float64, [(self.nprof, n)]), ("x_fallback", x_fallback, t.float64, [(self.nprof, n)]),
                                    ("done", done, t.int32, [(self.nprof,)]), ("trial_ok", trial_ok, t.int32, [(self.nprof,)]),
                                    ("lo", lo, t.float64, [(n,), (self.nprof, n)]), ("hi", hi, t.float64, [(n,), (self.nprof, n)])):
            if a is None and name != "x_src":
                continue
            if not isinstance(a, t.Tensor) or a.dtype != dt or a.device != self.dev or not a.is_contiguous() or tuple(a.shape) not in shapes:
                raise ValueError(f"{name} must be a contiguous {dt} tensor {' or '.join(str(list(s)) for s in shapes)} on {self.dev}")
        per = [a.dim() == 2 for a in (lo, hi) if a is not None]
        if len(set(per)) > 1:
            raise ValueError("lo and hi must both be [nstate] or both [nprof, nstate]")
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        rt = self.rt
        d = lambda a: None if a is None else _vp(a.data_ptr())  # noqa: E731
        rt._chk(rt.lib.monortm_hip_oe_scatter_dev(rt.ctx, self.nprof, n, _ptr(kind), _ptr(index), _ptr(mol), d(x_src), d(x_fallback), d(done), d(lo),
                                                  d(hi), int(bool(per) and per[0]), d(self.nlay), self.lm, self.nmol, d(self.T), self.lm, d(self.TZ),
                                                  self.lm + 1, d(self.WKL), self.lm * self.nmol, d(self.CLW), self.lm, d(self.tmpsfc0),
                                                  d(self.tmpsfc), d(trial_ok), _vp(s.cuda_stream)))

    def oe_accept(self, y_trial, y_obs, Se, x_trial, c_trial, xa, step_status, trial_ok, loop: dict, up=10.0, down=0.5, gamma_first=1.0,
                  gamma_floor=1e-3, gamma_max=1e8, conv=0.01, last=False, stream=None, se_kind=None) -> None:
        """monortm_hip_oe_accept_dev, asynchronously: the decision on a trial step.  loop holds the state it updates in place - x_cur,
        c_cur [nprof, nstate], J_cur, gamma [nprof] float64 and done, n_acc, n_rej [nprof] int32.  Every array a contiguous tensor on the
        batch's device; Se in any shape of oe_step_full."""
        t = self.torch
        nprof, n = (int(v) for v in x_trial.shape)
        m = int(y_obs.numel()) // nprof
        se_kind, se_pp = oe_se_kind(Se.shape, nprof, m, se_kind)
        f64 = [("y_trial", y_trial, m), ("y_obs", y_obs, m), ("Se", Se, None), ("x_trial", x_trial, n), ("c_trial", c_trial, n), ("xa", xa, n),
               ("x_cur", loop["x_cur"], n), ("c_cur", loop["c_cur"], n), ("J_cur", loop["J_cur"], 1), ("gamma", loop["gamma"], 1)]
        i32 = [(k, v, 1) for k, v in (("step_status", step_status), ("trial_ok", trial_ok), ("done", loop["done"]), ("n_acc", loop["n_acc"]),
                                      ("n_rej", loop["n_rej"]))]
        for dt, group in ((t.float64, f64), (t.int32, i32)):
            for name, a, per in group:
                if not isinstance(a, t.Tensor) or a.dtype != dt or a.device != self.dev or not a.is_contiguous() or \
                        (per is not None and a.numel() != nprof * per):
                    raise ValueError(f"{name} must be a contiguous {dt} tensor of {nprof} x {per} elements on {self.dev}")
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        rt = self.rt
        d = lambda a: _vp(a.data_ptr())  # noqa: E731
        rt._chk(rt.lib.monortm_hip_oe_accept_dev(rt.ctx, nprof, m, n, d(y_trial), d(y_obs), d(Se), se_kind, se_pp, d(x_trial), d(c_trial), d(xa),
                                                 d(step_status), d(trial_ok), float(up), float(down), float(gamma_first), float(gamma_floor),
                                                 float(gamma_max), float(conv), int(bool(last)),
                                                 *[d(loop[k]) for k in ("x_cur", "c_cur", "J_cur", "gamma", "done", "n_acc", "n_rej")], _vp(s.cuda_stream)))

    def lm_start(self, y_obs, path, obs: int, state, xa, Sa, se=None, Se=None, gamma0=0.0, up=10.0, down=0.5, gamma_first=1.0, gamma_floor=1e-3,
                 gamma_max=1e8, conv=0.01, lo=None, hi=None, x0=None, c0=None, mols=None, quantity="tb", stream=None) -> dict:
        """The loop state of retrieve_lm, with the first iterate (xa, or x0 with its dual vector c0) written into the batch: the dict that
        lm_iterate advances.  Its tensors are cached per (nstate, nmeas): a second loop of the same shape allocates nothing."""
        _lm_check(se, Se, x0, c0)
        t = self.torch
        items = _oe_items(state, self.lm)
        wmap = oe_write_map(state, self.lm, self.nmol)
        if mols is None:
            mols = tuple(dict.fromkeys(code for name, code, _ in items if name == "w"))
        n = len(items)
        if not isinstance(xa, t.Tensor) or tuple(xa.shape) != (self.nprof, n):
            raise ValueError(f"xa must be a tensor [{self.nprof}, {n}]")
        nv, nc = self.rt._obs_shape(obs)
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        cache = self.__dict__.setdefault("_lm", {})
        key = (n, nv, nc)
        if key not in cache:
            z = lambda *sh: t.zeros(*sh, dtype=t.float64, device=self.dev)  # noqa: E731
            zi = lambda: t.zeros(self.nprof, dtype=t.int32, device=self.dev)  # noqa: E731
            cache[key] = dict(x_cur=z(self.nprof, n), c_cur=z(self.nprof, n), J_cur=z(self.nprof), gamma=z(self.nprof), done=zi(), n_acc=zi(),
                              n_rej=zi(), trial_ok=zi())
        L = dict(cache[key], y_obs=y_obs, path=path, obs=obs, state=state, wmap=wmap, xa=xa, Sa=Sa, Se=se if Se is None else Se, lo=lo, hi=hi,
                 mols=mols, quantity=quantity, stream=stream,
                 knobs=dict(up=up, down=down, gamma_first=gamma_first, gamma_floor=gamma_floor, gamma_max=gamma_max, conv=conv))
        with t.cuda.stream(s):
            L["x_cur"].copy_(xa if x0 is None else x0)
            if c0 is None:
                L["c_cur"].zero_()
            else:
                L["c_cur"].copy_(c0)
            L["gamma"].copy_(t.as_tensor(gamma0, dtype=t.float64).expand(self.nprof))
            for k in ("J_cur", "done", "n_acc", "n_rej"):
                L[k].zero_()
        self.oe_scatter(wmap, L["x_cur"], stream=s)
        return L

    def lm_iterate(self, L: dict, first=False, last=False) -> dict:
        """One iteration of retrieve_lm on the loop state of lm_start, six steps on one stream with no host branch on device data:
        obs_jacobian; oe_step_lm (first: its cost becomes J_cur); the trial x_new scattered into the batch - x_cur instead where it
        leaves the box or the profile is done; obs; the decision; x_cur scattered.  After one warm call a second allocates nothing on
        the device, and a graph capture of the call replays into the same tensors.  Returns the tensors of this iteration (jac, step, y)."""
        t = self.torch
        s = L["stream"] if L["stream"] is not None else t.cuda.current_stream(self.dev)   # (None: the stream current at this call)
        jac = self.obs_jacobian(L["path"], L["obs"], mols=L["mols"], quantity=L["quantity"], stream=s)
        if "map" not in L:
            L["map"] = _oe_map_of(L["state"], self.lm, jac["vars"].numpy())
        step = self.oe_step_lm(jac, L["map"], L["y_obs"], L["x_cur"], L["xa"], L["Sa"], L["Se"], gamma=L["gamma"], c=L["c_cur"], stream=s)
        if first:
            with t.cuda.stream(s):
                L["J_cur"].copy_(step["cost"])
        self.oe_scatter(L["wmap"], step["x_new"], x_fallback=L["x_cur"], done=L["done"], lo=L["lo"], hi=L["hi"], trial_ok=L["trial_ok"], stream=s)
        y = self.obs(L["path"], L["obs"], quantity=L["quantity"], stream=s)
        self.oe_accept(y, L["y_obs"], L["Se"], step["x_new"], step["c_new"], L["xa"], step["status"], L["trial_ok"], L, last=last, stream=s,
                       **L["knobs"])
        self.oe_scatter(L["wmap"], L["x_cur"], stream=s)
        return dict(jac=jac, step=step, y=y)

    def retrieve_lm(self, y_obs, path, obs: int, state, xa, Sa, se=None, Se=None, maxit=10, gamma0=0.0, up=10.0, down=0.5, gamma_first=1.0,
                    gamma_floor=1e-3, gamma_max=1e8, conv=0.01, lo=None, hi=None, x0=None, c0=None, mols=None, quantity="tb", diagnostics=(),
                    keep=False, stream=None) -> dict:
        """An adaptive optimal-estimation retrieval on the resident batch: up to maxit Levenberg-Marquardt iterations in which every
        profile accepts or rejects its own trial step, adapts its own gamma and stops on its own, all on the device (lm_iterate).  The
        cost J = chi2 + (x - xa)^T Sa^-1 (x - xa) is evaluated through the dual vector c = Sa^-1 (x - xa) that the iterate carries.
        state, y_obs, xa, Sa, se / Se, mols, quantity as retrieve (the same refusals).  The loop starts at xa (c = 0), or at x0 with the
        caller's c0 = Sa^-1 (x0 - xa); gamma0 a scalar or [nprof].  A step is accepted where the trial lies inside [lo, hi] ([nstate]
        or [nprof, nstate] tensors, either may be None), J at the trial is finite and J does not rise: gamma <- gamma down (0 below
        gamma_floor), and the profile has converged (done 1) where J fell by no more than conv x nmeas.  Otherwise gamma <- max(gamma up,
        gamma_first), and the profile stalls (done 4) beyond gamma_max.  done 2: the step itself failed; 3: out of iterations.
        Returns x (the last accepted iterate - what the batch holds), J, gamma, done, n_acc, n_rej [nprof], J_history [maxit + 1, nprof],
        (x, J, gamma, done, n_acc and n_rej ARE the loop's cached buffers: the next retrieve_lm or lm_start of the same shape on this batch
        overwrites them - clone what you keep)
        and from one undamped oe_step_full at x: post_var, avk_diag, chi2, status and the diagnostics asked for (names of oe_step_full's
        `want`).  keep=True: kept, per iteration the clones retrieve keeps plus c, c_new, cost, y_trial, status, the loop state before
        (gamma, J, done) and after (gamma_after, J_after, done_after, n_acc, n_rej, x_after, trial_ok) and the batch's T, TZ, WKL, CLW and
        tmpsfc after the iteration."""
        diagnostics = _oe_want(diagnostics)
        _lm_check(se, Se, x0, c0)
        if int(maxit) < 1:
            raise ValueError("retrieve_lm: maxit must be >= 1")
        t = self.torch
        L = self.lm_start(y_obs, path, obs, state, xa, Sa, se=se, Se=Se, gamma0=gamma0, up=up, down=down, gamma_first=gamma_first,
                          gamma_floor=gamma_floor, gamma_max=gamma_max, conv=conv, lo=lo, hi=hi, x0=x0, c0=c0, mols=mols, quantity=quantity,
                          stream=stream)
        s = stream if stream is not None else t.cuda.current_stream(self.dev)
        with t.cuda.stream(s):
            hist = t.zeros(int(maxit) + 1, self.nprof, dtype=t.float64, device=self.dev)
            kept = []
            for it in range(int(maxit)):
                before = {k: L[k].clone() for k in ("gamma", "J_cur", "done", "x_cur", "c_cur")} if keep else None
                r = self.lm_iterate(L, first=it == 0, last=it + 1 == int(maxit))
                if it == 0:
                    hist[0].copy_(r["step"]["cost"])
                    if keep:
                        before["J_cur"] = r["step"]["cost"].clone()
                hist[it + 1].copy_(L["J_cur"])
                if keep:
                    kept.append(dict({k: r["jac"][k].clone() for k in ("y", "k_t", "k_tz", "k_w", "k_clw", "k_sfc")}, x=before["x_cur"], c=before["c_cur"],
                                     gamma=before["gamma"], J=before["J_cur"], done=before["done"],
                                     **{k: r["step"][k].clone() for k in ("x_new", "c_new", "cost", "status")}, y_trial=r["y"].clone(),
                                     **{k + "_after": L[k].clone() for k in ("gamma", "done")}, J_after=L["J_cur"].clone(), x_after=L["x_cur"].clone(),
                                     **{k: L[k].clone() for k in ("n_acc", "n_rej", "trial_ok")},
                                     **{k: getattr(self, k).clone() for k in ("T", "TZ", "WKL", "CLW", "tmpsfc")}))
            # the posterior belongs to the undamped problem at the final iterate: that call's x_new is discarded
            jac = self.obs_jacobian(L["path"], obs, mols=L["mols"], quantity=quantity, stream=s)
            fin = self.oe_step_full(jac, L["map"], y_obs, L["x_cur"], xa, Sa, L["Se"], gamma=None, want=diagnostics, stream=s)
        out = dict({k: fin[k] for k in ("post_var", "avk_diag", "chi2", "status") + diagnostics}, x=L["x_cur"], J=L["J_cur"], gamma=L["gamma"],
                   done=L["done"], n_acc=L["n_acc"], n_rej=L["n_rej"], J_history=hist)
        if keep:
            out["kept"] = kept
        return out

    # ---- HIP graph: the three launches of a step recorded once, replayed with a single call ------------------
    def capture(self):
        """Record step() into a HIP graph (lines, continuum/cloud/total and rtm kernel nodes).  One warm step runs
        first so that workspace allocations happen outside the capture; kernel-event profiling must be off."""
        t = self.torch
        self.rt.profile(0)
        self.step()
        t.cuda.synchronize(self.dev)
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g):
            self.step()
        self.graph = g
        return g

    def replay(self):
        self.graph.replay()

    def check(self):
        s = self.torch.cuda.current_stream(self.dev)
        self.rt._chk(self.rt.lib.monortm_hip_check(self.rt.ctx, _vp(s.cuda_stream)))

    def dumps(self, profiles: list[Profile]) -> list[Dump]:
        g = lambda x: x.cpu().numpy()  # noqa: E731
        O, OBM, OC, OCLW = g(self.O), g(self.OBM), g(self.OC), g(self.OCLW)
        rup, rdn, trtot, rad, tb, tmr, ts = (g(x) for x in (self.RUP, self.RDN, self.TRTOT, self.RAD, self.TB, self.TMR,
                                                             self.tmpsfc))
        return [Dump(O[i, : p.nlay], OBM[i, : p.nlay], OC[i, : p.nlay], OCLW[i, : p.nlay], rup[i], rdn[i], trtot[i], rad[i],
                     tb[i], tmr[i], float(ts[i])) for i, p in enumerate(profiles)]

    def spectral_outputs(self):
        """[nprof, 6, nwn] tensor (RAD, TB, TRTOT, TMR, RUP, RDN) - what a profile-sharded job gathers (a contiguous copy; the
        zero-copy form is spectral_block())."""
        return self._spec[self._cur].permute(1, 0, 2).contiguous()
