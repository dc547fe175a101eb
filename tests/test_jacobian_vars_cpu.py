"""Jacobian variables without a GPU: the names of api.JAC_VARS, api.jac_codes, and the codes of the C header."""
import os
import re

import numpy as np
import pytest

from monortm_amd import api

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "monortm_hip.h")
CNTNM = ("xself", "xfrgn", "xco2c", "xo3cn", "xo2cn", "xn2cn", "xrayl")   # the order of cntnm_fac[7]
WANT = dict(p=1001, wbrod=1002, sclcpl=1021, sclhw=1022, y0res=1023, **{n: 1011 + i for i, n in enumerate(CNTNM)})


def test_names_and_codes():
    assert api.JAC_VARS == WANT
    assert len(set(api.JAC_VARS.values())) == len(api.JAC_VARS) and min(api.JAC_VARS.values()) > 39   # no molecule number among them
    for name, code in WANT.items():
        got = api.jac_codes([name])
        assert got.dtype == np.int32 and got.tolist() == [code], name
    got = api.jac_codes((1, "p", 3, "xself", np.int64(7), 1022, "Y0RES"))
    assert got.dtype == np.int32 and got.flags.c_contiguous
    assert got.tolist() == [1, 1001, 3, 1011, 7, 1022, 1023]
    assert api.jac_codes(()).shape == (0,) and api.jac_codes(()).dtype == np.int32
    assert api.jac_codes((1, 3)).tolist() == [1, 3]
    assert api.jac_codes(np.array([2, 1], np.int64)).tolist() == [2, 1]
    assert api.jac_codes("wbrod").tolist() == [1002]


@pytest.mark.parametrize("bad", ["pressure", "", "xself ", "h2o", "1"])
def test_unknown_names_raise(bad):
    with pytest.raises(ValueError):
        api.jac_codes((1, bad))


def test_header_defines_equal_jac_vars():
    text = open(HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MONORTM_JVAR_(\w+)\s+(\d+)\b", text, re.M)}
    assert set(defs) == {"P", "WBROD", "CNTNM0", "SCLCPL", "SCLHW", "Y0RES"}, defs
    from_header = {k.lower(): v for k, v in defs.items() if k != "CNTNM0"}
    from_header.update({n: defs["CNTNM0"] + i for i, n in enumerate(CNTNM)})
    assert from_header == api.JAC_VARS
    # the header names the factors behind MONORTM_JVAR_CNTNM0 + i in the order of cntnm_fac[7]
    assert re.search(r"XSELF,\s*XFRGN,\s*XCO2C,\s*XO3CN,\s*XO2CN,\s*XN2CN,\s*XRAYL", text)
