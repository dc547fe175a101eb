"""Channel- and beam-averaged Jacobians (monortm_hip_obs_create, monortm_hip_rtm_obs_jac, monortm_hip_obs_jacobian; DESIGN.md section
3.9), the part that needs no GPU: the operator's validation and dense form in Python, the entry points declared, bound and exported,
and a null context refused by every one of them."""
import ctypes
import os
import re

import numpy as np
import pytest

import obs_cases as oc
from common import ROOT
from monortm_amd import _build, api

SYMBOLS = {"monortm_hip_obs_create": 10, "monortm_hip_obs_destroy": 2, "monortm_hip_rtm_obs_jac": 22, "monortm_hip_rtm_obs_jac_dev": 23,
           "monortm_hip_obs_jacobian": 37, "monortm_hip_obs_jacobian_dev": 39}   # name: arguments


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "monortm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_build.build_hip())
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/monortm_hip.h"
        assert name in api.SYMBOLS, f"{name} is not bound in api.SYMBOLS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert len(m.group(1).split(",")) == nargs == len(api.SYMBOLS[name][1]), name
    assert api.OBS_JAC_RTM_FIELDS == ("y", "k_t", "k_tz", "k_sfc")
    assert api.OBS_JAC_FIELDS == ("o", "y", "k_t", "k_tz", "k_w", "k_clw", "k_sfc")


def test_null_context_is_an_error_not_a_crash():
    """Every new entry point returns MONORTM_EARG for a NULL context (no GPU is touched)."""
    lib = api.load_library()
    z = [None] * 12
    h = ctypes.c_int(5)
    assert lib.monortm_hip_obs_create(None, 1, 1, 1, 1, None, None, None, None, ctypes.byref(h)) == 6
    assert lib.monortm_hip_obs_destroy(None, 1) == 6
    assert lib.monortm_hip_rtm_obs_jac(None, 1, 1, 1, None, None, 1, None, 1, *z[:5], 0, None, None, 1, *z[:4]) == 6
    assert lib.monortm_hip_rtm_obs_jac_dev(None, 1, 1, 1, None, None, 1, None, 1, *z[:5], 0, None, None, 1, *z[:5]) == 6
    assert lib.monortm_hip_obs_jacobian(None, 1, 1, None, 0.0, None, 1, 7, *z[:6], 1.0, 1.0, 0.0, 0, *z[:5], 1, 0, None, 1, None, 0, 1,
                                        *z[:7]) == 6
    assert lib.monortm_hip_obs_jacobian_dev(None, 1, 1, None, 0.0, None, 1, 7, *z[:6], 1.0, 1.0, 0.0, 0, *z[:5], 1, 0, None, 1, None, 0, 1,
                                            *z[:9]) == 6
    assert b"null context" in lib.monortm_hip_last_error(None)


def test_dense_against_a_hand_written_matrix():
    """3 paths in views of 2 / 0 / 1, 4 wavenumbers in channels {0: samples 3 and 0, 1: none, 2: sample 1}, sample 2 unused."""
    op = api.ObsOperator([0, 2, 2, 3], [0.5, -2.0, 3.0], [0, 2, -1, 0], [1.0, 4.0, 9.0, -1.0], nchan=3)
    assert (op.npath, op.nwn, op.nview, op.nchan) == (3, 4, 3, 3)
    W = np.zeros((3, 3, 3, 4))               # [view, channel, path, wavenumber]
    W[0, 0, 0] = 0.5 * np.array([1.0, 0, 0, -1.0])
    W[0, 0, 1] = -2.0 * np.array([1.0, 0, 0, -1.0])
    W[0, 2, 0] = 0.5 * np.array([0, 4.0, 0, 0])
    W[0, 2, 1] = -2.0 * np.array([0, 4.0, 0, 0])
    W[2, 0, 2] = 3.0 * np.array([1.0, 0, 0, -1.0])
    W[2, 2, 2] = 3.0 * np.array([0, 4.0, 0, 0])
    np.testing.assert_array_equal(op.dense(), W.reshape(9, 12))
    q = np.random.default_rng(0).normal(size=(2, 3, 5, 4))     # [nprof, npath, layers, nwn]
    want = np.einsum("vcji,pjli->pvlc", W, q)
    got, S = oc.reference(op, q)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
    assert np.all(S >= np.abs(got) - 1e-14) and np.all(S[:, 1] == 0) and np.all(S[:, :, :, 1] == 0)
    assert api.ObsOperator([0, 1], [1.0], [0, 0, 2], [1, 1, 1]).nchan == 3          # nchan defaults to max(chan) + 1


def test_the_cases_hold_what_they_promise():
    for views, chmap in oc.PAIRS + (("B", "nested"),):
        op = oc.operator(views, chmap, 70)
        assert tuple(np.diff(op.view_start)) == oc.VIEWS[views]
        assert np.any(op.wpath < 0) and np.any(op.wpath > 0)
    ch, w, nchan = oc.nested_map(70)
    members = [np.nonzero(ch == c)[0] for c in range(nchan)]
    assert members[0][0] < members[1][0] < members[2][0] < members[2][1] < members[1][1] < members[0][1]      # nested sidebands
    assert members[3].min() < 64 <= members[3].max() and len(members[4]) == 1 and len(members[5]) == 0
    assert np.any(ch == -1) and np.any(w[ch >= 0] < 0) and np.any(w[ch >= 0] > 0)
    ch, w, nchan = oc.comb_map(70)
    assert all(np.any(np.nonzero(ch == c)[0] < 64) and np.any(np.nonzero(ch == c)[0] >= 64) for c in range(4, 10))
    ident = oc.identity(5, 70)
    np.testing.assert_array_equal(ident.dense(), np.eye(350))


@pytest.mark.parametrize("bad", [
    dict(view_start=[0, 3, 2, 4]),                    # decreases
    dict(view_start=[1, 2, 4]),                       # does not start at 0
    dict(view_start=[0, 2, 3]),                       # does not end at npath
    dict(view_start=[0]),                             # no view
    dict(view_start=[[0, 4]]),                        # not 1-D
    dict(view_start=[0.0, 4.0]),                      # not integers
    dict(wpath=[]),                                   # no path
    dict(wpath=[1.0, np.nan, 1.0, 1.0]),
    dict(wpath=[1.0, np.inf, 1.0, 1.0]),
    dict(chan=[0, 1, 3]),                             # >= nchan
    dict(chan=[0, -2, 1]),
    dict(chan=[0, 1]),                                # length differs from wchan's
    dict(wchan=[1.0, -np.inf, 1.0]),
    dict(nchan=0),
    dict(nchan=api.OBS_MAX_CHAN + 1),
    dict(wpath=np.ones(api.OBS_MAX_PATHS + 1), view_start=[0, api.OBS_MAX_PATHS + 1]),
])
def test_validation(bad):
    good = dict(view_start=[0, 2, 4], wpath=[1.0, -1.0, 0.5, 0.5], chan=[0, -1, 2], wchan=[1.0, 2.0, -3.0], nchan=3)
    api.ObsOperator(**good)
    with pytest.raises(ValueError):
        api.ObsOperator(**dict(good, **bad))


def test_from_sets_permutation():
    """Views given as sets of the caller's path indices: the operator holds the paths of the views, view by view; perm[k] is the
    caller's index of the operator's path k.  Paths in no view (3 and 6 of 7 here) are not part of the operator: a NaN along one of
    them cannot reach a measurement, and the empty view stays empty."""
    op, perm = api.ObsOperator.from_sets(views=[[4, 1], [0, 5, 2], []], channels=[[3, 0], [2]], npath=7, nwn=5)
    np.testing.assert_array_equal(perm, [4, 1, 0, 5, 2])
    assert op.npath == 5
    np.testing.assert_array_equal(op.view_start, [0, 2, 5, 5])
    np.testing.assert_array_equal(op.wpath, [0.5, 0.5, 1 / 3, 1 / 3, 1 / 3])
    np.testing.assert_array_equal(op.chan, [0, -1, 1, 0, -1])
    np.testing.assert_array_equal(op.wchan, [0.5, 0, 1.0, 0.5, 0])
    q = np.random.default_rng(1).normal(size=(1, 7, 5))                       # in the caller's path order
    q[0, 3] = np.nan
    q[0, 6] = np.inf
    got, S = oc.reference(op, q[:, perm])
    want = np.zeros((1, 3, 2))
    want[0, 0] = [q[0, [4, 1]][:, [3, 0]].mean(), q[0, [4, 1], 2].mean()]
    want[0, 1] = [q[0, [0, 5, 2]][:, [3, 0]].mean(), q[0, [0, 5, 2], 2].mean()]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    assert np.all(S[0, 2] == 0)
    for kw in (dict(views=[[0, 0]], channels=[[0]]), dict(views=[[0], [0]], channels=[[0]]), dict(views=[[0]], channels=[[1], [1]]),
               dict(views=[[3]], channels=[[0]], npath=3), dict(views=[[0]], channels=[[-1]]), dict(views=[], channels=[[0]]),
               dict(views=[[], []], channels=[[0]])):
        with pytest.raises(ValueError):
            api.ObsOperator.from_sets(**kw)
