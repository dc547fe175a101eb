"""Measurement operators of tests/test_obs_cpu.py and tests/test_obs_jacobian.py (monortm_hip_obs_create), and
the float64 reference of a contracted field.

Views (rtm_obs_jac_kernel walks a view's paths in tiles of 4):
  A   9 paths in views of 4 / 1 / 4       one full tile, a one-path tile, one full tile
  B  13 paths in views of 5 / 0 / 8       a full and a short tile, an EMPTY view, two full tiles
  C  21 paths in one view                 five full tiles and a one-path tile
Channel maps on nwn wavenumbers (blocks of 64: with nwn = 70 one full block and one of 6 live lanes):
  nested  7 channels: 0, 1, 2 nested sidebands around one centre (0 outermost), 3 with members in both wavenumber blocks (nwn > 64), 4 a
          single sample (the last wavenumber), 5 EMPTY, 6 a run of eleven; every other sample is -1; weights of mixed sign
  comb    10 channels, chan[i] = i mod 10: every sample used, every channel interleaved with all others (with nwn = 70 channels 4 .. 9 have
          members in both blocks); positive weights that sum to 1 per channel"""
import numpy as np

from monortm_amd import api

VIEWS = {"A": (4, 1, 4), "B": (5, 0, 8), "C": (21,)}
PAIRS = (("A", "nested"), ("B", "comb"), ("C", "nested"))   # (views, channel map) of the parametrised tests


def factors(npath, seed=3):
    """Path factors in [0.7, 12): the range of FACTORS9 of tests/test_scan.py."""
    return np.random.default_rng(seed).uniform(0.7, 12.0, npath)


def view_arrays(name, mixed=True):
    sizes = VIEWS[name]
    vs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rng = np.random.default_rng(100 + len(sizes) + int(vs[-1]))
    w = rng.normal(0.0, 1.0, int(vs[-1])) if mixed else np.concatenate([np.full(n, 1.0 / n) for n in sizes if n])
    return vs, w


def nested_map(nwn):
    assert nwn >= 30
    ch = np.full(nwn, -1, np.int32)
    c = nwn // 4
    for k, d in enumerate((3, 2, 1)):
        ch[[c - d, c + d]] = k
    straddle = [60, 61, 63, 64, 66] if nwn > 66 else [nwn - 9, nwn - 8, nwn - 6, nwn - 5, nwn - 3]
    ch[straddle] = 3
    ch[nwn - 1] = 4
    run = [0, 1, 2] + list(range(nwn // 2, nwn // 2 + 8))
    assert np.all(ch[run] == -1)
    ch[run] = 6
    w = np.random.default_rng(7).normal(0.0, 1.0, nwn)
    return ch, w, 7


def comb_map(nwn):
    ch = (np.arange(nwn) % 10).astype(np.int32)
    w = np.random.default_rng(8).uniform(0.5, 1.5, nwn)
    for c in range(10):
        w[ch == c] /= w[ch == c].sum()
    return ch, w, 10


def operator(views, chmap, nwn, mixed=True):
    vs, wp = view_arrays(views, mixed)
    ch, wc, nchan = {"nested": nested_map, "comb": comb_map}[chmap](nwn)
    return api.ObsOperator(vs, wp, ch, wc, nchan=nchan)


def identity(npath, nwn):
    return api.ObsOperator(np.arange(npath + 1), np.ones(npath), np.arange(nwn), np.ones(nwn))


def contract(W, k, nview, nchan):
    """k [nprof, npath, ..., nwn] (float64) contracted with the dense weights W [nview * nchan, npath * nwn] -> [nprof, nview, ..., nchan]."""
    k = np.moveaxis(np.asarray(k, np.float64), 1, -2)
    out = k.reshape(k.shape[:-2] + (-1,)) @ W.T
    return np.moveaxis(out.reshape(out.shape[:-1] + (nview, nchan)), -2, 1)


def reference(op, k):
    """(the contracted field, S = sum |wpath_j wchan_i term_ji| of every element)."""
    W = op.dense()
    return contract(W, k, op.nview, op.nchan), contract(np.abs(W), np.abs(np.asarray(k, np.float64)), op.nview, op.nchan)
