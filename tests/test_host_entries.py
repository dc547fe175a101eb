"""Every host-buffer entry of the C ABI, sharded over three devices with ragged and empty blocks.

A multi-device context cuts a call into contiguous blocks of ceil(P/G) profiles and runs each block as a call of its own on one shard.
So what a three-shard context (MONORTM_DEVICES="0,0,0") returns for the profiles [p0, p0 + n) of a block must be, BIT FOR BIT, what a
one-device context returns when it is called on those n profiles alone - the full Jacobians included, because the shard then runs MODM
on the very batch shape of the single call.  nprof = 5 gives the blocks 2, 2, 1 and nprof = 4 the blocks 2, 2, 0.

The shapes are the smallest that keep every per-profile stride distinct (nlay_max = 6, nlay_max + 1 = 7, nwn = 5, npath = 3,
nview x nchan = 4, nmol = 7, njac = 1), so an array shifted by another array's stride cannot go unnoticed.  Every output is pre-filled
with FILL and carries one extra profile's worth of FILL at its end, which must survive; rows beyond nlay[p] are compared as they come
back.  The calls go straight through ctypes: a null optional argument reaches the C entry as null."""
import os

import numpy as np
import pytest

from monortm_amd import api, synth, tape3
from test_scan_jacobian import FILL, _p, err

pytestmark = pytest.mark.gpu

NLAY = [6, 4, 5, 6, 3]
LM, NWN, NPATH, NVIEW, NCHAN, NMOL = 6, 5, 3, 2, 2, 7
G = 3   # shards


def blocks(nprof):
    """shard_block of api.hip: (p0, n) of every shard that gets profiles."""
    per = -(-nprof // G)
    return [(g * per, min(nprof, (g + 1) * per) - g * per) for g in range(G) if g * per < nprof]


@pytest.fixture(scope="module")
def ctxs(workdir):
    """(one-device, three-shard) contexts per real_kind on a synthetic TAPE3, the measurement operator created on each, and the inputs."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    t3 = f"{workdir}/TAPE3_host_entries"
    tape3.write_tape3(t3, synth.synthetic_lines(150, seed=12, lc_frac=0.5, sdep_frac=0.1))
    wn = synth.c2_channels(NWN, seed=8)
    prs = [synth.perturbed_profile(700 + i, wn, nlay=NLAY[i], cloud=(i % 2 == 0), irt=(1, 3, 2)[i % 3]) for i in range(len(NLAY))]
    rng = np.random.default_rng(20)
    op = api.ObsOperator([0, 2, 3], rng.uniform(0.2, 1.0, NPATH), [0, 1, 0, -1, 1], rng.uniform(0.2, 1.0, NWN), nchan=NCHAN)
    assert (op.npath, op.nwn, op.nview, op.nchan) == (NPATH, NWN, NVIEW, NCHAN)
    made, old = {}, os.environ.get("MONORTM_DEVICES")
    os.environ["MONORTM_DEVICES"] = ",".join(["0"] * G)
    try:
        for rk in (8, 4):
            one = api.MonoRTM(t3, wn[0], wn[-1], real_kind=rk)
            multi = api.MonoRTM(t3, wn[0], wn[-1], real_kind=rk, ngpu=0)
            assert multi.lib.monortm_hip_device_count(multi.ctx) == G
            made[rk] = (one, multi, one.obs_create(op), multi.obs_create(op))
    finally:
        if old is None:
            del os.environ["MONORTM_DEVICES"]
        else:
            os.environ["MONORTM_DEVICES"] = old
    yield made, prs
    for one, multi, _, _ in made.values():
        one.close()
        multi.close()


def inputs(r, prs):
    """The arrays of all entries for the batch prs, in the context's REAL kind: name -> array with the profile axis first."""
    dt, n = r.dtype, len(prs)
    _, _, nlay, _, irt, _, _, ts, em, rf = r._pack_rtm(prs)
    rng = np.random.default_rng(21)

    def pack(get, width=None):   # zero padding up to LM, whatever the batch's own deepest profile
        return api.pack_layers(prs, LM, get, width, dt)

    a = dict(nlay=nlay, irt=irt, ts=ts, em=em, rf=rf, T=pack(lambda p: p.t), P=pack(lambda p: p.p), CLW=pack(lambda p: p.clw),
             WB=pack(lambda p: p.wbrodl), WKL=pack(lambda p: p.wkl, NMOL))
    a["TZ"] = np.zeros((n, LM + 1), dt)
    for i, p in enumerate(prs):
        a["TZ"][i, : p.nlay + 1] = p.tz
    a["O"] = np.clip(np.exp(rng.normal(np.log(7e-3), 1.6, (n, LM, NWN))), 1e-5, 5.0).astype(dt)
    a["path"] = rng.uniform(1.0, 3.0, (n, NPATH, LM)).astype(dt)
    a["em3"] = rng.uniform(0.6, 1.0, (n, NPATH, NWN)).astype(dt)
    a["rf3"] = (1.0 - a["em3"]).astype(dt)
    return a


# per-profile shapes of the outputs
V, W, WZ = (NWN,), (LM, NWN), (LM + 1, NWN)
PV, PW, PWZ = (NPATH, NWN), (NPATH, LM, NWN), (NPATH, LM + 1, NWN)
Y, YK, YKZ = (NVIEW, NCHAN), (NVIEW, LM, NCHAN), (NVIEW, LM + 1, NCHAN)


class Call:
    """One call of an entry on the profiles [p0, p0 + n) of the inputs: every output (and the in/out tmpsfc) is a fresh array of n + 1
    profiles filled with FILL; i(name) / o(name, shape) hand the pointers out, o(...) of a name in `drop` is null."""

    def __init__(self, r, a, p0, n, drop):
        self.r, self.a, self.p0, self.n, self.drop, self.out, self.keep = r, a, p0, n, drop, {}, []

    def i(self, name):
        x = np.ascontiguousarray(self.a[name][self.p0 : self.p0 + self.n])
        self.keep.append(x)
        return _p(x)

    def o(self, name, shape, dtype=None):
        if name in self.drop:
            return None
        self.out[name] = np.full((self.n + 1,) + shape, FILL, dtype or self.r.dtype)
        return _p(self.out[name])

    def fac(self, pr):
        self.keep.append(np.ascontiguousarray(pr.cntnm, np.float64))
        return _p(self.keep[-1])

    def io(self, name):
        p = self.o(name, ())
        self.out[name][: self.n] = self.a[name][self.p0 : self.p0 + self.n]
        return p


def modm(c, pr, wn, v):
    return c.r.lib.monortm_hip_modm_xs(c.r.ctx, c.n, NWN, _p(wn), pr.dvset, c.i("nlay"), LM, NMOL, c.i("P"), c.i("T"), c.i("CLW"), c.i("WKL"),
                                       c.i("WB"), c.fac(pr), pr.sclcpl, pr.sclhw, pr.y0res, pr.ibrd, 0, None, None, c.o("o", W),
                                       c.o("o_by_mol", (LM, NMOL, NWN)), c.o("oc", (LM, api.NCONT, NWN)), c.o("o_clw", W))


def rtm_outs(c, s):
    return [c.o(k, s) for k in ("rup", "rdn", "trtot", "rad", "tb", "tmr")]


def rtm(c, pr, wn, v):
    return c.r.lib.monortm_hip_rtm(c.r.ctx, c.n, NWN, _p(wn), c.i("nlay"), LM, c.i("irt"), v["iout"], c.i("T"), c.i("TZ"), c.i("O"), c.io("ts"),
                                   c.i("em"), c.i("rf"), *rtm_outs(c, V))


def sfc(c, v):
    return (c.i("em3"), c.i("rf3")) if v["sfc"] else (c.i("em"), c.i("rf"))


def rtm_scan(c, pr, wn, v):
    return c.r.lib.monortm_hip_rtm_scan(c.r.ctx, c.n, NPATH, NWN, _p(wn), c.i("nlay"), LM, c.i("irt"), v["iout"], c.i("T"), c.i("TZ"), c.i("O"),
                                        c.i("path"), c.io("ts"), v["sfc"], *sfc(c, v), *rtm_outs(c, PV))


def rtm_jac(c, pr, wn, v):
    return c.r.lib.monortm_hip_rtm_jac(c.r.ctx, c.n, NWN, _p(wn), c.i("nlay"), LM, c.i("irt"), 1, c.i("T"), c.i("TZ"), c.i("O"), c.i("ts"),
                                       c.i("em"), c.i("rf"), c.o("rad", V), c.o("tb", V), c.o("k_o", W), c.o("k_t", W), c.o("k_tz", WZ),
                                       c.o("k_sfc", (3, NWN)))


def modm_in(c, pr, wn):
    return (_p(wn), pr.dvset, c.i("nlay"), LM, NMOL, c.i("P"), c.i("T"), c.i("CLW"), c.i("WKL"), c.i("WB"), c.fac(pr), pr.sclcpl, pr.sclhw,
            pr.y0res, pr.ibrd, c.i("irt"), c.i("TZ"), c.i("ts"))


def mols(c, v):
    jm = np.array([1], np.int32)
    c.keep.append(jm)
    return (1, _p(jm)) if v["njac"] else (0, None)


def jacobian(c, pr, wn, v):
    return c.r.lib.monortm_hip_jacobian(c.r.ctx, c.n, NWN, *modm_in(c, pr, wn), c.i("em"), c.i("rf"), 1, *mols(c, v), c.o("o", W), c.o("rad", V),
                                        c.o("tb", V), c.o("k_t", W), c.o("k_tz", WZ), c.o("k_w", (LM, 1, NWN)), c.o("k_clw", W), c.o("k_o", W),
                                        c.o("k_sfc", (3, NWN)))


def rtm_scan_jac(c, pr, wn, v):
    return c.r.lib.monortm_hip_rtm_scan_jac(c.r.ctx, c.n, NPATH, NWN, _p(wn), c.i("nlay"), LM, c.i("irt"), 0, c.i("T"), c.i("TZ"), c.i("O"),
                                            c.i("path"), c.i("ts"), v["sfc"], *sfc(c, v), c.o("rad", PV), c.o("tb", PV), c.o("k_o", PW),
                                            c.o("k_path", PW), c.o("k_t", PW), c.o("k_tz", PWZ), c.o("k_sfc", (NPATH, 3, NWN)))


def scan_jacobian(c, pr, wn, v):
    return c.r.lib.monortm_hip_scan_jacobian(c.r.ctx, c.n, NWN, *modm_in(c, pr, wn), *sfc(c, v), 1, *mols(c, v), NPATH, c.i("path"), v["sfc"],
                                             c.o("o", W), c.o("rad", PV), c.o("tb", PV), c.o("k_t", PW), c.o("k_tz", PWZ),
                                             c.o("k_w", (NPATH, LM, 1, NWN)), c.o("k_clw", PW), c.o("k_o", PW), c.o("k_path", PW),
                                             c.o("k_sfc", (NPATH, 3, NWN)))


def rtm_obs_jac(c, pr, wn, v):
    return c.r.lib.monortm_hip_rtm_obs_jac(c.r.ctx, c.n, NPATH, NWN, _p(wn), c.i("nlay"), LM, c.i("irt"), 1, c.i("T"), c.i("TZ"), c.i("O"),
                                           c.i("path"), c.i("ts"), v["sfc"], *sfc(c, v), v["obs"], c.o("y", Y), c.o("k_t", YK), c.o("k_tz", YKZ),
                                           c.o("k_sfc", (NVIEW, 3, NCHAN)))


def obs_jacobian(c, pr, wn, v):
    return c.r.lib.monortm_hip_obs_jacobian(c.r.ctx, c.n, NWN, *modm_in(c, pr, wn), *sfc(c, v), 1, *mols(c, v), NPATH, c.i("path"), v["sfc"],
                                            v["obs"], c.o("o", W), c.o("y", Y), c.o("k_t", YK), c.o("k_tz", YKZ),
                                            c.o("k_w", (NVIEW, LM, 1, NCHAN)), c.o("k_clw", YK), c.o("k_sfc", (NVIEW, 3, NCHAN)))


def vcen(c, wn, v):
    """The channels' nominal wavenumbers of quantity 2 (shared by the profiles), null otherwise."""
    if v["q"] != 2:
        return None
    c.keep.append(np.ascontiguousarray(np.linspace(wn[0], wn[-1], NCHAN)))
    return _p(c.keep[-1])


def rtm_obs(c, pr, wn, v):
    return c.r.lib.monortm_hip_rtm_obs(c.r.ctx, c.n, NPATH, NWN, _p(wn), c.i("nlay"), LM, c.i("irt"), v["q"], c.i("T"), c.i("TZ"), c.i("O"),
                                       c.i("path"), c.i("ts"), v["sfc"], *sfc(c, v), v["obs"], vcen(c, wn, v), c.o("y", Y))


def obs(c, pr, wn, v):
    return c.r.lib.monortm_hip_obs(c.r.ctx, c.n, NWN, *modm_in(c, pr, wn), *sfc(c, v), v["q"], NPATH, c.i("path"), v["sfc"], v["obs"],
                                   vcen(c, wn, v), c.o("o", W), c.o("y", Y))


def case(entry, rk=8, drop=(), **v):
    v = dict(dict(sfc=0, iout=1, njac=1), **v)
    name = "-".join([entry.__name__, f"r{rk}"] + [f"{k}{x}" for k, x in v.items() if k in ("sfc", "iout", "njac", "q")] + ["no_" + k for k in drop])
    return pytest.param(entry, rk, tuple(drop), v, id=name)


NO_W = ("k_w", "k_o", "k_path")
CASES = [
    case(modm), case(modm, rk=4),
    case(rtm), case(rtm, iout=0, drop=("tmr",)), case(rtm, rk=4),
    case(rtm_scan), case(rtm_scan, sfc=1, iout=0, drop=("tmr",)), case(rtm_scan, rk=4, sfc=1),
    case(rtm_jac), case(rtm_jac, rk=4),
    case(jacobian), case(jacobian, njac=0, drop=NO_W),
    case(rtm_scan_jac), case(rtm_scan_jac, sfc=1, drop=("k_o", "k_path")), case(rtm_scan_jac, rk=4),
    case(scan_jacobian), case(scan_jacobian, sfc=1, njac=0, drop=NO_W),
    case(rtm_obs_jac), case(rtm_obs_jac, sfc=1), case(rtm_obs_jac, rk=4),
    case(obs_jacobian), case(obs_jacobian, sfc=1, njac=0, drop=("k_w",)),
    case(rtm_obs, q=1), case(rtm_obs, sfc=1, q=2), case(rtm_obs, rk=4, q=0), case(rtm_obs, rk=4, sfc=1, q=1),
    case(obs, q=1), case(obs, sfc=1, q=2), case(obs, rk=4, q=1),
]


def bits(x):
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("nprof", [5, 4])
@pytest.mark.parametrize("entry,rk,drop,v", CASES)
def test_sharded_block_equals_the_block_alone(ctxs, entry, rk, drop, v, nprof):
    made, prs = ctxs
    one, multi, h_one, h_multi = made[rk]
    prs = prs[:nprof]
    wn, a = np.ascontiguousarray(prs[0].wn), inputs(one, prs)
    whole = Call(multi, a, 0, nprof, drop)
    assert entry(whole, prs[0], wn, dict(v, obs=h_multi)) == 0, err(multi)
    assert sum(n for _, n in blocks(nprof)) == nprof
    for p0, n in blocks(nprof):
        alone = Call(one, a, p0, n, drop)
        assert entry(alone, prs[0], wn, dict(v, obs=h_one)) == 0, err(one)
        assert whole.out.keys() == alone.out.keys()
        for k, x in alone.out.items():
            assert np.array_equal(bits(whole.out[k][p0 : p0 + n]), bits(x[:n])), f"{k}, profiles {p0}..{p0 + n - 1}"
            assert np.all(x[n:] == FILL), f"{k}: the one-device call wrote beyond its {n} profiles"
    for k, x in whole.out.items():
        assert np.all(x[nprof:] == FILL), f"{k}: the sharded call wrote beyond its {nprof} profiles"
        if k == "tb" and v["iout"] != 1:
            assert np.all(x == FILL), "TB of a call with iout /= 1 must be left alone"
        else:
            assert np.all((x[:nprof] != FILL).reshape(nprof, -1).any(axis=1)), f"{k} was not written for every profile"
