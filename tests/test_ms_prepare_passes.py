"""The prepare stage of lines_ms_kernel (monortm_amd/csrc/lines_ms_kernel.hip): a pass holds SPP = 64 // CL whole states, a lane
is (sub, l) = line l of the chunk for state t SPP + sub in pass t, and the line is resolved once per chunk.  Small shapes at which
that mapping can go wrong, the kernel forced with `lines_kernel = ms` and the chunk size set with `ms_items`; every profile against
the oracle (north_star's 1e-6) and against lines_kernel (1e-11: the two differ by the rounding of the shared reciprocals).

The layout the host chooses (modm_plan.hpp; `_layout` below mirrors it, tests/test_modm_plan_cpu.py holds the two together): G = min(12, 64 // LPS, nprof) states a wave with
LPS = ceil(nwn / 5); CL the largest of 64, 32, 21, 16, 12, 10, 9, 8 whose ceil(G / SPP) passes are within ms_items // 64; one pass
less while the wave's LDS exceeds 10080 bytes.  For the cases here (both line lists: five (molecule, isotopologue) slots):

  (nwn, nprof, ms_items)   G   CL  SPP  passes  LDS bytes
  (50, 7, 192)             6   32   2     3       9716    second group: one profile, five state slots without one
  (50, 4, 128)             4   32   2     2       6820
  (50, 4, 64)              4   16   4     1       4708    all four states in one pass
  (50, 6, 128)             6   21   3     2       8116    lane 63 idles; the rare-shape bits of a state start at 0, 21, 42
  (40, 8, 192)             8   16   4     2       8388    three passes would be CL 21 (CL 24 before): 10500 bytes with eight
                                                          states, so two passes of four states - the layout it had before
  (64, 5, 192)             4   32   2     2       6820    was CL 48 in three passes
  (1, 2, 192)              2   64   1     2       6036    one state a pass
"""
import numpy as np
import pytest

from common import RTOL, compare
from monortm_amd import api, synth, tape3

pytestmark = pytest.mark.gpu

NMOL = 7
CL_SET = (64, 32, 21, 16, 12, 10, 9, 8)
LDS_MAX = 10240 - 160
# (nwn, nprof, ms_items) -> (G, CL, passes, ms_items the LDS leaves)
CASES = {
    (50, 7, 192): (6, 32, 3, 192),
    (50, 4, 128): (4, 32, 2, 128),
    (50, 4, 64): (4, 16, 1, 64),
    (50, 6, 128): (6, 21, 2, 128),
    (40, 8, 192): (8, 16, 2, 128),
    (64, 5, 192): (4, 32, 2, 192),
    (1, 2, 192): (2, 64, 2, 192),
}
LISTS = {
    "coupled": dict(n=420, sdep_frac=0.15, lc_frac=0.4),   # non-plain chunks, rare-shape records
    "plain": dict(n=97),                                   # every chunk plain, a short last chunk
}


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need the MI355X")
    api.load_library()
    return True


def _layout(nwn, nprof, ms_items, nslot):
    """modm_plan.hpp's choice for lines_ms_kernel: (G, CL, passes, items budget taken, LDS bytes of the wave)."""
    lps = (nwn + 4) // 5
    g = min(12, 64 // lps, nprof)
    for items in range(ms_items, 63, -64):
        cl = next((c for c in CL_SET if -(-g // (64 // c)) <= items // 64), 0)
        if not cl:
            break
        spp = 64 // cl
        passes = -(-g // spp)
        stride = cl + 2
        while stride % 8 != 3:
            stride += 1
        lds = 32 * g * stride + 8 * (64 + g * 20 + g * NMOL + 2 * g * nslot) + 8 * (4 + 4 + 2 * 5 + 1) + 4 * (3 * NMOL + 2 + 64) + passes * 64 + 16
        if lds <= LDS_MAX:
            return g, cl, passes, items, lds
    return None


def _rt(t3, wn, kernel, ms_items):
    rt = api.MonoRTM(t3, wn[0], wn[-1])
    rt.set_option("lines_kernel", kernel)
    rt.set_option("ms_items", ms_items)
    return rt


def _close(a, b, what, tol=1e-11):
    for f in ("o", "o_by_mol", "rad", "tb", "tmr", "trtot", "rup", "rdn"):
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        scale = np.maximum(np.abs(y), 1e-9 * np.abs(y).max() if y.size else 1.0)
        if f == "o_by_mol":
            scale = np.maximum(np.abs(y), 1e-9 * np.abs(np.asarray(b.o))[:, None, :])
        err = float(np.max(np.abs(x - y) / np.maximum(scale, 1e-300))) if x.size else 0.0
        assert err <= tol, f"{what}: {f} differs by {err:.2e} between lines_kernel and lines_ms_kernel"


def test_layouts_of_the_cases():
    """The table of the module docstring is what the host rule gives, and only (40, 8, 192) has its item count lowered by the LDS."""
    for (nwn, nprof, ms_items), (g, cl, passes, items) in CASES.items():
        got = _layout(nwn, nprof, ms_items, nslot=5)
        assert got is not None and got[:4] == (g, cl, passes, items), f"{(nwn, nprof, ms_items)}: {got}"
        assert got[4] <= LDS_MAX


@pytest.mark.parametrize("which", list(LISTS))
@pytest.mark.parametrize("nwn,nprof,ms_items", list(CASES))
def test_ms_prepare_passes(workdir, gpu, nwn, nprof, ms_items, which):
    from oracle.pyoracle import Oracle

    kw = LISTS[which]
    rec = synth.synthetic_lines(seed=900 + nwn, **kw)
    phys = np.asarray(rec.iflg) >= 0
    assert len(set(int(m) % 100 for m in np.asarray(rec.mol)[phys])) == 5   # the slots _layout's table was computed for
    t3 = f"{workdir}/TAPE3_msp_{which}_{nwn}_{nprof}_{ms_items}"
    tape3.write_tape3(t3, rec)
    wn = synth.c2_channels(nwn, seed=nwn)
    lays = [64, 40, 17, 64, 33, 5, 64, 64, 12, 50, 64, 3, 64]
    profs = [synth.perturbed_profile(300 + i, wn, nlay=lays[i % len(lays)], cloud=(i % 2 == 0), irt=(1 if i % 3 == 0 else 3)) for i in range(nprof)]
    profs[1].wkl[:, 2] = 0.0   # no O3 in one state of a wave that walks its lines for the others
    out = {}
    for k in ("wn", "ms"):
        rt = _rt(t3, wn, k, ms_items)
        out[k] = rt.run(profs)
        rt.close()
    a, b = out["wn"], out["ms"]
    # (the forced kernel did run: its sums differ from lines_kernel's in the last bits)
    assert not all(np.array_equal(x.o_by_mol, y.o_by_mol) for x, y in zip(a, b))
    assert not b[1].o_by_mol[:, 2, :].any() and b[0].o_by_mol[:, 2, :].any()
    orc = Oracle(t3, wn[0], wn[-1])
    for i, pr in enumerate(profs):
        _close(b[i], a[i], f"{which} nwn={nwn} nprof={nprof} ms_items={ms_items} profile {i}")
        compare(b[i], orc.run(pr), rtol=RTOL, what=f"ms vs oracle {which} nwn={nwn} nprof={nprof} ms_items={ms_items} [{i}]")
    orc.close()
