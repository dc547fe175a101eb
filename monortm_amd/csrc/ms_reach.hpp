// ms_reach.hpp - the slots of lines_ms_kernel a table line can reach: the per-line rule of ms_reach_kernel (lines_ms_kernel.hip) as
// one host / device function, so that a host program can be held to it bit for bit (tests/native/ms_reach_check.cpp,
// tests/test_ms_reach_cpu.py: the Python mirror, the soundness of the margin).  DESIGN.md section 3.1m.
//
// Slot k of a wave = the k-th wavenumbers of its lanes = channels k LPS .. k LPS + LPS - 1 of every state.  Bit k of the word: the line
// can come within 25 cm-1 of some channel of slot k; bit 8 + k: its NEGATIVE resonance can (WN + Xnu <= 25 for the slot's lowest
// channel, modm.f90:713 / :757) - with the shifted centre Xnu anywhere within `pad` of the table's x.  `every` (a coupled O2 line: no
// rule, modm.f90:755-792; a NaN centre) reaches every slot that holds a channel.  The comparisons are negated on purpose: a NaN in
// x, pad or a channel sets the bit.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MS_REACH_HD __host__ __device__
#else
#define MS_REACH_HD
#endif

namespace monortm_dev {

constexpr int MS_REACH_SLOTS = 5;       // = MS_WPS (lines_ms_asm.hpp): wavenumbers per lane
constexpr double MS_REACH_RHO = 2.0;    // densest state (RHORAT = density over that at 1013.25 hPa, 296 K) the slot masks allow for

// the margin for the pressure shift: |Xnu - XNU0| <= max_abs_shift x RHORAT (line_table.cpp)
MS_REACH_HD inline double ms_reach_pad(double max_abs_shift) { return max_abs_shift * MS_REACH_RHO + 1e-6; }

// wn: the ascending channels, nwn of them (at most 64 where lines_ms_kernel runs)
MS_REACH_HD inline unsigned ms_reach_word(const double *wn, int nwn, int LPS, double x, bool every, double pad) {
    unsigned r = 0u;
    for (int k = 0; k < MS_REACH_SLOTS; k++) {
        const int c0 = LPS * k;
        if (c0 >= nwn) break;
        const double wlo = wn[c0], whi = wn[(c0 + LPS < nwn ? c0 + LPS : nwn) - 1];
        if (every || (!(x - pad - 25. > whi) && !(wlo - 25. > x + pad))) r |= 1u << k;
        // bits 8 .. 12: the NEGATIVE resonance reaches the slot (WN + Xnu <= 25 for its lowest channel, modm.f90:713 / :757)
        if (every || !(wlo + (x - pad) > 25.)) r |= 256u << k;
    }
    return r;
}

}  // namespace monortm_dev
