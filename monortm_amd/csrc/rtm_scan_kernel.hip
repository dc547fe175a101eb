// rtm_scan_kernel.hip - CALCTMR + RAD_UP_DN + RTM (reference src/RTMmono.f90) along several paths through one atmosphere, from ONE
// set of optical depths, for gfx950.  See DESIGN.md section 3.7.
#include "rtm_tile.hpp"

namespace {
using namespace monortm_dev;

// The layout of rtm_kernel (block = 64 wavenumbers x G layer groups of a profile, every thread walks its group of layers once from
// the top down, group sums combined through LDS in the reference's visiting order) with NP paths per thread; blockIdx.z = tile of
// NP paths, the last tile may hold fewer (npl; a workgroup-uniform count, so the guards below are scalar branches).
//   per layer, once for the tile: (double)O, B(T_layer), B at the lower level;
//   per path: tau = (double)O * factor rounded ONCE (__dmul_rn: no contraction into the sums that follow), which is the value a
//   caller's pre-scaled O holds in double, then exactly the terms of rtm_kernel.
// hc / kT of the layers and levels and the tile's factors are formed once per workgroup (LDS); factors of layers >= nlay[p] are
// never read.  The LDS pieces of the group sums hold one path at a time: 24 KB at G = 16 whatever NP is.
// The preloads, the optical depths per path and the forward sweep are rtm_tile.hpp's (shared with rtm_obs_kernel and the two adjoint
// kernels); this file keeps the group-0 sums with CALCTMR's, the rtm_combine epilogue and the stores.
template <typename R, int G, int NP>
__global__ __launch_bounds__(64 * G) void rtm_scan_kernel(RtmScanArgs a) {
    __shared__ double sUp[G][64], sDn[G][64], sEx[G][64];
    extern __shared__ __attribute__((aligned(16))) double sBeta[];  // [nlay_max] hc/kT of the layers, [nlay_max + 1] of the levels, [NP][nlay_max] factors
    const int lane = threadIdx.x, g = threadIdx.y;
    const int iw0 = blockIdx.x * 64 + lane, prof = blockIdx.y;
    const int j0 = blockIdx.z * NP, npl = min(NP, a.npath - j0);
    const int nwn = a.nwn, lm = a.nlay_max;
    const bool valid = iw0 < nwn;
    const int iw = valid ? iw0 : nwn - 1;
    const int nlay = max(0, min(a.nlay[prof], lm)), irt = a.irt[prof];  // out-of-range counts are flagged by lines_kernel / the host
    const double VV = a.wn[iw];
    const R *O = rp<R>(a.O) + (size_t)prof * lm * nwn + iw;
    const R *T = rp<R>(a.T) + (size_t)prof * lm, *TZ = rp<R>(a.TZ) + (size_t)prof * (lm + 1);
    const R *F = rp<R>(a.path) + ((size_t)prof * a.npath + j0) * lm;
    double *sBl = sBeta, *sBz = sBeta + lm, *sF = sBeta + 2 * lm + 1;
    tile_load_beta<G>(T, TZ, nlay, sBl, sBz);
    tile_load_factors<G>(F, npl, nlay, lm, sF, a.errflag);
    __syncthreads();
    const int chunk = (nlay + G - 1) / G;
    const int l0 = min(nlay, g * chunk), l1 = min(nlay, l0 + chunk);  // 0-based layer range [l0, l1)

    double above[NP], ODTOT[NP];
    tile_optical_depths(O, nwn, l0, l1, npl, lm, sF, sUp, above, ODTOT);
    const double c3 = K_RADCN1 * (VV * VV * VV);
    const bool up = irt != 3;
    double RUP[NP], RDN[NP], sumexp[NP];
    tile_forward_sweep<true>(O, nwn, l0, l1, npl, lm, sBl, sBz, sF, c3, VV, up, above, ODTOT, RUP, RDN, sumexp);
    // the group sums in the reference's visiting order, one path at a time: only group 0 goes on with them
#pragma unroll
    for (int j = 0; j < NP; j++)
        if (j < npl) {
            sUp[g][lane] = RUP[j];
            sDn[g][lane] = RDN[j];
            sEx[g][lane] = sumexp[j];
            __syncthreads();
            if (g == 0) {
                double u = 0., d = 0., e = 0.;
                for (int gg = 0; gg < G; gg++) u = u + sUp[gg][lane];
                for (int gg = G - 1; gg >= 0; gg--) {
                    d = d + sDn[gg][lane];
                    e = e + sEx[gg][lane];
                }
                RUP[j] = u;
                RDN[j] = d;
                sumexp[j] = e;
            }
            __syncthreads();
        }
    if (g != 0 || !valid) return;
    const double TSKY = 2.75;
    double tmpsfc = (double)wp<R>(a.tmpsfc)[prof];
    if (irt == 3 || irt == 2) tmpsfc = TSKY;  // RTMmono.f90:113-124
    const double SURFRAD = bb_fn(VV, K_RADCN2 / tmpsfc), COSMOS = bb_fn(VV, K_RADCN2 / TSKY);
    // TMPSFC is in/out as in rtm_kernel: lanes that still read the old value ignore it exactly when it is overwritten (irt = 2,3)
    if (iw == 0 && blockIdx.z == 0 && (irt == 3 || irt == 2)) wp<R>(a.tmpsfc)[prof] = (R)TSKY;
#pragma unroll
    for (int j = 0; j < NP; j++)
        if (j < npl) {
            const size_t o = ((size_t)prof * a.npath + j0 + j) * nwn + iw;
            const size_t os = a.sfc_per_path ? o : (size_t)prof * nwn + iw;
            const double ESFC = (double)rp<R>(a.emiss)[os], RSFC = (double)rp<R>(a.reflc)[os];
            double TRTOT, RAD, TB, TMR;
            rtm_combine(irt, VV, RUP[j], RDN[j], sumexp[j], ODTOT[j], ESFC, RSFC, SURFRAD, COSMOS, a.iout == 1, a.TMR != nullptr, TRTOT, RAD,
                        TB, TMR);
            if (a.TMR) wp<R>(a.TMR)[o] = (R)TMR;
            wp<R>(a.RUP)[o] = (R)RUP[j];
            wp<R>(a.RDN)[o] = (R)RDN[j];
            wp<R>(a.TRTOT)[o] = (R)TRTOT;
            wp<R>(a.RAD)[o] = (R)RAD;
            if (a.iout == 1) wp<R>(a.TB)[o] = (R)TB;
        }
}

constexpr int SCAN_NP = 4;  // paths per thread: 8 running doubles per path -> 64 of the 128 VGPRs a 1024-thread workgroup may use

template <typename R>
void launch_r(const RtmScanArgs &a, hipStream_t s) {
    dim3 grid((a.nwn + 63) / 64, a.nprof, (a.npath + SCAN_NP - 1) / SCAN_NP);
    // the rule of launch_rtm with the path tiles counted: few workgroups and many layers -> 16 layer groups
    const bool few = (long long)grid.x * grid.y * grid.z < 256 && a.nlay_max >= 48;
    const size_t lds = sizeof(double) * ((size_t)(2 * a.nlay_max + 1) + (size_t)SCAN_NP * a.nlay_max);
    if (few) hipLaunchKernelGGL((rtm_scan_kernel<R, 16, SCAN_NP>), grid, dim3(64, 16), lds, s, a);
    else if (a.nlay_max >= 24) hipLaunchKernelGGL((rtm_scan_kernel<R, 8, SCAN_NP>), grid, dim3(64, 8), lds, s, a);
    else hipLaunchKernelGGL((rtm_scan_kernel<R, 2, SCAN_NP>), grid, dim3(64, 2), lds, s, a);
}

}  // namespace

namespace monortm_dev {
void launch_rtm_scan(const RtmScanArgs &a, hipStream_t s) {
    if (a.real_kind == 4) launch_r<float>(a, s);
    else launch_r<double>(a, s);
}
}  // namespace monortm_dev
