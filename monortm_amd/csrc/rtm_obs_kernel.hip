// rtm_obs_kernel.hip - the forward measurement operator (monortm_hip_rtm_obs, monortm_hip_obs) for gfx950: Y per MEASUREMENT
// (view, channel), y = sum_{j in view} wpath_j sum_{i: chan_i = c} wchan_i q_ji, contracted inside the kernel that forms the
// monochromatic radiances along the paths - none of them reaches memory.  The forward half of rtm_obs_jac_kernel.hip: its layout, its
// owner threads, its order of additions, without the adjoint.  See DESIGN.md section 3.10.
#include "obs_exchange.hpp"
#include "rtm_tile.hpp"

namespace {
using namespace monortm_dev;

// the band brightness temperature of a contracted radiance at the channel's nominal wavenumber, formed as rtm_combine forms TB
__device__ __forceinline__ double band_tb(double vc, double rad) {
#pragma clang fp contract(off)
    const double c3 = K_RADCN1 * (vc * vc * vc);
    return K_RADCN2 * vc / log(c3 / rad + 1.);
}

// One workgroup = one (profile, view): 64 wavenumbers x G layer groups (a wave each).  It walks the view's paths in tiles of NP and, per
// tile, the wavenumber blocks of 64, serially (blocks no channel has a member in are skipped); per (tile, block) the forward sums of
// rtm_scan_kernel - the very functions of rtm_tile.hpp it calls (the preloads, the optical depths per path, the forward sweep) - then
// the group sums through LDS one path at a time in the reference's visiting order and rtm_combine.
// Where that kernel stores q of path j, group 0 adds wpath_j x q to a register sum over the tile's paths (j ascending), hands the sum to
// the channel's owner lane (to_channels: wavenumbers ascending) and the owner adds it to Y (tiles ascending, blocks ascending within a
// tile).  Every element of Y has ONE owner thread for the whole launch - group 0, lane = channel mod 64 - which zero-fills it first: no
// atomics, no order left to the hardware.  quantity 2: RAD is contracted and the owner converts its finished element in place.
// The layer groups of a profile follow from ITS nlay (2 below 24 layers, G from 24 on), not from the batch's nlay_max: a profile gives
// the same bits alone and inside any batch.
// R: element type of the REAL inputs; A: of Y (A = double with R = float: the host entry rounds once, at the end).
template <typename R, typename A, int G, int NP>
__global__ __launch_bounds__(64 * G) void rtm_obs_kernel(RtmObsArgs a) {
    __shared__ double sUp[G][64], sDn[G][64], sSlab[64], sMw[64], sW[NP];
    __shared__ int sMl[64];
    extern __shared__ __attribute__((aligned(16))) double sBeta[];  // [nlay_max] hc/kT of the layers, [nlay_max + 1] of the levels, [NP][nlay_max] factors
    const int lane = threadIdx.x, g = threadIdx.y;
    const int view = blockIdx.x, prof = blockIdx.y;
    const int nwn = a.nwn, lm = a.nlay_max, nchan = a.nchan;
    const int nlay = max(0, min(a.nlay[prof], lm)), irt = a.irt[prof];
    const size_t pw = (size_t)prof * lm * nwn;   // (profile, layer 0, wn 0) of the [nprof][nlay_max][nwn] array
    const R *T = rp<R>(a.T) + (size_t)prof * lm, *TZ = rp<R>(a.TZ) + (size_t)prof * (lm + 1);
    double *sBl = sBeta, *sBz = sBeta + lm, *sF = sBeta + 2 * lm + 1;
    const int Geff = (G > 2 && nlay < 24) ? 2 : G;
    const int chunk = (nlay + Geff - 1) / Geff;
    const int l0 = min(nlay, g * chunk), l1 = min(nlay, l0 + chunk);  // 0-based layer range [l0, l1); empty for g >= Geff

    A *Y = wp<A>(a.Y) + ((size_t)prof * a.nview + view) * nchan;
    if (g == 0)
        for (int c = lane; c < nchan; c += 64) Y[c] = (A)0;
    tile_load_beta<G>(T, TZ, nlay, sBl, sBz);
    const int js = a.view_start[view], je = a.view_start[view + 1];
    const int nblk = (nwn + 63) / 64;
    const bool up = irt != 3;
    const double TSKY = 2.75;
    const double tsfc_in = (double)rp<R>(a.tmpsfc)[prof];
    const double tmpsfc = (irt == 3 || irt == 2) ? TSKY : tsfc_in;  // RTMmono.f90:113-124 (not written back here)

    for (int j0 = js; j0 < je; j0 += NP) {   // tiles of the view's paths; every bound below is workgroup-uniform
        const int npl = min(NP, je - j0);
        __syncthreads();   // (every wave is done with the factors of the tile before)
        tile_load_factors<G>(rp<R>(a.path) + ((size_t)prof * a.npath + j0) * lm, npl, nlay, lm, sF, a.errflag);
        if (g == 0 && lane < NP) sW[lane] = lane < npl ? a.wpath[j0 + lane] : 0.;

        for (int b = 0; b < nblk; b++) {
            const int *ms = a.mstart + (size_t)b * (nchan + 1);
            const int mb = ms[0], mcnt = ms[nchan] - mb;
            if (mcnt == 0) continue;   // no sample of the block is in any channel
            __syncthreads();   // (group 0 is done with the members of the block before)
            if (g == 0 && lane < mcnt) {
                sMl[lane] = a.mlane[mb + lane];
                sMw[lane] = a.mw[mb + lane];
            }
            __syncthreads();
            const int iw0 = b * 64 + lane;
            const int iw = iw0 < nwn ? iw0 : nwn - 1;   // (lanes beyond the grid repeat its last point; no member list names them)
            const double VV = a.wn[iw];
            const R *O = rp<R>(a.O) + pw + iw;

            double above[NP], ODTOT[NP];
            tile_optical_depths(O, nwn, l0, l1, npl, lm, sF, sUp, above, ODTOT);
            const double c3 = K_RADCN1 * (VV * VV * VV);
            double RUP[NP], RDN[NP], no_tmr[1];
            tile_forward_sweep<false>(O, nwn, l0, l1, npl, lm, sBl, sBz, sF, c3, VV, up, above, ODTOT, RUP, RDN, no_tmr);
            // the group sums in the reference's visiting order, one path at a time: only group 0 goes on with them
#pragma unroll
            for (int j = 0; j < NP; j++)
                if (j < npl) {
                    sUp[g][lane] = RUP[j];
                    sDn[g][lane] = RDN[j];
                    __syncthreads();
                    if (g == 0) {
                        double u = 0., d = 0.;
                        for (int gg = 0; gg < G; gg++) u = u + sUp[gg][lane];
                        for (int gg = G - 1; gg >= 0; gg--) d = d + sDn[gg][lane];
                        RUP[j] = u;
                        RDN[j] = d;
                    }
                    __syncthreads();
                }
            if (g == 0) {   // (a whole wave: no workgroup barrier inside)
                // the surface and the cosmic background: the same for every path of the tile
                const double SURFRAD = bb_fn(VV, K_RADCN2 / tmpsfc), COSMOS = bb_fn(VV, K_RADCN2 / TSKY);
                double sq[1] = {0.};   // sum over the tile's paths of wpath x q
#pragma unroll
                for (int j = 0; j < NP; j++)
                    if (j < npl) {
                        const size_t os = a.sfc_per_path ? ((size_t)prof * a.npath + j0 + j) * nwn + iw : (size_t)prof * nwn + iw;
                        const double ESFC = (double)rp<R>(a.emiss)[os], RSFC = (double)rp<R>(a.reflc)[os];
                        double TRTOT, RAD, TB, TMR;
                        rtm_combine(irt, VV, RUP[j], RDN[j], 0., ODTOT[j], ESFC, RSFC, SURFRAD, COSMOS, a.quantity == 1, false, TRTOT, RAD, TB, TMR);
                        sq[0] = fma(sW[j], a.quantity == 1 ? TB : RAD, sq[0]);
                    }
                A *const dst[1] = {Y};
                to_channels<A, 1>(sSlab, sq, nchan, ms, mb, sMl, sMw, dst, lane);
            }
        }
    }
    // the band brightness temperature: the owner converts what it has summed (its own stores, in program order).  An element without a
    // sample - an empty view, a channel without a member - stays 0; a radiance that is not positive and finite has no temperature
    if (a.quantity == 2 && g == 0)
        for (int c = lane; c < nchan; c += 64) {
            const double vc = a.vcen[c];
            if (!(vc > 0. && vc < __builtin_inf())) atomicOr(a.errflag, ERRBIT_ARG);
            bool sampled = false;
            for (int b = 0; b < nblk && !sampled; b++) sampled = a.mstart[(size_t)b * (nchan + 1) + c + 1] > a.mstart[(size_t)b * (nchan + 1) + c];
            if (je > js && sampled) {
                const double y = (double)Y[c];
                Y[c] = (A)((y > 0. && y < __builtin_inf()) ? band_tb(vc, y) : __builtin_nan(""));
            }
        }
}

// paths per tile: that of rtm_obs_jac_kernel, so that the tiles - and with them the order of the additions - are the same
constexpr int OBS_NP = 4;

template <typename R, typename A>
void launch_t(const RtmObsArgs &a, hipStream_t s) {
    dim3 grid(a.nview, a.nprof);
    // the layer groups of rtm_obs_jac_kernel; inside a G = 8 launch a profile below 24 layers works with 2 of them
    const size_t lds = sizeof(double) * ((size_t)(2 * a.nlay_max + 1) + (size_t)OBS_NP * a.nlay_max);
    if (a.nlay_max >= 24) hipLaunchKernelGGL((rtm_obs_kernel<R, A, 8, OBS_NP>), grid, dim3(64, 8), lds, s, a);
    else hipLaunchKernelGGL((rtm_obs_kernel<R, A, 2, OBS_NP>), grid, dim3(64, 2), lds, s, a);
}

}  // namespace

namespace monortm_dev {
void launch_rtm_obs(const RtmObsArgs &a, int out_kind, hipStream_t s) {
    if (a.real_kind == 4 && out_kind == 8) launch_t<float, double>(a, s);
    else if (a.real_kind == 4) launch_t<float, float>(a, s);
    else launch_t<double, double>(a, s);
}
}  // namespace monortm_dev
