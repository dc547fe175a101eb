// rtm_obs_jac_kernel.hip - channel- and beam-averaged Jacobians of path scans (monortm_hip_rtm_obs_jac, monortm_hip_obs_jacobian) for
// gfx950: K per MEASUREMENT (view, channel), y = sum_{j in view} wpath_j sum_{i: chan_i = c} wchan_i q_ji, contracted inside the kernel
// that forms the monochromatic per-path terms - none of them reaches memory.  See DESIGN.md section 3.9.
#include "cloud_tkc.hpp"
#include "obs_exchange.hpp"   // OBS_SLAB, wave_fence, to_channels: shared with rtm_obs_kernel.hip
#include "rtm_tile.hpp"       // the tile sweep and the adjoint's per-path and per-(layer, path) arithmetic: shared with the scan kernels

namespace {
using namespace monortm_dev;

// One workgroup = one (profile, view): 64 wavenumbers x G layer groups (a wave each).  It walks the view's paths in tiles of NP and, per
// tile, the wavenumber blocks of 64, serially; per (tile, block) the two passes of rtm_scan_jac_kernel - the very functions of
// rtm_tile.hpp it calls (the preloads, the optical depths per path, the forward sweep, jac_path_weights, jac_layer_terms) - and around
// them its operations in its order (planck_d, odclw_tkc, tau = (double)O * factor rounded ONCE, the difference quotients of Opert).
// Where that kernel stores a term of path j, this one adds wpath_j x term to a register sum over the tile's paths (j ascending), hands
// the sum to the channel's owner lane (to_channels: wavenumbers ascending) and adds it to the output (tiles ascending, blocks ascending
// within a tile).  Every output element has ONE owner thread for the whole launch - the group that walks layer k (level k + 1; level 0,
// Y and K_SFC: group 0), lane = channel mod 64 - which zero-fills it first: no atomics, no order left to the hardware.
// The layer groups of a profile follow from ITS nlay (2 below 24 layers, G from 24 on: launch_rtm_jac_t's rule), not from the batch's
// nlay_max: a profile gives the same bits alone and inside any batch.
// R: element type of the REAL inputs; A: of the outputs (A = double with R = float: the host entry rounds once, at the end).
template <typename R, typename A, int G, int NP, bool FULL>
__global__ __launch_bounds__(64 * G) void rtm_obs_jac_kernel(RtmObsJacArgs a) {
    __shared__ double sUp[G][64], sDn[G][64], sSlab[G][OBS_SLAB * 64], sMw[64], sW[NP];
    __shared__ int sMl[64];
    extern __shared__ __attribute__((aligned(16))) double sBeta[];  // [nlay_max] hc/kT of the layers, [nlay_max + 1] of the levels, [NP][nlay_max] factors
    const int lane = threadIdx.x, g = threadIdx.y;
    const int view = blockIdx.x, prof = blockIdx.y;
    const int nwn = a.nwn, lm = a.nlay_max, nchan = a.nchan, njac = FULL ? a.njac : 0;
    const int nlay = max(0, min(a.nlay[prof], lm)), irt = a.irt[prof];
    const size_t pw = (size_t)prof * lm * nwn;   // (profile, layer 0, wn 0) of the [nprof][nlay_max][nwn] arrays
    const R *T = rp<R>(a.T) + (size_t)prof * lm, *TZ = rp<R>(a.TZ) + (size_t)prof * (lm + 1);
    double *sBl = sBeta, *sBz = sBeta + lm, *sF = sBeta + 2 * lm + 1;
    double *slab = sSlab[g];
    const int Geff = (G > 2 && nlay < 24) ? 2 : G;
    const int chunk = (nlay + Geff - 1) / Geff;
    const int l0 = min(nlay, g * chunk), l1 = min(nlay, l0 + chunk);  // 0-based layer range [l0, l1); empty for g >= Geff

    const size_t pv = (size_t)prof * a.nview + view;
    A *Y = wp<A>(a.Y) + pv * nchan, *KS = wp<A>(a.K_SFC) + pv * 3 * nchan;
    A *KT = wp<A>(a.K_T) + pv * lm * nchan, *KTZ = wp<A>(a.K_TZ) + pv * (lm + 1) * nchan;
    A *KW = FULL && njac ? wp<A>(a.K_W) + pv * lm * njac * nchan : nullptr;
    A *KC = FULL ? wp<A>(a.K_CLW) + pv * lm * nchan : nullptr;
    // every owner zero-fills its elements (and the padding: layers >= nlay, levels > nlay, which nothing is added to)
    for (int c = lane; c < nchan; c += 64) {
        for (int k = l0; k < l1; k++) {
            KT[(size_t)k * nchan + c] = (A)0;
            KTZ[(size_t)(k + 1) * nchan + c] = (A)0;
            if constexpr (FULL) {
                KC[(size_t)k * nchan + c] = (A)0;
                for (int i = 0; i < njac; i++) KW[((size_t)k * njac + i) * nchan + c] = (A)0;
            }
        }
        for (int k = nlay + g; k < lm; k += G) {
            KT[(size_t)k * nchan + c] = (A)0;
            KTZ[(size_t)(k + 1) * nchan + c] = (A)0;
            if constexpr (FULL) {
                KC[(size_t)k * nchan + c] = (A)0;
                for (int i = 0; i < njac; i++) KW[((size_t)k * njac + i) * nchan + c] = (A)0;
            }
        }
        if (g == 0) {
            KTZ[c] = (A)0;
            Y[c] = (A)0;
            KS[c] = (A)0;
            KS[nchan + c] = (A)0;
            KS[2 * (size_t)nchan + c] = (A)0;
        }
    }
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
            __syncthreads();   // (every wave is done with the members of the block before)
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

            // ---- pass 1: the group's forward sums (rtm_tile.hpp)
            double RUPg[NP], RDNg[NP], no_tmr[1];
            tile_forward_sweep<false>(O, nwn, l0, l1, npl, lm, sBl, sBz, sF, c3, VV, up, above, ODTOT, RUPg, RDNg, no_tmr);
            // the surface and the cosmic background: the same for every path of the tile
            const double ex_s = exp(VV * (K_RADCN2 / tmpsfc)), ex_c = exp(VV * (K_RADCN2 / TSKY));
            const double SURFRAD = c3 / (ex_s - 1.), COSMOS = c3 / (ex_c - 1.);
            // totals in the reference's visiting order (every group needs them) and the sums of the other groups, one path at a time;
            // then q, K_SFC and the weights of the path
            double gU[NP], gD[NP], gT[NP], upLow0[NP], dnHigh0[NP];
            double sq[4] = {0., 0., 0., 0.};   // sums over the tile's paths of wpath x (q, dq/dTMPSFC, dq/dEMISS, dq/dREFLC)
#pragma unroll
            for (int j = 0; j < NP; j++) {
                gU[j] = 0.;
                gD[j] = 0.;
                gT[j] = 0.;
                upLow0[j] = 0.;
                dnHigh0[j] = 0.;
                if (j < npl) {
                    sUp[g][lane] = RUPg[j];
                    sDn[g][lane] = RDNg[j];
                    __syncthreads();
                    double RUP = 0., RDN = 0., upLow = 0., dnHigh = 0.;
                    for (int gg = 0; gg < G; gg++) {
                        RUP = RUP + sUp[gg][lane];
                        if (gg < g) upLow = upLow + sUp[gg][lane];
                    }
                    for (int gg = G - 1; gg >= 0; gg--) {
                        RDN = RDN + sDn[gg][lane];
                        if (gg > g) dnHigh = dnHigh + sDn[gg][lane];
                    }
                    __syncthreads();
                    const double TRTOT = exp(-ODTOT[j]);
                    const size_t os = a.sfc_per_path ? ((size_t)prof * a.npath + j0 + j) * nwn + iw : (size_t)prof * nwn + iw;
                    const double ESFC = (double)rp<R>(a.emiss)[os], RSFC = (double)rp<R>(a.reflc)[os];
                    double RAD, lx, dq;
                    jac_path_weights(irt, TRTOT, RUP, RDN, ESFC, RSFC, SURFRAD, COSMOS, c3, VV, a.quantity, RAD, lx, dq, gU[j], gD[j], gT[j]);
                    const double wj = sW[j];
                    sq[0] = fma(wj, a.quantity == 1 ? K_RADCN2 * VV / lx : RAD, sq[0]);
                    if (irt == 1) {   // (0 otherwise)
                        double ksfc[3];
                        jac_path_sfc(irt, dq, TRTOT, RDN, ESFC, SURFRAD, COSMOS, VV, ex_s, tmpsfc, ksfc);
#pragma unroll
                        for (int i = 0; i < 3; i++) sq[1 + i] = fma(wj, ksfc[i], sq[1 + i]);
                    }
                    upLow0[j] = upLow;              // sum of up_l, l < the group's bottom layer
                    dnHigh0[j] = dnHigh;            // sum of dn_l, l > the group's top layer
                }
            }
            if (g == 0) {
                A *const dst[4] = {Y, KS, KS + nchan, KS + 2 * (size_t)nchan};
                to_channels<A, 4>(slab, sq, nchan, ms, mb, sMl, sMw, dst, lane);
            }

            // ---- pass 2: per-layer derivatives, layers l1-1 .. l0 (0-based), top-down (no workgroup barrier below: a wave's trip count is its own)
            if (l1 > l0) {
                double ODTd[NP], ODTu[NP], upIncl[NP], dnAbove[NP], dn_lev[NP];
#pragma unroll
                for (int j = 0; j < NP; j++) {
                    ODTd[j] = ODTOT[j] - above[j];
                    ODTu[j] = above[j];
                    upIncl[j] = 0.;
                    dnAbove[j] = dnHigh0[j];
                    dn_lev[j] = 0.;
                }
                // the sums of up_l, l <= the group's top layer, from pass 2's own terms, error-free (jac_up_sum, rtm_tile.hpp)
                double upLo[NP];
                {
                    double ODTu2[NP];
#pragma unroll
                    for (int j = 0; j < NP; j++) {
                        ODTu2[j] = above[j];
                        upIncl[j] = 0.;
                        upLo[j] = 0.;
                    }
                    if (up) {
                        double B2, dB2, Bzu2, dBzu2;
                        planck_d(c3, VV, sBz[l1], &Bzu2, &dBzu2);
                        for (int k = l1 - 1; k >= l0; k--) {
                            const double o2 = (double)O[(size_t)k * nwn];
                            planck_d(c3, VV, sBl[k], &B2, &dB2);
#pragma unroll
                            for (int j = 0; j < NP; j++)
                                if (j < npl) jac_up_sum(__dmul_rn(o2, sF[j * lm + k]), B2, Bzu2, up, ODTu2[j], upIncl[j], upLo[j]);
                            planck_d(c3, VV, sBz[k], &Bzu2, &dBzu2);
                        }
#pragma unroll
                        for (int j = 0; j < NP; j++) {
                            double s2, e2;
                            two_sum(upIncl[j], upLow0[j], s2, e2);
                            upIncl[j] = s2;
                            upLo[j] = upLo[j] + e2;
                        }
                    }
                }
                // B and dB/dT at the upper level of the group's top layer, and the downward sweep's term of level l1 from the layer above
                // (its lower level); level nlay (top of the atmosphere) is the lower level of no layer
                double Bzu, dBzu;
                planck_d(c3, VV, sBz[l1], &Bzu, &dBzu);
                if (l1 < nlay) {
                    const double o1 = (double)O[(size_t)l1 * nwn];
#pragma unroll
                    for (int j = 0; j < NP; j++)
                        if (j < npl) dn_lev[j] = jac_dn_lev_above(__dmul_rn(o1, sF[j * lm + l1]), gD[j], ODTd[j], dBzu);
                }
                for (int k = l1 - 1; k >= l0; k--) {
                    const double o = (double)O[(size_t)k * nwn];
                    double B, dB, Bzl, dBzl;
                    planck_d(c3, VV, sBl[k], &B, &dB);
                    planck_d(c3, VV, sBz[k], &Bzl, &dBzl);
                    double dOdT = 0., clw1 = 0.;
                    if constexpr (FULL) {
                        const size_t st = a.state_stride, ok = pw + (size_t)k * nwn + iw;
                        const R *Op = rp<R>(a.Opert);
                        dOdT = ((double)Op[ok] - (double)Op[st + ok]) * (0.5 / a.dt);
                        clw1 = odclw_tkc(VV, (double)T[k], 1.0);
                    }
                    double kof[NP];   // factor x dq/dtau of the layer, per path
                    double sk[3] = {0., 0., 0.};   // sums over the tile's paths of wpath x (K_T, K_TZ of level k + 1, K_CLW)
#pragma unroll
                    for (int j = 0; j < NP; j++) {
                        kof[j] = 0.;
                        if (j < npl) {
                            const double f = sF[j * lm + k];
                            double ko, kt, ktz;
                            jac_layer_terms(__dmul_rn(o, f), B, dB, Bzl, dBzl, Bzu, dBzu, up, gU[j], gD[j], gT[j], ODTd[j], ODTu[j], upIncl[j], upLo[j],
                                            dnAbove[j], dn_lev[j], ko, kt, ktz);   // (rtm_tile.hpp)
                            const double wj = sW[j];
                            sk[1] = fma(wj, ktz, sk[1]);
                            kof[j] = __dmul_rn(f, ko);
                            if constexpr (FULL) {
                                kt += kof[j] * dOdT;
                                sk[2] = fma(wj, kof[j] * clw1, sk[2]);
                            }
                            sk[0] = fma(wj, kt, sk[0]);
                        }
                    }
                    if constexpr (FULL) {
                        A *const dst[3] = {KT + (size_t)k * nchan, KTZ + (size_t)(k + 1) * nchan, KC + (size_t)k * nchan};
                        to_channels<A, 3>(slab, sk, nchan, ms, mb, sMl, sMw, dst, lane);
                        const size_t st = a.state_stride, ok = pw + (size_t)k * nwn + iw;
                        const R *Op = rp<R>(a.Opert);
                        for (int i = 0; i < njac; i++) {
                            const double d = ((double)Op[(2 + 2 * i) * st + ok] - (double)Op[(3 + 2 * i) * st + ok]) * (0.5 / a.dlnw);
                            double sw[1] = {0.};
#pragma unroll
                            for (int j = 0; j < NP; j++)
                                if (j < npl) sw[0] = fma(sW[j], kof[j] * d, sw[0]);
                            A *const dw[1] = {KW + ((size_t)k * njac + i) * nchan};
                            to_channels<A, 1>(slab, sw, nchan, ms, mb, sMl, sMw, dw, lane);
                        }
                    } else {
                        const double s2[2] = {sk[0], sk[1]};
                        A *const dst[2] = {KT + (size_t)k * nchan, KTZ + (size_t)(k + 1) * nchan};
                        to_channels<A, 2>(slab, s2, nchan, ms, mb, sMl, sMw, dst, lane);
                    }
                    Bzu = Bzl;
                    dBzu = dBzl;
                }
                if (l0 == 0) {
                    double s0[1] = {0.};
#pragma unroll
                    for (int j = 0; j < NP; j++)
                        if (j < npl) s0[0] = fma(sW[j], dn_lev[j], s0[0]);
                    A *const dst[1] = {KTZ};
                    to_channels<A, 1>(slab, s0, nchan, ms, mb, sMl, sMw, dst, lane);
                }
            }
        }
    }
}

// paths per tile: that of rtm_scan_jac_kernel (DESIGN.md section 3.9 has the resource table)
constexpr int OBS_JAC_NP = 4;

template <typename R, typename A, bool FULL>
void launch_t(const RtmObsJacArgs &a, hipStream_t s) {
    dim3 grid(a.nview, a.nprof);
    // the layer groups of launch_rtm_jac_t (jacobian_kernel.hip); inside a G = 8 launch a profile below 24 layers works with 2 of them
    const size_t lds = sizeof(double) * ((size_t)(2 * a.nlay_max + 1) + (size_t)OBS_JAC_NP * a.nlay_max);
    if (a.nlay_max >= 24) hipLaunchKernelGGL((rtm_obs_jac_kernel<R, A, 8, OBS_JAC_NP, FULL>), grid, dim3(64, 8), lds, s, a);
    else hipLaunchKernelGGL((rtm_obs_jac_kernel<R, A, 2, OBS_JAC_NP, FULL>), grid, dim3(64, 2), lds, s, a);
}

}  // namespace

namespace monortm_dev {
void launch_rtm_obs_jac(const RtmObsJacArgs &a, bool full, int out_kind, hipStream_t s) {
    if (full) launch_t<double, double, true>(a, s);   // (monortm_hip_obs_jacobian: real_kind 8 only)
    else if (a.real_kind == 4 && out_kind == 8) launch_t<float, double, false>(a, s);
    else if (a.real_kind == 4) launch_t<float, float, false>(a, s);
    else launch_t<double, double, false>(a, s);
}
}  // namespace monortm_dev
