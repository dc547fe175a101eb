// rtm_scan_jac_kernel.hip - Jacobians of RAD / TB along several paths through one atmosphere (monortm_hip_rtm_scan_jac,
// monortm_hip_scan_jacobian) for gfx950: the exact adjoint of RAD_UP_DN + RTM (reference src/RTMmono.f90:13-221) per path, from ONE
// set of optical depths and ONE set of perturbed MODM states.  See DESIGN.md section 3.8.
#include "cloud_tkc.hpp"
#include "rtm_tile.hpp"

namespace {
using namespace monortm_dev;

// The layout of rtm_scan_kernel (block = 64 wavenumbers x G layer groups of a profile, NP paths per thread, blockIdx.z = tile of NP
// paths of which the last may hold fewer - npl, a workgroup-uniform count, so the barriers below stay in uniform control flow; hc / kT
// of the layers and levels and the tile's factors in LDS; tau = (double)O * factor rounded ONCE) with the two passes of rtm_jac_kernel
// per path, its operations in its order: on optical depths a caller scaled beforehand the two kernels differ by instruction
// contraction only.  The preloads, the optical depths per path and the forward sweep are rtm_tile.hpp's, shared with rtm_scan_kernel
// and the obs kernels; a path's pass-1 epilogue (jac_path_weights) and the per-(layer, path) body of pass 2 (jac_layer_terms,
// jac_dn_lev_above) are rtm_tile.hpp's as well, shared with rtm_jac_kernel and rtm_obs_jac_kernel.
//   pass 1: the group sums of the optical depth, the upward and the downward terms (rtm_layer_terms), exchanged through LDS one path
//           at a time; RAD, TB, K_SFC and the weights gU = dq/dRUP, gD = dq/dRDN, gT = TRTOT dq/dTRTOT of every path;
//   pass 2: every group walks its layers again, top-down.  Per layer, ONCE for the tile: (double)O, B and dB/dT of the layer and of its
//           lower level, and with FULL the difference quotients of the perturbed states' O and ODCLW_TKC(wn, T_k, 1) - none of them
//           depends on the path.  Per path: ko = dq/dtau_k exactly as rtm_jac_kernel forms it, then
//             K_O = factor ko (dq / dO_k of the vertical O),  K_PATH = O ko (dq / dfactor_k),
//             K_T = the Planck term (+ K_O dO_k/dT_k),  K_W = K_O dO_k/dlnW,  K_CLW = K_O ODCLW_TKC(wn, T_k, 1),  K_TZ as rtm_jac_kernel.
// Factors of layers >= nlay[p] are never read; a factor of an active layer that is negative or not finite raises ERRBIT_ARG.
// R: element type of the REAL arrays; the arithmetic is double.
template <typename R, int G, int NP, bool FULL>
__global__ __launch_bounds__(64 * G) void rtm_scan_jac_kernel(RtmScanJacArgs a) {
    __shared__ double sUp[G][64], sDn[G][64];
    extern __shared__ __attribute__((aligned(16))) double sBeta[];  // [nlay_max] hc/kT of the layers, [nlay_max + 1] of the levels, [NP][nlay_max] factors
    const int lane = threadIdx.x, g = threadIdx.y;
    const int iw0 = blockIdx.x * 64 + lane, prof = blockIdx.y;
    const int j0 = blockIdx.z * NP, npl = min(NP, a.npath - j0);
    const int nwn = a.nwn, lm = a.nlay_max;
    const bool valid = iw0 < nwn;
    const int iw = valid ? iw0 : nwn - 1;
    const int nlay = max(0, min(a.nlay[prof], lm)), irt = a.irt[prof];
    const double VV = a.wn[iw];
    const size_t pw = (size_t)prof * lm * nwn;   // (profile, layer 0, wn 0) of the [nprof][nlay_max][nwn] arrays
    const R *O = rp<R>(a.O) + pw + iw;
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

    // ---- pass 1: the group's forward sums (rtm_tile.hpp)
    double RUPg[NP], RDNg[NP], no_tmr[1];
    tile_forward_sweep<false>(O, nwn, l0, l1, npl, lm, sBl, sBz, sF, c3, VV, up, above, ODTOT, RUPg, RDNg, no_tmr);
    // the surface and the cosmic background: the same for every path of the tile
    const double TSKY = 2.75;
    const double tsfc_in = (double)rp<R>(a.tmpsfc)[prof];
    const double tmpsfc = (irt == 3 || irt == 2) ? TSKY : tsfc_in;  // RTMmono.f90:113-124 (not written back here)
    const double ex_s = exp(VV * (K_RADCN2 / tmpsfc)), ex_c = exp(VV * (K_RADCN2 / TSKY));
    const double SURFRAD = c3 / (ex_s - 1.), COSMOS = c3 / (ex_c - 1.);
    // totals in the reference's visiting order (every group needs them) and the sums of the other groups, one path at a time; then
    // RAD, TB, K_SFC and the weights of the path
    double gU[NP], gD[NP], gT[NP], upLow0[NP], dnHigh0[NP];
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
            const size_t pj = (size_t)prof * a.npath + j0 + j;
            const size_t o = pj * nwn + iw;
            const size_t os = a.sfc_per_path ? o : (size_t)prof * nwn + iw;
            const double ESFC = (double)rp<R>(a.emiss)[os], RSFC = (double)rp<R>(a.reflc)[os];
            double RAD, lx, dq;
            jac_path_weights(irt, TRTOT, RUP, RDN, ESFC, RSFC, SURFRAD, COSMOS, c3, VV, a.quantity, RAD, lx, dq, gU[j], gD[j], gT[j]);
            if (g == 0 && valid) {
                wp<R>(a.RAD)[o] = (R)RAD;
                wp<R>(a.TB)[o] = (R)(K_RADCN2 * VV / lx);
                R *ks = wp<R>(a.K_SFC) + pj * 3 * nwn + iw;
                double ksfc[3];
                jac_path_sfc(irt, dq, TRTOT, RDN, ESFC, SURFRAD, COSMOS, VV, ex_s, tmpsfc, ksfc);
                ks[0] = (R)ksfc[0];
                ks[nwn] = (R)ksfc[1];
                ks[2 * (size_t)nwn] = (R)ksfc[2];
            }
            upLow0[j] = upLow;              // sum of up_l, l < the group's bottom layer
            dnHigh0[j] = dnHigh;            // sum of dn_l, l > the group's top layer
        }
    }
    if (!valid) return;   // (no barrier below)

    // ---- pass 2: per-layer derivatives, layers l1-1 .. l0 (0-based), top-down
    const size_t pj0 = (size_t)prof * a.npath + j0;          // (profile, first path of the tile)
    const size_t lw = (size_t)lm * nwn, zw = (size_t)(lm + 1) * nwn;
    R *KO = a.K_O ? wp<R>(a.K_O) + pj0 * lw + iw : nullptr;
    R *KP = a.K_PATH ? wp<R>(a.K_PATH) + pj0 * lw + iw : nullptr;
    R *KT = wp<R>(a.K_T) + pj0 * lw + iw;
    R *KTZ = wp<R>(a.K_TZ) + pj0 * zw + iw;
    R *KW = FULL ? wp<R>(a.K_W) + pj0 * lw * a.njac + iw : nullptr;
    R *KC = FULL ? wp<R>(a.K_CLW) + pj0 * lw + iw : nullptr;
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
            double kof[NP];   // K_O of the layer: factor x dq/dtau
#pragma unroll
            for (int j = 0; j < NP; j++) {
                kof[j] = 0.;
                if (j < npl) {
                    const double f = sF[j * lm + k];
                    double ko, kt, ktz;
                    jac_layer_terms(__dmul_rn(o, f), B, dB, Bzl, dBzl, Bzu, dBzu, up, gU[j], gD[j], gT[j], ODTd[j], ODTu[j], upIncl[j], upLo[j],
                                    dnAbove[j], dn_lev[j], ko, kt, ktz);   // (rtm_tile.hpp)
                    const size_t jk = (size_t)j * lw + (size_t)k * nwn;
                    KTZ[(size_t)j * zw + (size_t)(k + 1) * nwn] = (R)ktz;
                    kof[j] = __dmul_rn(f, ko);
                    if (KO) KO[jk] = (R)kof[j];
                    if (KP) KP[jk] = (R)__dmul_rn(o, ko);
                    if constexpr (FULL) {
                        kt += kof[j] * dOdT;
                        KC[jk] = (R)(kof[j] * clw1);
                    }
                    KT[jk] = (R)kt;
                }
            }
            if constexpr (FULL) {
                const size_t st = a.state_stride, ok = pw + (size_t)k * nwn + iw;
                const R *Op = rp<R>(a.Opert);
                for (int i = 0; i < a.njac; i++) {
                    const double d = ((double)Op[(2 + 2 * i) * st + ok] - (double)Op[(3 + 2 * i) * st + ok]) * (0.5 / a.dlnw);
#pragma unroll
                    for (int j = 0; j < NP; j++)
                        if (j < npl) KW[((size_t)j * lm + k) * a.njac * nwn + (size_t)i * nwn] = (R)(kof[j] * d);
                }
            }
            Bzu = Bzl;
            dBzu = dBzl;
        }
        if (l0 == 0) {
#pragma unroll
            for (int j = 0; j < NP; j++)
                if (j < npl) KTZ[(size_t)j * zw] = (R)dn_lev[j];
        }
    }
    // zero padding: layers >= nlay, levels > nlay
    for (int j = 0; j < npl; j++) {
        for (int k = nlay + g; k < lm; k += G) {
            const size_t jk = (size_t)j * lw + (size_t)k * nwn;
            if (KO) KO[jk] = (R)0;
            if (KP) KP[jk] = (R)0;
            KT[jk] = (R)0;
            KTZ[(size_t)j * zw + (size_t)(k + 1) * nwn] = (R)0;
            if constexpr (FULL) {
                for (int i = 0; i < a.njac; i++) KW[((size_t)j * lm + k) * a.njac * nwn + (size_t)i * nwn] = (R)0;
                KC[jk] = (R)0;
            }
        }
        if (nlay == 0 && g == 0) KTZ[(size_t)j * zw] = (R)0;
    }
}

// paths per thread: the largest of 1, 2, 4 at which no instantiation uses scratch (DESIGN.md section 3.8 has the table)
constexpr int SCAN_JAC_NP = 4;

template <typename R, bool FULL>
void launch_t(const RtmScanJacArgs &a, hipStream_t s) {
    dim3 grid((a.nwn + 63) / 64, a.nprof, (a.npath + SCAN_JAC_NP - 1) / SCAN_JAC_NP);
    // the layer groups of launch_rtm_jac_t (jacobian_kernel.hip): no 1024-thread variant, the second pass spills at 128 VGPRs
    const size_t lds = sizeof(double) * ((size_t)(2 * a.nlay_max + 1) + (size_t)SCAN_JAC_NP * a.nlay_max);
    if (a.nlay_max >= 24) hipLaunchKernelGGL((rtm_scan_jac_kernel<R, 8, SCAN_JAC_NP, FULL>), grid, dim3(64, 8), lds, s, a);
    else hipLaunchKernelGGL((rtm_scan_jac_kernel<R, 2, SCAN_JAC_NP, FULL>), grid, dim3(64, 2), lds, s, a);
}

}  // namespace

namespace monortm_dev {
void launch_rtm_scan_jac(const RtmScanJacArgs &a, bool full, hipStream_t s) {
    if (full) launch_t<double, true>(a, s);   // (monortm_hip_scan_jacobian: real_kind 8 only)
    else if (a.real_kind == 4) launch_t<float, false>(a, s);
    else launch_t<double, false>(a, s);
}
}  // namespace monortm_dev
