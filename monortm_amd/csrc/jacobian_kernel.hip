// jacobian_kernel.hip - Jacobians of RAD / TB (monortm_hip_rtm_jac, monortm_hip_jacobian) for gfx950.  See DESIGN.md section 3.6.
//   jac_perturb_kernel: the base and the +-h states of a Jacobian call as MODM inputs (T +- h; WKL of one molecule, P or WBRODL
//                       x (1 +- eps))
//   rtm_jac_kernel:     the exact adjoint of RAD_UP_DN + RTM (reference src/RTMmono.f90:13-221), chained with the central
//                       differences of the perturbed states' optical depths (FULL)
#include "cloud_tkc.hpp"
#include "rtm_tile.hpp"   // jac_path_weights, jac_layer_terms, jac_dn_lev_above: shared with rtm_scan_jac_kernel and rtm_obs_jac_kernel

namespace {
using namespace monortm_dev;

// ------------------------------------------------------------------------------------------------
// jac_perturb_kernel: one thread per (state, profile, layer).  State 0 = the base, 1 / 2 = T + h / T - h, 3 + 2i / 4 + 2i =
// WKL(jac_mol[i]) x (1 + eps) / (1 - eps), or P / WBRODL x (1 +- eps) where jac_mol[i] is MONORTM_JVAR_P / _WBROD (DESIGN.md
// section 3.11).  Layers >= nlay[p] are copied unchanged (the caller's padding).
// State rayl_state (when not 0) scales nothing and holds the layer as the Rayleigh term alone sees it: the term is XRAYL f(v, T) WTOT
// with WTOT = WBRODL + sum of WKL, summed in the order of continuum_kernel.hip, and nothing else of MODM survives WKL = 0, CLW = 0.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jac_perturb_kernel(JacPerturbArgs a) {
    const size_t npl = (size_t)a.nprof * a.nlay_max;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npl * (size_t)a.nstate) return;
    const int s = (int)(i / npl);
    const size_t pl = i - (size_t)s * npl;
    const int prof = (int)(pl / a.nlay_max), k = (int)(pl - (size_t)prof * a.nlay_max);
    const bool in = k < a.nlay[prof];
    const double *src_l[4] = {a.P, a.T, a.CLW, a.WBRODL};
    double *dst_l[4] = {a.xP, a.xT, a.xCLW, a.xWBRODL};
    for (int f = 0; f < 4; f++) dst_l[f][(size_t)s * npl + pl] = src_l[f][pl];
    if (in && (s == 1 || s == 2)) a.xT[(size_t)s * npl + pl] = a.T[pl] + (s == 1 ? a.dt : -a.dt);
    const int var = (s >= 3) ? a.jac_mol[(s - 3) >> 1] : 0;   // what this state scales: a 1-based molecule, or P / WBRODL
    const int mol = var - 1;                                  // (0-based; matches no molecule for the base, T, P and WBRODL states)
    const double fac = ((s - 3) & 1) ? 1. - a.dlnw : 1. + a.dlnw;
    if (in && var == MONORTM_JVAR_P) a.xP[(size_t)s * npl + pl] = a.P[pl] * fac;
    if (in && var == MONORTM_JVAR_WBROD) a.xWBRODL[(size_t)s * npl + pl] = a.WBRODL[pl] * fac;
    const double *w = a.WKL + pl * a.nmol;
    double *xw = a.xWKL + ((size_t)s * npl + pl) * a.nmol;
    for (int m = 0; m < a.nmol; m++) xw[m] = (in && m == mol) ? w[m] * fac : w[m];
    if (in && a.rayl_state != 0 && s == a.rayl_state) {
        double WTOT = a.WBRODL[pl];
        for (int m = 0; m < a.nmol; m++) { WTOT = WTOT + w[m]; xw[m] = 0.; }
        a.xWBRODL[(size_t)s * npl + pl] = WTOT;
        a.xCLW[(size_t)s * npl + pl] = 0.;
    }
    if (k == 0) a.xnlay[(size_t)s * a.nprof + prof] = a.nlay[prof];
}

// planck_d (B(T) and dB/dT): device_common.hpp, shared with rtm_scan_jac_kernel.hip

// ------------------------------------------------------------------------------------------------
// rtm_jac_kernel: block = 64 wavenumbers x G layer groups of one profile, as rtm_kernel.  With tau = O_k, t = exp(-tau),
// p = 0.193 tau + 0.013 tau^2 (the Pade weight), a sweep's own-layer term is TR (1 - t) (B + p Bz) / (1 + p); Bz is the upper
// level for RUP, the lower for RDN (RTMmono.f90:197,210).
//   pass 1: the group sums of the optical depth, the upward and the downward terms (the forward sums of rtm_kernel, same order),
//           exchanged through LDS;
//   pass 2: every group walks its layers again, top-down, and writes per layer
//     dRUP/dtau_k = TRu_k df_up/dtau - sum_{l<k} up_l   (tau_k lies above every lower layer)
//     dRDN/dtau_k = TRd_k df_dn/dtau - sum_{l>k} dn_l
//     dTRTOT/dtau_k = -TRTOT, combined through the irt forms of RAD (RTMmono.f90:138-147) and dTB/dRAD,
//   and the Planck terms: dB(T_k) into K_T, dB(TZ_j) of both sweeps into K_TZ.  Level j is written by the group that owns layer
//   j - 1 (level 0 by group 0); the downward term of the layer above a group's top is formed once more for it.
// The arithmetic of both - RAD's irt forms with dq/dRAD and the weights, and the per-layer body - is rtm_tile.hpp's, one definition
// for this kernel and the scan kernels' NP paths; this file keeps the exchange through LDS, the FULL chain and the stores.
// FULL (monortm_hip_jacobian): the central differences of the perturbed states' O (states 1, 2: T +- h; 3 + 2i, 4 + 2i: ln WKL of
// jac_mol[i] +- eps) times dq/dO_k into K_T and K_W, dq/dO_k ODCLW_TKC(wn, T_k, 1) into K_CLW.
// R: element type of the REAL arrays; the arithmetic is double.
// ------------------------------------------------------------------------------------------------
template <typename R, int G, bool FULL>
__global__ __launch_bounds__(64 * G) void rtm_jac_kernel(RtmJacArgs a) {
    __shared__ double sPart[G][64], sUp[G][64], sDn[G][64];
    extern __shared__ __attribute__((aligned(16))) double sBeta[];  // [nlay_max] hc/kT of the layers, [nlay_max + 1] of the levels
    const int lane = threadIdx.x, g = threadIdx.y;
    const int iw0 = blockIdx.x * 64 + lane, prof = blockIdx.y;
    const int nwn = a.nwn, nlm = a.nlay_max;
    const bool valid = iw0 < nwn;
    const int iw = valid ? iw0 : nwn - 1;
    const int nlay = max(0, min(a.nlay[prof], nlm)), irt = a.irt[prof];
    const double VV = a.wn[iw];
    const size_t pw = (size_t)prof * nlm * nwn;   // (profile, layer 0, wn 0) of the [nprof][nlay_max][nwn] arrays
    const R *O = rp<R>(a.O) + pw + iw;
    const R *T = rp<R>(a.T) + (size_t)prof * nlm, *TZ = rp<R>(a.TZ) + (size_t)prof * (nlm + 1);
    double *sBl = sBeta, *sBz = sBeta + nlm;
    tile_load_beta<G>(T, TZ, nlay, sBl, sBz);
    const int chunk = (nlay + G - 1) / G;
    const int l0 = min(nlay, g * chunk), l1 = min(nlay, l0 + chunk);  // 0-based layer range [l0, l1)

    double part = 0.;
    for (int l = l0; l < l1; l++) part = part + (double)O[(size_t)l * nwn];
    sPart[g][lane] = part;
    __syncthreads();
    double below = 0., ODTOT = 0.;
    for (int gg = 0; gg < G; gg++) {
        if (gg < g) below = below + sPart[gg][lane];
        ODTOT = ODTOT + sPart[gg][lane];
    }
    const double above = ODTOT - below - part;
    const double c3 = K_RADCN1 * (VV * VV * VV);
    const bool up = irt != 3;

    // ---- pass 1: the forward sums of rtm_kernel (RTMmono.f90:193-217), layers l1 .. l0+1 (1-based)
    double RUPg = 0., RDNg = 0.;
    {
        double ODTd = ODTOT - above, ODTu = above, unused = 0.;  // (CALCTMR's sum: not needed here)
        double bb_top = (up && l1 > l0) ? planck(c3, VV, sBz[l1]) : 0.;
        for (int l = l1; l >= l0 + 1; l--) {
            const double ODVI = (double)O[(size_t)(l - 1) * nwn];
            const double bb = planck(c3, VV, sBl[l - 1]), bbz = planck(c3, VV, sBz[l - 1]);
            rtm_layer_terms(ODVI, bb, bbz, bb_top, up, ODTd, ODTu, RUPg, RDNg, unused);  // rtm_kernel's rounding (device_common.hpp)
            bb_top = bbz;
        }
    }
    sUp[g][lane] = RUPg;
    sDn[g][lane] = RDNg;
    __syncthreads();
    // totals in the reference's visiting order (every group needs them), and the sums of the other groups
    double RUP = 0., RDN = 0., upLow = 0., dnHigh = 0.;
    for (int gg = 0; gg < G; gg++) {
        RUP = RUP + sUp[gg][lane];
        if (gg < g) upLow = upLow + sUp[gg][lane];
    }
    for (int gg = G - 1; gg >= 0; gg--) {
        RDN = RDN + sDn[gg][lane];
        if (gg > g) dnHigh = dnHigh + sDn[gg][lane];
    }
    const double TRTOT = exp(-ODTOT);
    const size_t o = (size_t)prof * nwn + iw;
    const double TSKY = 2.75;
    const double tsfc_in = (double)rp<R>(a.tmpsfc)[prof];
    const double tmpsfc = (irt == 3 || irt == 2) ? TSKY : tsfc_in;  // RTMmono.f90:113-124 (not written back here)
    const double ex_s = exp(VV * (K_RADCN2 / tmpsfc)), ex_c = exp(VV * (K_RADCN2 / TSKY));
    const double SURFRAD = c3 / (ex_s - 1.), COSMOS = c3 / (ex_c - 1.);
    const double ESFC = (double)rp<R>(a.emiss)[o], RSFC = (double)rp<R>(a.reflc)[o];
    if (!valid) return;   // (no barrier below; leaving here and not behind the stores saves registers: DESIGN.md section 3.6)
    // RAD through its irt forms, dq/dRAD, the weights of pass 2 and the surface terms (rtm_tile.hpp)
    double RAD, lx, dq, gU, gD, gT;
    jac_path_weights(irt, TRTOT, RUP, RDN, ESFC, RSFC, SURFRAD, COSMOS, c3, VV, a.quantity, RAD, lx, dq, gU, gD, gT);
    if (g == 0) {
        wp<R>(a.RAD)[o] = (R)RAD;
        wp<R>(a.TB)[o] = (R)(K_RADCN2 * VV / lx);
        R *ks = wp<R>(a.K_SFC) + (size_t)prof * 3 * nwn + iw;
        double ksfc[3];
        jac_path_sfc(irt, dq, TRTOT, RDN, ESFC, SURFRAD, COSMOS, VV, ex_s, tmpsfc, ksfc);
        ks[0] = (R)ksfc[0];
        ks[nwn] = (R)ksfc[1];
        ks[2 * (size_t)nwn] = (R)ksfc[2];
    }

    // ---- pass 2: per-layer derivatives, layers l1-1 .. l0 (0-based), top-down
    R *KO = a.K_O ? wp<R>(a.K_O) + pw + iw : nullptr;
    R *KT = wp<R>(a.K_T) + pw + iw;
    R *KTZ = wp<R>(a.K_TZ) + (size_t)prof * (nlm + 1) * nwn + iw;
    R *KW = FULL ? wp<R>(a.K_W) + pw * a.njac + iw : nullptr;
    R *KC = FULL ? wp<R>(a.K_CLW) + pw + iw : nullptr;
    if (l1 > l0) {
        double ODTd = ODTOT - above, ODTu = above;
        // the sum of up_l, l <= the group's top layer, from pass 2's own terms, error-free (jac_up_sum, rtm_tile.hpp)
        double upIncl = 0., upLo = 0.;
        if (up) {
            double ODTu2 = above, B2, dB2, Bzu2, dBzu2;
            planck_d(c3, VV, sBz[l1], &Bzu2, &dBzu2);
            for (int k = l1 - 1; k >= l0; k--) {
                planck_d(c3, VV, sBl[k], &B2, &dB2);
                jac_up_sum((double)O[(size_t)k * nwn], B2, Bzu2, up, ODTu2, upIncl, upLo);
                planck_d(c3, VV, sBz[k], &Bzu2, &dBzu2);
            }
            double s2, e2;
            two_sum(upIncl, upLow, s2, e2);
            upIncl = s2;
            upLo = upLo + e2;
        }
        double dnAbove = dnHigh;        // sum of dn_l, l > current layer
        // B and dB/dT at the upper level of the group's top layer, and the downward sweep's term of level l1 from the layer
        // above (its lower level); level nlay (top of the atmosphere) is the lower level of no layer
        double Bzu, dBzu;
        planck_d(c3, VV, sBz[l1], &Bzu, &dBzu);
        double dn_lev = 0.;
        if (l1 < nlay) dn_lev = jac_dn_lev_above((double)O[(size_t)l1 * nwn], gD, ODTd, dBzu);
        for (int k = l1 - 1; k >= l0; k--) {
            const double tau = (double)O[(size_t)k * nwn];
            double B, dB, Bzl, dBzl;
            planck_d(c3, VV, sBl[k], &B, &dB);
            planck_d(c3, VV, sBz[k], &Bzl, &dBzl);
            double ko, kt, ktz;
            jac_layer_terms(tau, B, dB, Bzl, dBzl, Bzu, dBzu, up, gU, gD, gT, ODTd, ODTu, upIncl, upLo, dnAbove, dn_lev, ko, kt, ktz);   // (rtm_tile.hpp)
            KTZ[(size_t)(k + 1) * nwn] = (R)ktz;
            Bzu = Bzl;
            dBzu = dBzl;
            if (KO) KO[(size_t)k * nwn] = (R)ko;
            if constexpr (FULL) {
                const size_t st = a.state_stride, ok = pw + (size_t)k * nwn + iw;
                const R *Op = rp<R>(a.Opert);
                kt += ko * (((double)Op[ok] - (double)Op[st + ok]) * (0.5 / a.dt));
                for (int i = 0; i < a.njac; i++) {
                    const double d = ((double)Op[(2 + 2 * i) * st + ok] - (double)Op[(3 + 2 * i) * st + ok]) * (0.5 / a.dlnw);
                    KW[((size_t)k * a.njac + i) * nwn] = (R)(ko * d);
                }
                KC[(size_t)k * nwn] = (R)(ko * odclw_tkc(VV, (double)T[k], 1.0));
            }
            KT[(size_t)k * nwn] = (R)kt;
        }
        if (l0 == 0) KTZ[0] = (R)dn_lev;
    }
    // zero padding: layers >= nlay, levels > nlay
    for (int k = nlay + g; k < nlm; k += G) {
        if (KO) KO[(size_t)k * nwn] = (R)0;
        KT[(size_t)k * nwn] = (R)0;
        KTZ[(size_t)(k + 1) * nwn] = (R)0;
        if constexpr (FULL) {
            for (int i = 0; i < a.njac; i++) KW[((size_t)k * a.njac + i) * nwn] = (R)0;
            KC[(size_t)k * nwn] = (R)0;
        }
    }
    if (nlay == 0 && g == 0) KTZ[0] = (R)0;
}

template <typename R, bool FULL>
void launch_rtm_jac_t(const RtmJacArgs &a, hipStream_t s) {
    dim3 grid((a.nwn + 63) / 64, a.nprof);
    // the layer groups of launch_rtm (rtm_kernel.hip), except that few workgroups of many layers take 8 groups, not 16: a
    // 1024-thread workgroup leaves 128 VGPRs, and the second pass spills there (FULL: 12 bytes a lane)
    const size_t lds = sizeof(double) * (size_t)(2 * a.nlay_max + 1);
    if (a.nlay_max >= 24) hipLaunchKernelGGL((rtm_jac_kernel<R, 8, FULL>), grid, dim3(64, 8), lds, s, a);
    else hipLaunchKernelGGL((rtm_jac_kernel<R, 2, FULL>), grid, dim3(64, 2), lds, s, a);
}

}  // namespace

namespace monortm_dev {
void launch_jac_perturb(const JacPerturbArgs &a, hipStream_t s) {
    const size_t n = (size_t)a.nstate * a.nprof * a.nlay_max;
    hipLaunchKernelGGL(jac_perturb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}
void launch_rtm_jac(const RtmJacArgs &a, bool full, hipStream_t s) {
    if (full) launch_rtm_jac_t<double, true>(a, s);   // (monortm_hip_jacobian: real_kind 8 only)
    else if (a.real_kind == 4) launch_rtm_jac_t<float, false>(a, s);
    else launch_rtm_jac_t<double, false>(a, s);
}
}  // namespace monortm_dev
