// rtm_tile.hpp - the steps the radiance kernels that walk NP paths per thread through G layer groups share: rtm_scan_kernel.hip,
// rtm_obs_kernel.hip, rtm_scan_jac_kernel.hip, rtm_obs_jac_kernel.hip (the tile sweep), and with the single-path rtm_jac_kernel of
// jacobian_kernel.hip the two blocks of the adjoint.  ONE definition of each step: what DESIGN.md sections 3.7 - 3.10 say about equal bits
// between these kernels holds because they run the same text, not because copies of it were compiled alike.
// Layout every function assumes: blockDim = (64, G), threadIdx.x = lane = wavenumber, threadIdx.y = g = layer group, a wave each; the
// group walks the 0-based layers [l0, l1); npl <= NP live paths of the tile, a workgroup-uniform count; dynamic LDS sBl [lm] / sBz
// [lm + 1] = hc/kT of the layers / levels, sF [NP][lm] = the tile's factors.
#pragma once
#include "device_common.hpp"

namespace monortm_dev {

// ---- the tile sweep --------------------------------------------------------------------------------------------------------------

// hc/kT of the layers and levels of a profile into sBl / sBz.  All 64 x G threads; NO barrier inside: one follows before sBl / sBz are read.
template <int G, typename R>
__device__ __forceinline__ void tile_load_beta(const R *T, const R *TZ, int nlay, double *sBl, double *sBz) {
    for (int l = threadIdx.y * 64 + threadIdx.x; l < 2 * nlay + 1; l += 64 * G) {
        if (l < nlay) sBl[l] = K_RADCN2 / (double)T[l];
        else sBz[l - nlay] = K_RADCN2 / (double)TZ[l - nlay];
    }
}

// The factors of a tile's npl paths (F: [npl][lm], the first path of the tile) into sF, as doubles; a factor of an active layer that is
// negative or not finite raises ERRBIT_ARG.  All 64 x G threads; NO barrier inside: the caller has one behind it before sF is read, and
// one in front of it where a tile before may still be read.
template <int G, typename R>
__device__ __forceinline__ void tile_load_factors(const R *F, int npl, int nlay, int lm, double *sF, int *errflag) {
    for (int j = 0; j < npl; j++)
        for (int l = threadIdx.y * 64 + threadIdx.x; l < nlay; l += 64 * G) {
            const double f = (double)F[(size_t)j * lm + l];
            if (!(f >= 0. && f < __builtin_inf())) atomicOr(errflag, ERRBIT_ARG);
            sF[j * lm + l] = f;
        }
}

// Per path of the tile the optical depth of the whole column (ODTOT) and of the layers above the group's (above), from the groups'
// partial sums of tau = (double)O * factor rounded ONCE.  O: the thread's wavenumber of layer 0.  TWO workgroup barriers per live
// path (the LDS piece sUp holds one path at a time): called by all 64 x G threads in uniform control flow, with sF complete.
template <typename R, int G, int NP>
__device__ __forceinline__ void tile_optical_depths(const R *O, int nwn, int l0, int l1, int npl, int lm, const double *sF,
                                                    double (&sUp)[G][64], double (&above)[NP], double (&ODTOT)[NP]) {
    const int lane = threadIdx.x, g = threadIdx.y;
    double part[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) part[j] = 0.;
    for (int l = l0; l < l1; l++) {
        const double o = (double)O[(size_t)l * nwn];
#pragma unroll
        for (int j = 0; j < NP; j++)
            if (j < npl) part[j] = part[j] + __dmul_rn(o, sF[j * lm + l]);
    }
#pragma unroll
    for (int j = 0; j < NP; j++) {
        above[j] = 0.;
        ODTOT[j] = 0.;
        if (j < npl) {
            sUp[g][lane] = part[j];
            __syncthreads();
            double below = 0., tot = 0.;
            for (int gg = 0; gg < G; gg++) {
                if (gg < g) below = below + sUp[gg][lane];
                tot = tot + sUp[gg][lane];
            }
            ODTOT[j] = tot;
            above[j] = tot - below - part[j];
            __syncthreads();
        }
    }
}

// The group's forward sums of RAD_UP_DN (RTMmono.f90:193-217) and, with TMR, of CALCTMR (:302-315): layers l1 .. l0+1 (1-based), top
// down; planck of the layer and of its lower level once per layer for the tile, per path tau rounded once and rtm_layer_terms
// (device_common.hpp: rtm_kernel's rounding).  TMR = false: sumexp is not kept and the caller passes one element.  No barrier; a
// wave's trip count is its own.
template <bool TMR, typename R, int NP>
__device__ __forceinline__ void tile_forward_sweep(const R *O, int nwn, int l0, int l1, int npl, int lm, const double *sBl, const double *sBz,
                                                   const double *sF, double c3, double VV, bool up, const double (&above)[NP],
                                                   const double (&ODTOT)[NP], double (&RUP)[NP], double (&RDN)[NP],
                                                   double (&sumexp)[TMR ? NP : 1]) {
    double ODTd[NP], ODTu[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) {
        RUP[j] = 0.;
        RDN[j] = 0.;
        if (TMR) sumexp[j] = 0.;
        ODTd[j] = ODTOT[j] - above[j];  // downward sweep: optical depth from the surface up to and including the layer, running difference
        ODTu[j] = above[j];             // upward sweep: optical depth above the layer
    }
    double bb_top = (up && l1 > l0) ? planck(c3, VV, sBz[l1]) : 0.;  // B at the upper level of the group's top layer
    for (int l = l1; l >= l0 + 1; l--) {
        const double o = (double)O[(size_t)(l - 1) * nwn];
        const double bb = planck(c3, VV, sBl[l - 1]), bbz = planck(c3, VV, sBz[l - 1]);
#pragma unroll
        for (int j = 0; j < NP; j++)
            if (j < npl) {
                double unused = 0.;  // (CALCTMR's sum where it is not kept)
                const double ODVI = __dmul_rn(o, sF[j * lm + l - 1]);
                rtm_layer_terms(ODVI, bb, bbz, bb_top, up, ODTd[j], ODTu[j], RUP[j], RDN[j], TMR ? sumexp[j] : unused);
            }
        bb_top = bbz;
    }
}

// ---- the adjoint (rtm_jac_kernel, rtm_scan_jac_kernel, rtm_obs_jac_kernel) ---------------------------------------------------------

// a + b with b kept as it was rounded: tau = (double)O * factor is rounded ONCE, and the running optical depth above a layer must add that
// tau - left to the compiler, the product is contracted into the sum (fma(O, factor, ODTu)) in one kernel and not in another, and their
// transmittances part by an ulp; in the lowest layers of an opaque channel, where dq/dtau is the residue of a cancellation, that ulp is
// the whole term
__device__ __forceinline__ double add_rounded(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

// s + e = a + b exactly (Knuth): the sum as rounded and what the rounding dropped
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e) {
#pragma clang fp contract(off)
    s = a + b;
    const double bv = s - a;
    e = (a - (s - bv)) + (b - bv);
}

// What pass 2 needs of one (layer, path) for the upward sweep: t = exp(-tau), the Pade weight and 1 / (1 + pade), emis = 1 - t, TRu =
// exp(-ODTu) (ODTu: the optical depth above the layer), bup = B + pade Bzu and the layer's upward term upk.  ONE definition with
// contraction off: jac_up_sum and jac_layer_terms must form upk to the same bit (see jac_up_sum).
__device__ __forceinline__ void jac_up_parts(double tau, double B, double Bzu, bool up, double ODTu, double &t, double &pade, double &rp1,
                                             double &emis, double &TRu, double &bup, double &upk) {
#pragma clang fp contract(off)
    t = exp_cw(-tau);
    pade = 0.193 * tau + 0.013 * (tau * tau);
    rp1 = rcp2(1. + pade);
    emis = 1. - t;
    TRu = up ? exp_cw(-ODTu) : 0.;
    bup = B + pade * Bzu;
    upk = up ? ((TRu * emis) * bup) * rp1 : 0.;
}

// Pass 2 walks a group's layers top-down and needs, per layer, the sum of the upward terms of the layers BELOW it.  Held as a running
// difference from the rounded group sum of pass 1, that sum keeps ~10 eps x RUP where the truth is e^-tau of nothing (at and under an
// opaque layer) - invisible in dq/dtau on the column's scale, but K_PATH = O x dq/dtau multiplies it by the opaque layer's O (1e6
// against a column whose other layers have O = 1e-5: 2.4e-5 of the column's largest K_PATH; LABNOTES section 23).  So the group's sum
// is formed once more from pass 2's OWN terms, error-free (H + L = the exact sum of the rounded terms up to eps^2), and
// jac_layer_terms takes the same terms off again, error-free: what is left under an opaque layer is eps^2 x RUP.
// One layer's step of that sum, layers top-down as in pass 2 (ODTu advances as there).
__device__ __forceinline__ void jac_up_sum(double tau, double B, double Bzu, bool up, double &ODTu, double &H, double &L) {
    double t, pade, rp1, emis, TRu, bup, upk, s, e;
    jac_up_parts(tau, B, Bzu, up, ODTu, t, pade, rp1, emis, TRu, bup, upk);
    ODTu = add_rounded(ODTu, tau);
    two_sum(H, upk, s, e);
    H = s;
    L = L + e;
}

// One path's epilogue of pass 1: RAD through the irt forms (RTMmono.f90:138-147, as rtm_combine rounds it), lx = log(c3 / RAD + 1) (TB =
// RADCN2 v / lx), dq = dq/dRAD and the weights gU = dq/dRUP, gD = dq/dRDN, gT = TRTOT dq/dTRTOT of pass 2.  Pure arithmetic of one
// thread, as is jac_path_sfc below: no barrier, no store.
__device__ __forceinline__ void jac_path_weights(int irt, double TRTOT, double RUP, double RDN, double ESFC, double RSFC, double SURFRAD,
                                                 double COSMOS, double c3, double VV, int quantity, double &RAD, double &lx, double &dq,
                                                 double &gU, double &gD, double &gT) {
    double cU = 0., cD = 0., cT = 0.;   // dRAD/dRUP, dRAD/dRDN, dRAD/dTRTOT
    RAD = 0.;
    if (irt == 1) {
        RAD = fma(TRTOT, fma(RSFC, fma(TRTOT, COSMOS, RDN), ESFC * SURFRAD), RUP);
        cU = 1.; cD = TRTOT * RSFC; cT = ESFC * SURFRAD + RSFC * RDN + 2. * RSFC * TRTOT * COSMOS;
    }
    if (irt == 2) {
        RAD = fma(TRTOT, fma(TRTOT, COSMOS, RDN), RUP);
        cU = 1.; cD = TRTOT; cT = RDN + 2. * TRTOT * COSMOS;
    }
    if (irt == 3) {
        RAD = fma(TRTOT, COSMOS, RDN);
        cU = 0.; cD = 1.; cT = COSMOS;
    }
    const double X = c3 / RAD + 1.;
    lx = log(X);
    dq = 1.;
    // dTB/dRAD = RADCN2 v (c3 / RAD) / (ln^2 X X RAD); RAD enters once per factor: RAD^2 underflows for RAD < 1.5e-154 (a cold opaque
    // column in the ultraviolet), where the derivative is finite
    if (quantity == 1) dq = (K_RADCN2 * VV) * ((c3 / RAD) / X) / ((lx * lx) * RAD);
    gU = dq * cU;
    gD = dq * cD;
    gT = dq * cT * TRTOT;
}
// ... and its surface terms dq/dTMPSFC, dq/dEMISS, dq/dREFLC (0 unless irt = 1), for the threads that store or contract them.  ex_s =
// exp(hc v / k tmpsfc), the exponential SURFRAD was formed with; where it overflows, dq/dTMPSFC is 0.
__device__ __forceinline__ void jac_path_sfc(int irt, double dq, double TRTOT, double RDN, double ESFC, double SURFRAD, double COSMOS,
                                             double VV, double ex_s, double tmpsfc, double (&ksfc)[3]) {
    ksfc[0] = ksfc[1] = ksfc[2] = 0.;
    if (irt == 1) {
        const double xs = VV * (K_RADCN2 / tmpsfc);
        // ex_s = inf (hc v / k tmpsfc > 709.78: a cold surface in the ultraviolet): SURFRAD = 0 and inf / inf is NaN where dB/dT has
        // underflowed to 0, as in planck_d
        const double dBs = (ex_s == __builtin_inf()) ? 0. : SURFRAD * (ex_s / (ex_s - 1.)) * (xs / tmpsfc);
        ksfc[0] = dq * TRTOT * ESFC * dBs;
        ksfc[1] = dq * TRTOT * SURFRAD;
        ksfc[2] = dq * TRTOT * (RDN + TRTOT * COSMOS);
    }
}

// The downward sweep's term of level l1 from the layer ABOVE a group's top layer (its lower level), which pass 2 starts from where
// l1 < nlay: tau of that layer, ODTd = the optical depth up to and including the group's top layer, dBzu = dB/dT at level l1.
__device__ __forceinline__ double jac_dn_lev_above(double tau, double gD, double ODTd, double dBzu) {
#pragma clang fp contract(off)
    const double pade = 0.193 * tau + 0.013 * (tau * tau);
    return gD * exp_cw(-ODTd) * (1. - exp_cw(-tau)) * pade * rcp2(1. + pade) * dBzu;
}

// Pass 2 for one (layer k, path), layers taken top-down: tau the layer's optical depth along the path (rounded once), B / dB, Bzl /
// dBzl, Bzu / dBzu the Planck function and dB/dT of the layer, its lower and its upper level.  Advances the running optical depths
// (ODTd, ODTu), the sums of the other layers' terms (upIncl + upLo -> sum_{l<k} up_l, error-free: in, the lower groups' sum plus
// jac_up_sum's H and L over the group's layers down to this one; dnAbove -> sum_{l>=k} dn_l) and dn_lev (in: the
// downward term of level k + 1 from the layer above, out: of level k from this layer).  Out: ko = dq/dtau_k, kt = the Planck term of
// dq/dT_k, ktz = dq/dTZ_{k+1}.  Pure arithmetic of one thread: no barrier, no store.
__device__ __forceinline__ void jac_layer_terms(double tau, double B, double dB, double Bzl, double dBzl, double Bzu, double dBzu, bool up,
                                                double gU, double gD, double gT, double &ODTd, double &ODTu, double &upIncl,
                                                double &upLo, double &dnAbove, double &dn_lev, double &ko, double &kt, double &ktz) {
    // every product and sum rounded as written: which of them the compiler would fuse depends on the code around the call, and the
    // instantiations of one kernel (a profile alone: G = 2; inside a batch: G = 8 working with two groups) must agree to the bit
#pragma clang fp contract(off)
    double t, pade, rp1, emis, TRu, bup, upk, s, e;
    jac_up_parts(tau, B, Bzu, up, ODTu, t, pade, rp1, emis, TRu, bup, upk);
    const double pp = 0.193 + 0.026 * tau;
    ODTd = ODTd - tau;
    const double TRd = exp_cw(-ODTd);
    ODTu = add_rounded(ODTu, tau);
    const double bdn = B + pade * Bzl;
    const double dn = ((TRd * emis) * bdn) * rp1;
    two_sum(upIncl, -upk, s, e);   // the very upk jac_up_sum added
    upIncl = s;
    upLo = upLo + e;
    const double upBelow = upIncl + upLo;   // sum_{l<k} up_l
    const double dfdn = t * bdn * rp1 + emis * pp * (Bzl - B) * (rp1 * rp1);
    const double dfup = t * bup * rp1 + emis * pp * (Bzu - B) * (rp1 * rp1);
    const double dRUP = TRu * dfup - upBelow, dRDN = TRd * dfdn - dnAbove;
    dnAbove = dnAbove + dn;
    ko = gU * dRUP + gD * dRDN - gT;
    kt = (gU * TRu + gD * TRd) * emis * rp1 * dB;
    const double wz = emis * pade * rp1;
    ktz = gU * TRu * wz * dBzu + dn_lev;
    dn_lev = gD * TRd * wz * dBzl;
}

}  // namespace monortm_dev
