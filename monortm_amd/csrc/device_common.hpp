// device_common.hpp - shared declarations of the MI355X (gfx950 / CDNA4) implementation:
// monortm_amd/csrc - MI355X (gfx950 / CDNA4) implementation of monoRTM's optical-depth and
// radiative-transfer hot path behind the C ABI of include/monortm_hip.h.
//
// Reference behaviour being replaced (paths relative to /root/reference):
//   MODM      src/modm.f90:21-274      LINES  src/modm.f90:277-440
//   line shapes src/modm.f90:567-831, :888-895, :965-1251
//   CONTNM    src/contnm.f90:25-1142 (+ accessors)   XINT/RADFN src/lblrtm_sub.f90
//   TIPS_2003 src/tips_2003.f90:2-298, :4610         ODCLW_TKC src/CloudOptProp.f90:29-157
//   CALCTMR / RTM / RAD_UP_DN  src/RTMmono.f90
//
// Design (DESIGN.md has the full account):
//   * one process = one GPU; a context owns the device line table (44 B per line, SoA);
//   * lines_kernel: workgroup = (profile, layer, tile of wavenumbers, slice of the line list), lane = 1 or 2 wavenumbers.
//     Everything of a line that does not depend on the wavenumber (shifted centre, S~, Lorentz and
//     Doppler widths, coupling factors, pedestal) is prepared ONCE per (layer, line) by one lane,
//     staged in LDS, and then broadcast-read by every wave: the inner loops are one FP64 reciprocal
//     and 7-18 FP64 instructions per (wavenumber, layer, line), chosen per sub-run of lines of one class.
//     The reference recomputes all of it per wavenumber (6 exp, 2 pow, 3 sqrt per evaluation).  On dense
//     grids distant lines enter through per-molecule far-field moments of the tile instead.
//   * finish_kernel: workgroup = (profile, layer); MT_CKD continuum on the 1 cm-1 ABSRB grid in LDS,
//     second interpolation to the wavenumbers, TKC cloud liquid, line-slice sums, totals.
//   * rtm_kernel: workgroup = 64 wavenumbers x G layer groups of a profile; CALCTMR + RAD_UP_DN + RTM recurrences in
//     registers, group sums combined through LDS in the reference's order.
// No MFMA (nothing here is a dense contraction), no Triton, no CUDA compatibility layer.
#pragma once
#include <hip/hip_runtime.h>

// Timing-experiment switches change RESULTS (stages left out, guards removed, series cut short): a build that defines one of
// them must say that it is an experiment (tools/build_variant.sh NAME -DMONORTM_EXPERIMENT=1 -D...), so that none can slip into
// the shipped library through an environment's compiler flags.  __graft_entry__.build() / _build.py define none.
#if (defined(FAR_ABL_HOT) || defined(FAR_ABL_STEPS) || defined(FAR_ABL_TRANS) || defined(MONORTM_ABLATE_LOOP) || defined(MONORTM_ABLATE_EVAL) || \
     defined(MONORTM_ABLATE_VOIGT) || defined(MONORTM_ABLATE_ZSEARCH) || defined(MONORTM_ABLATE_EXP4) || defined(MONORTM_ABLATE_COUPLE) ||     \
     defined(MONORTM_NO_CLAMP_GUARD) || defined(MONORTM_NO_UNIFIED) || defined(MONORTM_NO_VSCAN) ||              \
     defined(MONORTM_NO_HALF) || defined(MONORTM_NO_FULL) || defined(MONORTM_NO_CHUNKFAR) || defined(MONORTM_NO_SGL_TSKIP) || defined(LINES_TIMING) || \
     defined(LINES_CLASS_STATS) || defined(MW_TIMING)) &&                                                                                          \
    !defined(MONORTM_EXPERIMENT)
#error "a timing-experiment / A-B switch of monortm_amd is defined: such builds are measurements, not the product - add -DMONORTM_EXPERIMENT=1"
#endif

#include <cstdint>

#include "../../include/monortm_hip.h"

namespace monortm_dev {

// ------------------------------------------------------------------------------------------------
// constants: the literal decimal strings of the reference as doubles (src/PhysConstants.f90:19-39)
// ------------------------------------------------------------------------------------------------
#define K_PI 3.1415926535898
#define K_PLANCK 6.62606876E-27
#define K_BOLTZ 1.3806503E-16
#define K_CLIGHT 2.99792458E+10
#define K_AVOGAD 6.02214199E+23
#define K_RADCN1 1.191042722E-12
#define K_RADCN2 1.4387752
#define K_ONEPL 1.001
#define K_ONEMI 0.999
#define K_T0 296.0
#define K_P0 1013.25

constexpr int MXMOL = 39;
constexpr int MXBRD = 7;
constexpr int NSCOR = MXMOL * 9;

#ifndef MONORTM_FAR_P
#define MONORTM_FAR_P 56
#endif
constexpr int FAR_P = MONORTM_FAR_P;   // Chebyshev sums of a far field (lines_device.hpp: "Far field of a tile")
#ifndef MONORTM_FAR_KAPPA
#define MONORTM_FAR_KAPPA 1.2          // least distance of a far line in tile half-widths (lines_device.hpp: FAR_KAPPA; modm_plan.hpp: which grids have far lines)
#endif
// ---- the far field of dense grids formed OUTSIDE lines_kernel (far_kernel.hip, round 5) -------------------------------------------
// Intervals of wavenumbers in up to FAR_MAXLEV levels: level 0 = the tiles of lines_kernel (tw wavenumbers each), level l = groups
// of 2^l consecutive tiles.  gi = far_level_offset(l) + j numbers them; the parent of (l, j) is (l + 1, j / 2).
constexpr int FAR_MAXLEV = 6;
constexpr int FAR_GEOM_INTS = 8;            // per (profile, layer, interval, molecule): lowS, lowE, highS, highE, e0, e1s, e1e, unused
constexpr int FAR_SEGS = 5;                 // per (profile, layer, tile, molecule): up to 5 runs of table lines that the tile walks itself
constexpr int FAR_SEG_INTS = 2 * FAR_SEGS;  // (base_k = first line - lines before the run, cum_k = lines up to and including the run)
constexpr int FAR_MOM_STRIDE = FAR_P + 2;   // Chebyshev sums (Clenshaw's convention), sum of the constant pedestals, "anything there" flag
__host__ __device__ inline int far_level_count(int ntile, int l) { return (ntile + (1 << l) - 1) >> l; }
__host__ __device__ inline int far_level_offset(int ntile, int l) {
    int o = 0;
    for (int k = 0; k < l; k++) o += far_level_count(ntile, k);
    return o;
}

// Placement of far_kernel's workgroups (one per interval and molecule): workgroups are dealt round-robin over the 8 XCDs, so
// workgroup x runs on XCD x mod 8.  A molecule gets a share of the XCDs in proportion to its lines (table order), and its
// intervals go round its share: the intervals of a molecule re-read the same records from ONE L2 (or a few), and a molecule
// with a third of the lines does not hold one XCD three times as long as the others (measured: 0.64 ms per level with
// molecule = x mod 8 on a list where one of five molecules has 37 % of the lines).
// mol_start: DevLines::mol_start.  far_xcd_share: XCDs [xlo, xlo + nx) of molecule m (0-based); nx = 0: no lines.
__host__ __device__ inline void far_xcd_share(const int *mol_start, int nmol, int m, int *xlo, int *nx) {
    const long long base = mol_start[1], N = (long long)mol_start[nmol + 1] - base;
    const long long s0 = mol_start[m + 1] - base, s1 = mol_start[m + 2] - base;
    if (N <= 0 || s1 <= s0) { *xlo = 0; *nx = 0; return; }
    const int lo = (int)((16 * s0 + N) / (2 * N)) < 7 ? (int)((16 * s0 + N) / (2 * N)) : 7;
    int hi = (int)((16 * s1 + N) / (2 * N));
    if (hi > 8) hi = 8;
    if (hi < lo + 1) hi = lo + 1;
    *xlo = lo;
    *nx = hi - lo;
}
// the same as a table for one level, formed on the host and passed by value (a workgroup finds its item with scalar compares;
// the divisions of far_xcd_share per molecule and workgroup were a third of a tile-level wave's instructions)
struct FarPlace {
    unsigned char xlo[MXMOL], nx[MXMOL];
    unsigned short cnt[MXMOL][8];   // workgroups of molecule m on XCD k
    double node[64];                // Chebyshev nodes cos(pi (n + 1/2) / FAR_P) of the re-expansion (formed by the host: a cos() per lane
                                    // and workgroup was a tenth of a tile-level workgroup's instructions)
};
// workgroups of molecule m on XCD k at a level of nint intervals: intervals (k - xlo), (k - xlo) + nx, ...
__host__ __device__ inline int far_xcd_items(int nint, int k, int xlo, int nx) {
    if (nx <= 0 || k < xlo || k >= xlo + nx || k - xlo >= nint) return 0;
    return (nint - (k - xlo) + nx - 1) / nx;
}

enum : int { ERRBIT_TEMP = 1, ERRBIT_SDV = 2, ERRBIT_ARG = 4 };  // ARG: nlay[p] outside 1..nlay_max, wn not ascending or a bad path factor (device arrays)

struct DevTables {  // device copies of monortm_tables.h
    const double *self296, *self260, *frgn296, *fco2, *n2c296, *n2sf296, *n2c220, *n2sf220, *xfac_rhu, *xfacco2,
        *tdep_bandhead, *tips_qoft, *tips_q296, *smass;
    // branches above 1340 cm-1
    const double *o3ch_x, *o3ch_y, *o3ch_z, *o3hh0, *o3hh1, *o3hh2, *o3huv, *o2f_x, *o2f_t, *o2inf1, *o2inf3, *o2vis, *o2fuv,
        *n2f_272, *n2f_228, *n2f_ah2o, *n2f1;
    const int *tips_isonm, *tips_offset;
    // log(T-low table / 296 K table) of the three temperature interpolations exp(tfac * log(ratio)) below 820 cm-1 (H2O self,
    // N2 rototranslational and its scale factor): formed once per context by logratio_kernel with the device's own log(),
    // so finish_mw_kernel gets the bits finish_kernel computes in place
    const double *lr_self, *lr_n2c, *lr_n2sf;
};

struct DevLines {
    const double *vnu, *s0adj, *lc;
    const float *alfa, *hwhm, *epp, *tmpalf, *pshift, *sdep, *brd_dat;
    const uint32_t *meta;
    const int32_t *brd_flg;
    int mol_start[MXMOL + 2];
    unsigned long long sorted_mask;
    unsigned long long lc_mask;  // molecules that own at least one line-coupled entry
    double max_abs_shift;
};

struct ModmArgs {
    int nprof, nwn, nlay_max, nmol, ibrd;
    double dvset, sclcpl, sclhw, y0res;
    double cntnm[7];
    // "real" arrays are REAL(real_kind): double (8) or float (4); wavenumbers are always double
    // (the reference keeps WN REAL*8 in both builds, src/modm.f90:139)
    int real_kind;
    const double *wn;
    const void *P, *T, *CLW, *WKL, *WBRODL;
    const int *nlay;
    void *O, *O_BY_MOL, *OC, *O_CLW;
    int *errflag;
    // line slicing (few workgroups otherwise): nslice blocks share one (profile, layer, tile); each writes its
    // partial sums to partial[slice][profile][layer][mol][wn], finish_kernel adds them in slice order
    int nslice;
    void *partial;
    int slices_reduced;  // the slice sums were formed by reduce_slices_kernel (wide grids), not inside finish_kernel
    // nslice == 1: lines_kernel leaves sum_mol O_BY_MOL (as stored, added in molecule order) per (profile, layer, wn) here, so
    // the finish kernel of the microwave range reads nwn values per layer instead of nmol x nwn; null otherwise
    double *osum;
    int fair;       // lines_kernel, one-wave workgroups: waves lower their issue priority as they progress (grids of a few rounds)
    // dense grids: LinePhysM (32 B; + LinePhysY, 16 B, for coupled lines) of every table line for every (profile, layer), formed by physics_kernel before lines_kernel
    // (phys_lines = lines of the table); null: lines_kernel forms them in place, per tile
    void *phys;
    int phys_lines;
    // cross-section molecules (IXSECT = 1): column amounts [profile][layer][nxs] in, their total optical depth
    // [profile][layer][wn] out (xsec_kernel), added into O by the finish kernels; both null otherwise
    const void *XAMNT;
    void *ODXSEC;
    int nxs;
    // dense grids with the physics pass: the far field of every tile formed by far_kernel (far_kernel.hip) before lines_kernel.
    // farmom [profile][layer][interval][molecule][FAR_MOM_STRIDE] Chebyshev sums, fargeom [..][interval][molecule][FAR_GEOM_INTS]
    // the far lines of every interval in index space, farseg [profile][layer][tile][molecule][FAR_SEG_INTS] the runs of table
    // lines that lines_kernel still walks.  All null: lines_kernel forms the far field of a tile itself, chunk by chunk.
    double *farmom;
    int *fargeom, *farseg;
    int far_levels, far_ni, far_tw, far_ntile;   // levels in use, intervals of all levels, wavenumbers per tile, tiles
};

// device copy of the cross-section tables (monortm_hip_xsec_tables): per (molecule, spectral region) a row of
// reg = (molecule, V1FX, V2FX of FSCDXS, points, temperatures, XDOPLR, V1, V2 of the last file header), its temperatures (ascending) and measurement pressures [mbar], and
// the offsets of its spectra in pool
struct DevXsec {
    const double *reg, *temps, *pres, *pool;
    const long long *offs;
    int nxs, nreg;
};

struct RtmArgs {
    int nprof, nwn, nlay_max, iout;
    int real_kind;
    const double *wn;
    const void *T, *TZ, *O, *emiss, *reflc;
    const int *nlay, *irt;
    void *tmpsfc, *RUP, *RDN, *TRTOT, *RAD, *TB, *TMR;
};

// Path scans (rtm_scan_kernel.hip): CALCTMR + RTM along npath paths per profile from ONE set of optical
// depths.  path [nprof][npath][nlay_max]: the factor of every layer's optical depth along the path; emiss, reflc [nprof][nwn]
// (sfc_per_path = 0) or [nprof][npath][nwn] (1); outputs [nprof][npath][nwn].  A factor of an active layer that is negative or
// not finite raises ERRBIT_ARG in errflag.
struct RtmScanArgs {
    int nprof, npath, nwn, nlay_max, iout;
    int real_kind, sfc_per_path;
    const double *wn;
    const void *T, *TZ, *O, *path, *emiss, *reflc;
    const int *nlay, *irt;
    void *tmpsfc, *RUP, *RDN, *TRTOT, *RAD, *TB, *TMR;
    int *errflag;
};

// Jacobians (jacobian_kernel.hip).  The adjoint of RTM: O, T, TZ, surface in; RAD, TB and the derivatives
// of q = RAD (quantity 0) or TB (quantity 1) out - K_O, K_T [nprof][nlay_max][nwn], K_TZ [nprof][nlay_max + 1][nwn], K_SFC [nprof][3][nwn]
// (K_O may be null when FULL).  FULL: K_W [nprof][nlay_max][njac][nwn] and K_CLW from the perturbed states' optical depths Opert:
// state s at Opert + (s - 1) state_stride, s = 1 / 2: T +- dt, 3 + 2i / 4 + 2i: WKL(jac_mol[i]) x (1 +- dlnw).
struct RtmJacArgs {
    int nprof, nwn, nlay_max, quantity, real_kind, njac;
    const double *wn;
    const void *T, *TZ, *O, *tmpsfc, *emiss, *reflc;
    const int *nlay, *irt;
    void *RAD, *TB, *K_O, *K_T, *K_TZ, *K_SFC, *K_W, *K_CLW;
    const void *Opert;
    size_t state_stride;   // elements of one state's O: nprof x nlay_max x nwn
    double dt, dlnw;
};
// Jacobians of path scans (rtm_scan_jac_kernel.hip): the adjoint of RTM along npath paths per profile from ONE
// set of optical depths; path, emiss, reflc, sfc_per_path and errflag as RtmScanArgs, the others as RtmJacArgs with a path axis behind
// the profile's: RAD, TB [nprof][npath][nwn], K_O (= factor x dq/dtau, may be null), K_PATH (= O x dq/dtau, may be null), K_T, K_CLW
// [nprof][npath][nlay_max][nwn], K_TZ [nprof][npath][nlay_max + 1][nwn], K_SFC [nprof][npath][3][nwn], K_W [nprof][npath][nlay_max][njac][nwn].
struct RtmScanJacArgs {
    int nprof, npath, nwn, nlay_max, quantity, real_kind, njac, sfc_per_path;
    const double *wn;
    const void *T, *TZ, *O, *path, *tmpsfc, *emiss, *reflc;
    const int *nlay, *irt;
    void *RAD, *TB, *K_O, *K_PATH, *K_T, *K_TZ, *K_SFC, *K_W, *K_CLW;
    const void *Opert;
    size_t state_stride;   // elements of one state's O: nprof x nlay_max x nwn
    double dt, dlnw;
    int *errflag;
};
// Channel- and beam-averaged Jacobians of path scans (rtm_obs_jac_kernel.hip): the inputs of RtmScanJacArgs and the
// device tables of a measurement operator (monortm_hip_obs_create, checked on the host): view_start [nview + 1] (the paths of view v are
// view_start[v] .. view_start[v + 1] - 1), wpath [npath]; per block b of 64 wavenumbers the members of every channel, ascending in
// wavenumber: mstart [nblk][nchan + 1] into mlane (lane of the member within its block) and mw (its wchan).  Outputs Y [nprof][nview][nchan],
// K_T, K_CLW [nprof][nview][nlay_max][nchan], K_TZ [nprof][nview][nlay_max + 1][nchan], K_SFC [nprof][nview][3][nchan],
// K_W [nprof][nview][nlay_max][njac][nchan].
struct RtmObsJacArgs {
    int nprof, npath, nwn, nlay_max, quantity, real_kind, njac, sfc_per_path, nview, nchan;
    const double *wn;
    const void *T, *TZ, *O, *path, *tmpsfc, *emiss, *reflc;
    const int *nlay, *irt;
    const int *view_start, *mstart, *mlane;
    const double *wpath, *mw;
    void *Y, *K_T, *K_TZ, *K_SFC, *K_W, *K_CLW;
    const void *Opert;
    size_t state_stride;   // elements of one state's O: nprof x nlay_max x nwn
    double dt, dlnw;
    int *errflag;
};
// The forward measurement operator (rtm_obs_kernel.hip): the inputs of RtmScanArgs (tmpsfc: input only) and the
// device tables of a measurement operator as in RtmObsJacArgs; quantity 0 / 1: q = RAD / TB, 2: the band brightness temperature - RAD
// is contracted and the finished element converted at the channel's nominal wavenumber vcen [nchan] (read for quantity 2 only; a value
// that is not finite and > 0 raises ERRBIT_ARG).  Output Y [nprof][nview][nchan].
struct RtmObsArgs {
    int nprof, npath, nwn, nlay_max, quantity, real_kind, sfc_per_path, nview, nchan;
    const double *wn;
    const void *T, *TZ, *O, *path, *tmpsfc, *emiss, *reflc;
    const int *nlay, *irt;
    const int *view_start, *mstart, *mlane;
    const double *wpath, *mw, *vcen;
    void *Y;
    int *errflag;
};
// the MODM inputs of the base (state 0) and the perturbed states, [nstate][nprof][nlay_max](x nmol), real_kind 8
struct JacPerturbArgs {
    int nstate, nprof, nlay_max, nmol;
    double dt, dlnw;
    int jac_mol[MXMOL];   // what states 3 + 2i / 4 + 2i scale: a 1-based molecule's WKL, or MONORTM_JVAR_P / _WBROD
    int rayl_state;       // the state (the last one) that holds the inputs of Rayleigh alone - WKL = 0, WBRODL = WTOT, CLW = 0 -, or 0: none
    const double *P, *T, *CLW, *WKL, *WBRODL;
    const int *nlay;
    double *xP, *xT, *xCLW, *xWKL, *xWBRODL;
    int *xnlay;
};

// The cross-section molecules in a full Jacobian call (xsec_jac_kernel.hip), real_kind 8: ODXSEC of nx further
// states - 2: T +- h, 4: and P (1 +- eps) - summed on the base state's plan, and the named molecules' own terms.  The base state is
// the caller's P, T, XAMNT [nprof][nlay_max](x nxs); further state s reads its (P', T') from state pstate[s] of the perturbed arrays
// xP, xT [state][nprof][nlay_max] (jac_perturb_kernel) and writes slot oslot[s] of ODX [slot][nprof][nlay_max][nwn].  kplus[x] != 0:
// molecule x (0-based position in the cross-section request) is a Jacobian variable, and state kplus[x] of xO (state k at xO + k
// stride, stride = nprof x nlay_max x nwn) gets two_eps XAMNT sigma_x radfn of the base state.
struct XsecJacArgs {
    int nprof, nwn, nlay_max, nx;
    const double *wn, *P, *T, *XAMNT;
    const int *nlay;
    const double *xP, *xT;
    int pstate[4], oslot[4];
    double *ODX, *xO;
    size_t stride;
    int kplus[38];
    double two_eps;
};

// The optimal-estimation step (oe_kernel.hip), real_kind 8.  K[kind] are the K_T, K_TZ, K_W, K_CLW, K_SFC of
// monortm_hip_obs_jacobian, [nprof][nview][rows][nchan]: kstride = nview x rows x nchan elements per profile, vstride = rows x nchan per
// view.  map [2][nstate] on the device: the kind of state s, then state_row[s] x nchan - both checked on the host.  Sa [nstate][nstate]
// (x nprof with sa_per_profile), lower triangle read; se [nmeas] (x nprof with se_per_profile); gamma [nprof] or null.  ws: the
// workspace, [nprof][2][nmeas][nstate] doubles.  post_var, avk_diag, chi2 may be null.
// The full entries (section 3.14): se_kind 1 - se is Se [nmeas][nmeas] (x nprof with se_per_profile), lower triangle read; gain_t
// [nprof][nmeas][nstate] and dofs [nprof] may be null (dofs is summed from avk_diag, which is not null then).  After the launch the
// workspace holds b = L^-1 K and a = L^-1 W^T of every profile of status 0: what oe_cov_kernel reads.
struct OeArgs {
    int nprof, nview, nchan, nmeas, nstate, sa_per_profile, se_per_profile;
    const double *K[5];
    size_t kstride[5];
    int vstride[5];
    const int *map;
    const double *Y, *y_obs, *x, *xa, *Sa, *se, *gamma;
    double *x_new, *post_var, *avk_diag, *chi2;
    int *status;
    double *ws;
    int se_kind;
    double *gain_t, *dofs;
    // the LM entries (section 3.15): any of the three not null selects the DUAL instantiations.  c [nprof][nstate] or null (0), the
    // dual vector Sa^-1 (x - xa) of the iterate; c_new [nprof][nstate] (not c itself) and cost [nprof] may be null
    const double *c;
    double *c_new, *cost;
};

// oe_scatter_kernel (section 3.15): a state vector written into the resident arrays through a write map on the device, [3][nstate]
// ints: kind (0 T, 1 TZ, 2 WKL, 3 CLW, 4 TMPSFC, -1 checked but not written), index (layer or level; a column of kind -1 is live where
// index < nlay[p]: the host stores level - 1 for a level and -1 for TMPSFC), mol (0-based, WKL only).  All of it is checked on the host:
// index < the rows of its array, mol < nmol, no two written columns with the same target.  Strides are elements per profile; WKL is
// [nprof][..][nmol].  lo, hi [nstate] (x nprof with box_per_profile) or null; x_fallback, done, trial_ok, tmpsfc_a / _b may be null.
struct OeScatterArgs {
    int nprof, nstate, nmol, box_per_profile;
    const int *wmap, *nlay, *done;
    const double *x_src, *x_fallback, *lo, *hi;
    double *T, *TZ, *WKL, *CLW, *tmpsfc_a, *tmpsfc_b;
    size_t t_stride, tz_stride, wkl_stride, clw_stride;
    int *trial_ok;
};

// oe_accept_kernel (section 3.15): the decision on a trial step, per profile.  Y_trial, y_obs [nprof][nmeas]; se as in OeArgs (se_kind,
// se_per_profile); x_trial, c_trial, xa [nprof][nstate]; the loop state x_cur, c_cur [nprof][nstate], J_cur, gamma [nprof] and done,
// n_acc, n_rej int [nprof] are updated in place.
struct OeAcceptArgs {
    int nprof, nmeas, nstate, se_kind, se_per_profile, last;
    const double *Y_trial, *y_obs, *se, *x_trial, *c_trial, *xa;
    const int *step_status, *trial_ok;
    double up, down, gamma_first, gamma_floor, gamma_max, conv;
    double *x_cur, *c_cur, *J_cur, *gamma;
    int *done, *n_acc, *n_rej;
};

// oe_cov_kernel: avk = a^T b and post_cov = g Sa - a^T a, [nprof][nstate][nstate] each (one of them may be null), from the workspace
// and the status the step kernel left on the same stream.
struct OeCovArgs {
    int nprof, nmeas, nstate, sa_per_profile;
    const double *ws, *Sa, *gamma;
    const int *status;
    double *avk, *post_cov;
};

// exp() and 1/x for the small kernels behind the line sum (radiance recurrences, microwave continuum): Cody-Waite reduction +
// degree-13 polynomial (the routine of the line kernel's prepare stage: 20 instructions, 1-2 ulp like the library call at ~35)
// and v_rcp_f64 + two Newton steps (1 ulp; an IEEE division is ~11 instructions).  exp_cw: |n| < 2^31 for every argument that
// occurs (optical depths, hc v / kT); ldexp saturates to 0 / +inf beyond the exponent range; fmax keeps the conversion defined
// for a NaN argument - the polynomial is NaN then, and so is the result.
__device__ __forceinline__ double exp_cw(double x) {
    const double n = rint(x * 1.44269504088896338700e+00);
    double r = fma(-n, 6.93147180369123816490e-01, x);
    r = fma(-n, 1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)fmax(n, -2200.));
}
__device__ __forceinline__ double rcp2(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    return fma(fma(-x, r, 1.0), r, r);
}

// Planck function bb_fn (RTMmono.f90:223-237) with v^3 RADCN1 = c3 formed once per wavenumber
__device__ __forceinline__ double planck(double c3, double v, double fbeta) {
    const double e = exp_cw(v * fbeta) - 1.;
    return (e == __builtin_inf()) ? 0. : c3 * rcp2(e);
}
// B(T) and dB/dT from the same exp_cw(x) - 1 as planck(): x = hc v / kT = v fbeta, fbeta = RADCN2 / T,
// dB/dT = B (e + 1) / e x / T = B (e + 1) / e v fbeta^2 / RADCN2
__device__ __forceinline__ void planck_d(double c3, double v, double fbeta, double *B, double *dB) {
    const double e = exp_cw(v * fbeta) - 1.;
    if (e == __builtin_inf()) { *B = 0.; *dB = 0.; return; }
    const double r = rcp2(e), b = c3 * r;
    *B = b;
    *dB = b * ((e + 1.) * r) * (v * fbeta * fbeta * (1. / K_RADCN2));
}
// ---- the arithmetic every radiance kernel shares -------------------------------------------------------------------------------------
// rtm_layer_terms: rtm_kernel (rtm_kernel.hip), rtm_jac_kernel's pass 1 (jacobian_kernel.hip) and tile_forward_sweep (rtm_tile.hpp), which
// is the forward sweep of rtm_scan_kernel, rtm_obs_kernel, rtm_scan_jac_kernel and rtm_obs_jac_kernel.  bb_fn and rtm_combine: rtm_kernel,
// rtm_scan_kernel, rtm_obs_kernel.
// A scan path with factor 1 is monortm_hip_rtm's result bit for bit (tests/test_rtm_extremes.py).  Left to the compiler, which
// products fuse into which sums depends on the surrounding code (scalars in one kernel, per-path arrays in the other) - RAD came out
// one ulp apart.  So the kernels call these, every product-sum is spelled out as an fma or a separately rounded product, and
// contraction is off inside them.
// Planck function with the library exp, as RTM's surface and cosmic terms (RTMmono.f90:223-237)
__device__ __forceinline__ double bb_fn(double v, double fbeta) {
#pragma clang fp contract(off)
    return K_RADCN1 * (v * v * v) / (exp(v * fbeta) - 1.);
}
// One layer's terms of RAD_UP_DN (RTMmono.f90:193-217) and CALCTMR (:302-315): ODVI the layer's optical depth, bb / bbz / bb_top the
// Planck function of the layer, its lower and its upper level; ODTd (the optical depth up to and including the layer) and ODTu
// (above the layer) are advanced to the layer below
__device__ __forceinline__ void rtm_layer_terms(double ODVI, double bb, double bbz, double bb_top, bool up, double &ODTd, double &ODTu,
                                                double &RUP, double &RDN, double &sumexp) {
#pragma clang fp contract(off)
    const double TRI = exp_cw(-ODVI);
    const double pade = fma(0.013, ODVI * ODVI, 0.193 * ODVI);
    const double rp1 = rcp2(1. + pade), emis = 1. - TRI;
    ODTd = ODTd - ODVI;
    const double TRd = exp_cw(-ODTd);
    const double bnum = fma(pade, bbz, bb);
    RDN = fma((TRd * emis) * bnum, rp1, RDN);        // TR (1 - TRI) (bb + pade bba) / (1 + pade), RTMmono.f90:216
    sumexp = fma((bnum * rp1) * TRd, emis, sumexp);  // beff TR (1 - TRI), RTMmono.f90:312-313
    if (up) {
        const double TRu = exp_cw(-ODTu);
        RUP = fma((TRu * emis) * fma(pade, bb_top, bb), rp1, RUP);  // RTMmono.f90:203
        ODTu = ODTu + ODVI;
    }
}
// RTM's combination of the sweeps (RTMmono.f90:138-147), TB and CALCTMR's mean radiating temperature (:316-321); TB and TMR only
// where the caller stores them (want_tb, want_tmr; 0 otherwise)
__device__ __forceinline__ void rtm_combine(int irt, double VV, double RUP, double RDN, double sumexp, double ODTOT, double ESFC, double RSFC,
                                            double SURFRAD, double COSMOS, bool want_tb, bool want_tmr, double &TRTOT, double &RAD,
                                            double &TB, double &TMR) {
#pragma clang fp contract(off)
    const double c3 = K_RADCN1 * (VV * VV * VV);
    TRTOT = exp(-ODTOT);
    TMR = 0.;
    if (want_tmr) {
        const double radtmr = sumexp / (1. - exp(-1 * ODTOT));
        TMR = K_RADCN2 * VV / log(c3 / radtmr + 1.);
    }
    const double sky = fma(TRTOT, COSMOS, RDN);
    RAD = 0.;
    if (irt == 1) RAD = fma(TRTOT, fma(RSFC, sky, ESFC * SURFRAD), RUP);
    if (irt == 2) RAD = fma(TRTOT, sky, RUP);
    if (irt == 3) RAD = sky;
    TB = want_tb ? K_RADCN2 * VV / log(c3 / RAD + 1.) : 0.;
}
// Doppler half width per unit wavenumber, HALFWHM_D / XNU (modm.f90:442-454) for an isotopologue of mass M [g/mol]
__device__ __forceinline__ double doppler_factor(double M, double T) {
    return sqrt(2. * log(2.) * ((K_BOLTZ * T) / (M / K_AVOGAD))) / K_CLIGHT;
}

template <typename R>
__host__ __device__ inline const R *rp(const void *p) { return static_cast<const R *>(p); }
template <typename R>
__host__ __device__ inline R *wp(void *p) { return static_cast<R *>(p); }

// ---- lines_ms_kernel (round 6): G states per one-wave workgroup, MS_WPS wavenumbers per lane (lines_ms_kernel.hip) -------------------
#define MS_WPS 5
#define MS_MAXSTEPS 4
constexpr int MS_HOTA_BYTES = 32;   // sizeof(HotA) (lineshape.hpp; asserted in lines_ms_kernel.hip): the host sizes the wave's LDS with it (modm_plan.hpp)
struct MsArgs {
    int G, LPS, CL, nsteps;   // states per wave, lanes per state, lines per chunk, prepare passes (ceil(G / spp))
    int spp;                  // states per prepare pass (64 / CL): lane = sub CL + l serves line l of state t spp + sub in pass t
    int sa_stride;            // HotA records per state in LDS (CL + 2: the class loops read two records ahead)
    int npg;                  // groups of G profiles (ceil(nprof / G)); grid = npg x nlay_max
    int nslot;                // (molecule, isotopologue) pairs of the line table: slot_base[m] + iso - 1
    int inv_cl;               // ceil(65536 / CL): lane / CL = (lane * inv_cl) >> 16 for lane < 64
    int inv_lps;              // ceil(65536 / LPS): lane / LPS likewise
    const int *slot_base;     // [nmol + 1] on the device
    void *scratch;            // per workgroup G x CL x (HotB + ColdLine): the records of the rare shapes of a chunk
    unsigned short *reach;    // [lines of the table] slots of channels each line / its negative resonance can reach (ms_reach_kernel, once per launch)
    float *near0;             // [lines of the table] distance of the table centre to the nearest channel, rounded down (ms_reach_kernel)
    int ablate;               // MONORTM_EXPERIMENT builds only (option ms_ablate; wrong results): 1 = prologue only, 2 = no evaluate stage, 3-5 parts of it,
                              // 6 = as 2 without the prepare stage's tail for the chunks a trip finished
    int prepare;              // option ms_prepare: MS_PREPARE_FUSED (= auto: one trip per plain chunk of two or three passes) / MS_PREPARE_PASSES (the pass loop always)
    int plan_on;              // option ms_plan: 1 = waves that match the launch-wide chunk plan take their windows and chunk words from it
    unsigned long long *plan; // the chunk plan, written once per launch by the plan blocks of ms_reach_kernel's grid (layout: MS_PLAN_* below)
};
#define MS_PREPARE_FUSED 0
#define MS_PREPARE_PASSES 1
// the chunk plan in 64-bit words.  Head: the ints lo[MXMOL] (first candidate line per molecule, 0x7fffffff: none) and off[MXMOL + 1]
// (prefix sums of the counts, off[nmol] = total) for states with RHORAT <= 1, then four counters of MONORTM_EXPERIMENT builds (waves,
// waves that match, chunks, chunks on the fast path).  Per chunk of CL candidates MS_PLAN_CHUNK words: [0] bit 0 = no coupled line / width
// or shift conversion in the chunk, bit 1 = a molecule beyond MXBRD; [2 + k] the lines that reach slot k, [2 + MS_WPS + k] those whose
// negative resonance does (the words of ms_prepare's tail for a chunk without a rare shape in a wave that is not dense)
constexpr int MS_PLAN_OFF = MXMOL;                     // (int index of off[0])
constexpr int MS_PLAN_CNT = (2 * MXMOL + 1 + 1) / 2;   // (word index of the counters)
constexpr int MS_PLAN_HEAD = MS_PLAN_CNT + 4;
constexpr int MS_PLAN_CHUNK = 2 + 2 * MS_WPS;
inline size_t lines_ms_plan_words(long long nlines, int CL) { return (size_t)MS_PLAN_HEAD + (size_t)MS_PLAN_CHUNK * (size_t)((nlines + CL - 1) / CL); }
size_t lines_ms_scratch(const MsArgs &ms, long long nwg);
void launch_lines_ms(const ModmArgs &a, const DevLines &L, const DevTables &tb, const MsArgs &ms, bool ibrd, hipStream_t s);

// ---- launchers: one translation unit per kernel family -------------------------------------------------------
// lines_kernel.hip: block = nw waves, lane = wpl wavenumbers (tile = wpl * nw * 64), as chosen by lines_config() (modm_plan.hpp);
// ibrd selects the species-broadening instantiation
void launch_physics(const ModmArgs &a, const DevLines &L, const DevTables &tb, int nlines, bool ibrd, hipStream_t s);
// far_kernel.hip: far_plan_kernel (which lines are far for which interval; independent of physics_kernel), then far_kernel per level,
// top level first (reads the plan and physics_kernel's records)
void launch_far_plan(const ModmArgs &a, const DevLines &L, const DevTables &tb, hipStream_t s);
void launch_far(const ModmArgs &a, const DevLines &L, const DevTables &tb, double rho_tile, double lines_per_cm, long long *launches,
                hipStream_t s);   // launches[4]: += 1 per level at the entry of its waves per workgroup (1, 2, 4, 8)
void launch_lines(const ModmArgs &a, const DevLines &L, const DevTables &tb, int nw, int wpl, bool ibrd, dim3 grid, size_t dyn_lds,
                  hipStream_t s);
// continuum_kernel.hip: high = spectral range reaches above 1340 cm-1; par = passes side by side in the waves of a
// 256-thread workgroup (small grids below 1340 cm-1; lds holds 4 sets of grids); threads = 64 with lds_sets = 4: four layers
// per one-wave workgroup (large microwave batches)
hipError_t launch_finish(const ModmArgs &a, const DevTables &tb, double V1ABS, double V2ABS, int NPTABS, int csize, bool high,
                         bool par, int threads, size_t lds, int lds_sets, hipStream_t s);
void launch_reduce_slices(const ModmArgs &a, hipStream_t s);
// spectral ranges that end below 820 cm-1: the continuum passes side by side in three stages (finish_mw_kernel)
void launch_logratio(const double *t296, const double *tlow, double *out, int n, hipStream_t s);
// per context: the spectral-range constants of finish_mw_kernel's stages A and B (continuum_kernel.hip: MwItemA / MwItemB)
struct MwCache {
    // one entry per spectral range seen by the context (a caller that alternates between two channel sets keeps both; round 4
    // held a single slot and re-built it - with a device-wide synchronisation - at every change).  The items of an entry are
    // built by a kernel on the stream of the call that first needs them; later calls on the same stream are ordered behind it
    // by the stream, calls on another stream wait for `built` once.
    struct Entry {
        double key[5];       // V1, V2, V1ABS, V2ABS, NPTABS
        void *items;
        hipEvent_t built;
        hipStream_t stream;  // the stream that built the items
        bool ready;          // `built` was seen complete: no stream has to wait any more
        unsigned long long last_use;
    };
    static constexpr int kMax = 8;
    Entry e[kMax];
    int n = 0;
    unsigned long long clock = 0;
    const char *why = nullptr;  // reason of the last failure, where hipGetErrorString would not say it
    void release();             // frees every entry (context teardown; the device is idle)
};
// layout_opt: option "finish_mw" (finish_mw_layout.hpp); cus: compute units; *column: the column layout served the call
hipError_t launch_finish_mw(const ModmArgs &a, const DevTables &tb, double V1, double V2, double V1ABS, double V2ABS, int NPTABS, MwCache &cache,
                            int layout_opt, int cus, bool *column, hipStream_t s);
// known-answer hook: device versions of W4, SD_Humlicek, SDVOIGT, RADFN, AtoB, ODCLW_TKC, TIPS scor (continuum_kernel.hip)
void launch_kat(int which, int n, const double *in, const double *tab, double *out, int *errflag, const DevTables &tb, hipStream_t s);
// xsec_kernel.hip: MONORTM_XSEC_SUB + convolve (src/monortm_sub.F90:1540-1834) -> a.ODXSEC
void launch_xsec(const ModmArgs &a, const DevXsec &x, hipStream_t s);
// xsec_jac_kernel.hip: the same walk with further states on the base state's plan -> a.ODX, a.xO
void launch_xsec_jac(const XsecJacArgs &a, const DevXsec &x, hipStream_t s);
// rtm_kernel.hip
void launch_rtm(const RtmArgs &a, hipStream_t s);
// rtm_scan_kernel.hip
void launch_rtm_scan(const RtmScanArgs &a, hipStream_t s);
// jacobian_kernel.hip (full = FULL instantiation, real_kind 8)
void launch_jac_perturb(const JacPerturbArgs &a, hipStream_t s);
void launch_rtm_jac(const RtmJacArgs &a, bool full, hipStream_t s);
// rtm_scan_jac_kernel.hip (full = FULL instantiation, real_kind 8)
void launch_rtm_scan_jac(const RtmScanJacArgs &a, bool full, hipStream_t s);
// rtm_obs_jac_kernel.hip (full = FULL instantiation, real_kind 8; out_kind: element size of the outputs - 8 with a.real_kind = 4 is the
// host entry's double accumulation)
void launch_rtm_obs_jac(const RtmObsJacArgs &a, bool full, int out_kind, hipStream_t s);
// rtm_obs_kernel.hip (out_kind as for launch_rtm_obs_jac)
void launch_rtm_obs(const RtmObsArgs &a, int out_kind, hipStream_t s);
// oe_kernel.hip: one launch, one workgroup per profile; raises the kernel's bound on dynamic LDS where nmeas needs it
// (se_kind 1 and a gain_t select the kernel's other instantiations; neither: the one launch of monortm_hip_oe_step)
hipError_t launch_oe_step(const OeArgs &a, hipStream_t s);
// oe_kernel.hip: grid (output tiles, profiles); no launch when both matrices are null
hipError_t launch_oe_cov(const OeCovArgs &a, hipStream_t s);
// oe_kernel.hip: one launch each, one workgroup per profile (the accept kernel raises its bound on dynamic LDS like the step)
hipError_t launch_oe_scatter(const OeScatterArgs &a, hipStream_t s);
hipError_t launch_oe_accept(const OeAcceptArgs &a, hipStream_t s);

}  // namespace monortm_dev
