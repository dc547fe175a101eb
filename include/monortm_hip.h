/* monortm_hip.h - C ABI of the MI355X-native MODM / CALCTMR / RTM hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI layer: its boundary is the Fortran
 * module-procedure interface used by PROGRAM MONORTM
 *     CALL MODM(...)     reference src/monortm.f90:557-561  ->  src/modm.f90:21-25
 *     CALL CALCTMR(...)  reference src/monortm.f90:567      ->  src/RTMmono.f90:239
 *     CALL RTM(...)      reference src/monortm.f90:573-574  ->  src/RTMmono.f90:13-14
 * and module procedures are compiler-mangled with compiler-specific array descriptors, so the
 * replacement is source level: monortm_amd/fortran/{modm_hip,rtmmono_hip}.f90 define modules
 * ModmMod / RTMmono with the reference's public names and argument lists and forward to the
 * entry points below through ISO_C_BINDING (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain C types, caller-owned contiguous buffers, no library types in any signature;
 *   - every function returns 0 on success, a MONORTM_E* code otherwise; the text of the last
 *     error is available from monortm_hip_last_error() (the reference has no status codes: every
 *     failure is a Fortran STOP; the Fortran shim turns a non-zero status into STOP);
 *   - arrays are C-ordered with the WAVENUMBER AXIS FASTEST, i.e. element (wn m, layer k) of the
 *     reference's O(m,k) is O[k*nwn + m]; a batch adds a leading profile axis;
 *   - monortm_real arrays hold the caller's default REAL: real_kind = 8 (IEEE double, the reference's "dbl" build:
 *     default REAL = 8 bytes, build/makefile.common:195-198) or real_kind = 4 (float, the "sgl" build).  The kind is
 *     fixed per context at init; wavenumbers are REAL*8 in both builds (src/modm.f90:139) and so are the scalars
 *     passed by value here.  With real_kind = 4 the Lorentz line sum is evaluated in float (one v_rcp_f32 per
 *     line), the per-(layer, line) preparation, the coupled / Voigt shapes, the continuum and the radiance
 *     recurrences in double with float loads / stores;
 *   - one context = one loaded TAPE3 on one GPU (monortm_hip_init) or on several (monortm_hip_init_multi); calls on a
 *     context are serialised by the caller
 *     (the reference's MODM is non-reentrant: SAVE / COMMON state, src/modm.f90:161-163).
 *   - the *_dev entry points take DEVICE pointers and a hipStream_t (as void*): inputs stay resident
 *     in HBM, nothing is copied, the call is asynchronous on that stream.
 */
#ifndef MONORTM_HIP_H
#define MONORTM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    MONORTM_OK = 0,
    MONORTM_EIO = 1,          /* TAPE3 missing / unreadable      (reference: lnfl_mod.f90:131-132 STOP) */
    MONORTM_EFORMAT = 2,      /* TAPE3 malformed / no isotope tag (reference: lnfl_mod.f90:297-302 STOP) */
    MONORTM_EUNSUPPORTED = 3, /* option outside the entry point called (IXSECT=1 through monortm_hip_modm: use _modm_xs; real_kind not 4 / 8) */
    MONORTM_ETEMP = 4,        /* layer temperature outside 70-3000 K (reference: tips_2003.f90:277 STOP) */
    MONORTM_ESDV = 5,         /* speed-dependent Voigt gave Re(v)<0 (reference: modm.f90:1062 STOP) */
    MONORTM_EARG = 6,         /* bad argument */
    MONORTM_EHIP = 7          /* HIP runtime error */
};

typedef void monortm_real; /* element type selected by real_kind: double or float */

#define MONORTM_NCONT 5 /* continuum slots returned in OC: molecules 1,2,3,7,22 (index_cont, modm.f90:166) */

/* Replaces the once-per-process GET_LNFL(IPR,ICP,HFILE,v1,v2) inside MODM (src/modm.f90:187-190,
 * src/lnfl_mod.f90:22-133): parses TAPE3 on the host with the reference's block skip / stop rules for
 * [v1-25, v2+25], builds the device line table.  device = HIP device ordinal (or -1: current). */
int monortm_hip_init(const char *tape3_path, double v1, double v2, int icp, int real_kind, int device, void **ctx);

/* The same for ngpu devices of this node (ngpu <= 0: every visible device): one line table, stream and set of staging
 * arenas per device.  monortm_hip_modm / monortm_hip_rtm on such a context shard the batch into contiguous blocks of
 * ceil(nprof / ngpu) profiles - the reference's only parallel axis, the independent-profile loop of src/monortm.f90:357 -
 * enqueue every device's block before waiting for the first, and each block comes back over its own device's PCIe link
 * straight into the caller's arrays (results are bit-identical to a one-device context: profiles do not interact).
 * The *_dev, profiling and check entry points need a one-device context.  MONORTM_DEVICES="0,1,.." overrides the device
 * list (an ordinal may repeat, which exercises the sharding on a one-GPU box). */
int monortm_hip_init_multi(const char *tape3_path, double v1, double v2, int icp, int real_kind, int ngpu, void **ctx);

int monortm_hip_device_count(void *ctx); /* devices (shards) behind a context: 1 for monortm_hip_init */

/* One process per GPU: the single gather of a profile-sharded job over RCCL / xGMI.
 * Reference axis: the independent-profile loop of src/monortm.f90:357 (the reference itself is serial and has no such step);
 * every rank runs monortm_hip_modm_dev / _rtm_dev on its contiguous block of ceil(P / G) profiles, then ONE gather of the
 * device-resident outputs to `root` - the call the Python layer makes through torch.distributed (monortm_amd/distributed.py),
 * here for C / Fortran callers.  RCCL is loaded on first use (dlopen), never by single-GPU callers.
 *   monortm_hip_comm_unique_id : rank 0 fills the 128-byte id (ncclGetUniqueId); the caller hands it to every rank (MPI, a file)
 *   monortm_hip_comm_init      : ncclCommInitRank on the context's device; collective over the `world` ranks
 *   monortm_hip_gather_dev     : `bytes` bytes from every rank's `send` (device) into recv[rank * bytes ..] on `root` (device;
 *                                may be NULL elsewhere), asynchronous on `stream` (ncclGather)
 * Errors: MONORTM_EHIP with the RCCL message in monortm_hip_last_error. */
int monortm_hip_comm_unique_id(void *id128);
int monortm_hip_comm_init(void *ctx, int world, int rank, const void *id128);
int monortm_hip_gather_dev(void *ctx, const void *send, size_t bytes, void *recv, int root, void *stream);

void monortm_hip_finalize(void *ctx);

const char *monortm_hip_last_error(void *ctx); /* ctx may be NULL: error of the last failed init */

/* Host-only (no GPU needed): parse TAPE3 exactly as monortm_hip_init would and report, per molecule m = 1..39
 * (index 0 = all): physical line records kept (IFLG >= 0), table entries (records the LINES walk treats as a
 * line) and entries that carry line-coupling coefficients.  Each array has 40 elements. */
int monortm_hip_tape3_probe(const char *tape3_path, double v1, double v2, long long *n_physical, long long *n_entries,
                            long long *n_coupled);

/* 1 when the context holds a line table (a TAPE3 path was given at init), else 0.  A context created with an empty
 * path serves CALCTMR / RTM only; MODM on it returns MONORTM_EARG (the reference always loads the line file on its
 * first MODM call: INIT flag, src/modm.f90:187-190). */
int monortm_hip_has_lines(void *ctx);

/* Number of cross-section regions the context holds (monortm_hip_xsec_tables), 0 before the first upload.  The Fortran
 * shim uses it to skip the per-profile re-upload that would mirror the reference's per-call re-read of the xs files
 * (src/monortm_sub.F90:1659-1673) when neither the context nor the /XSECTR/, /XSECTF/ entries have changed. */
int monortm_hip_xsec_regions(void *ctx);

/* Known-answer hook for the parity tests: evaluates ONE of the small device functions of the path for n argument sets on
 * the GPU.  args[n][4] in, out[n][2].  which: 1 W4(x,y) -> re,im (src/modm.f90:1100)  2 SD_Humlicek(x1,y1,x2,y2) -> re,im
 * (:1150)  3 SDVOIGT(deltnu,alphal,alphad,sdep) (:965)  4 RADFN(vi,xkt) (src/lblrtm_sub.f90:36)  5 AtoB(aa) on the TIPS
 * temperature grid with the 119-point table tab119 (src/tips_2003.f90:4610)  6 ODCLW_TKC(wn,temp,clw)
 * (src/CloudOptProp.f90:29)  7 scor(mol,iso) of TIPS_2003(39,T,scor) for args (T, mol, iso) (src/tips_2003.f90:2-298; out[.][1] = 1
 * where the reference would STOP, 0 where it leaves scor untouched)  8 HALFWHM_D(mol,iso,xnu,T) (src/modm.f90:442)
 * 9 bb_fn(v,fbeta) (src/RTMmono.f90:223) as the radiance kernels form it  10 exp_cw(x) and 11 rcp2(x), the exp() and 1 / x
 * of the radiance kernels (device_common.hpp), for their ulp bounds.  Returns MONORTM_ESDV when SDVOIGT meets the
 * reference's STOP condition. */
int monortm_hip_kat(void *ctx, int which, int n, const double *args, const double *tab119, double *out);

/* Diagnostics: which = 0 -> number of monortm_hip_rtm calls on this context that found the optical depths O of the
 * preceding monortm_hip_modm call still resident on the device (the caller handed back exactly what MODM returned, as
 * PROGRAM MONORTM does at src/monortm.f90:567-574) and skipped the upload.  which = 1 -> the same count for monortm_hip_rtm_scan.
 * which = 2 .. 7 -> launches of the continuum / cloud / total kernel of MODM on this context by variant, one per MODM evaluation
 * (a Jacobian call makes several): 2 finish_mw_kernel (last wavenumber < 820 cm-1 and an ABSRB grid of <= 1000 points), 3
 * finish_kernel<HIGH> (last wavenumber > 1340 cm-1), 4 finish_kernel<PAR> (fewer than 16 x compute units (profile, layer) workgroups),
 * 5 finish_kernel<Q4> (four layers per wave: ABSRB grid <= 64 points, <= 128 wavenumbers), 6 finish_kernel with 64 threads (ABSRB
 * grid <= 256 points, <= 128 wavenumbers), 7 finish_kernel with 256 threads.  which = 9 -> those launches of variant 2 that took the
 * column layout (finish_mw_kernel_col, option "finish_mw").  which = 16 .. 19 -> launches of far_kernel (the far field
 * of dense grids, one launch per level of intervals and MODM evaluation) with 1, 2, 4, 8 waves per workgroup; 8 and 10 .. 15 are unknown.
 * Counted on the host next to the launch; tests use them to know which variant served a call.  A multi-device context returns the
 * sum over its devices.  -1 for an unknown selector / NULL. */
long long monortm_hip_counter(void *ctx, int which);

/* Physical line records (IFLG >= 0) held for molecule mol (1..39); mol = 0 -> all molecules.
 * This is NBLM(mol) minus the coupling records (src/lnfl_mod.f90:66) and is what the
 * (wavenumber x layer x line) evaluation count of BASELINE.json is made of. */
long long monortm_hip_line_count(void *ctx, int mol);

/* MODM, host buffers (what the Fortran shim calls).  Replaces src/modm.f90:21-274.
 *   wn[nwn] ascending cm-1;  dvset: COMMON /MANE/ DVSET of the caller (0 => explicit channels; /= 0 promises wn[i] = wn[0] + i dvset,
 *   which the continuum interpolation relies on as the reference's does - a grid that breaks it is MONORTM_EARG);
 *   nlay[nprof] layers per profile (<= nlay_max);  nmol molecules (7..39), same for the batch;
 *   P,T,CLW,WBRODL [nprof][nlay_max];  WKL [nprof][nlay_max][nmol];
 *   cntnm_fac[7] = XSELF,XFRGN,XCO2C,XO3CN,XO2CN,XN2CN,XRAYL (CntnmFactors_t, CntnmFactors.f90:17-19);
 * outputs (zero-filled for layers >= nlay[p]):
 *   O [nprof][nlay_max][nwn], O_BY_MOL [nprof][nlay_max][nmol][nwn],
 *   OC [nprof][nlay_max][MONORTM_NCONT][nwn], O_CLW [nprof][nlay_max][nwn]. */
int monortm_hip_modm(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay,
                     int nlay_max, int nmol, const monortm_real *P, const monortm_real *T,
                     const monortm_real *CLW, const monortm_real *WKL, const monortm_real *WBRODL,
                     const double *cntnm_fac, double sclcpl, double sclhw, double y0res, int ibrd, int ixsect,
                     monortm_real *O, monortm_real *O_BY_MOL, monortm_real *OC, monortm_real *O_CLW);

/* Cross-section molecules (IXSECT = 1; replaces MONORTM_XSEC_SUB + convolve, src/monortm_sub.F90:1540-1834, called from
 * src/modm.f90:197).  The reference keeps the tables in COMMON /XSECTR/, /XSECTF/ (filled by XSREAD from FSCDXS, :1246-1421)
 * and re-reads the xs files in every call; here the caller hands the parsed tables over once per context (or whenever they
 * change):
 *   nxs molecules (in the order of the request = the second axis of XAMNT), nreg (molecule, spectral region) rows;
 *   reg[nreg][8] = molecule (0-based position in the request), V1FX, V2FX of the FSCDXS entry (a region is processed when some
 *   wavenumber of the call lies within 1 cm-1 of them, :1645), points per spectrum, temperatures (1..6), XDOPLR (:1383-1387),
 *   V1 and V2 on the header of the LAST xs file of the region (with the point count they define the grid of every spectrum of
 *   the region and the in-range test of a wavenumber, :1663-1666, :1709, :1789); temps[nreg][6] K ascending; pres_mb[nreg][6] measurement pressures in millibar (torr x 1013/760, :1626);
 *   offs[nreg][6] offsets of the spectra in pool[npool].  A multi-device context uploads to every device. */
int monortm_hip_xsec_tables(void *ctx, int nxs, int nreg, const double *reg, const double *temps, const double *pres_mb,
                            const long long *offs, const double *pool, long long npool);

/* MODM with the hidden inputs / the output of the cross-section path as arguments: XAMNT [nprof][nlay_max][nxs] = the
 * reference's COMMON /PATHX/ XAMNT (src/monortm.f90:233,:526-528), ODXSEC [nprof][nlay_max][nwn] = its ODXSEC argument
 * (src/modm.f90:24; total over the molecules, added into O at :268).  ixsect = 0: both may be NULL and the call is
 * monortm_hip_modm.  Not reproduced: the reference's own driver allocates ODXSEC(nwn, .) while MONORTM_XSEC_SUB indexes it
 * as (NWNMX, MXLAY) (:1611) and so writes out of bounds for every layer but the first; and convolve() overruns its
 * 10^7-point work array for layers whose pressure is below that of the measurement (:1758,:1773-1786) - the formulas are
 * evaluated as written, without those arrays. */
int monortm_hip_modm_xs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay,
                        int nlay_max, int nmol, const monortm_real *P, const monortm_real *T,
                        const monortm_real *CLW, const monortm_real *WKL, const monortm_real *WBRODL,
                        const double *cntnm_fac, double sclcpl, double sclhw, double y0res, int ibrd, int ixsect,
                        const monortm_real *XAMNT, monortm_real *ODXSEC,
                        monortm_real *O, monortm_real *O_BY_MOL, monortm_real *OC, monortm_real *O_CLW);

/* CALCTMR + RTM, host buffers.  Replaces src/RTMmono.f90:239-325 and :13-221.
 *   irt[nprof] 1 up / 2 limb / 3 down;  iout = 1 => TB computed;  T [nprof][nlay_max], TZ [nprof][nlay_max+1];
 *   O [nprof][nlay_max][nwn];  tmpsfc[nprof] is IN/OUT exactly like the reference's TMPSFC argument
 *   (set to 2.75 K for irt = 2,3; RTMmono.f90:113-124);  emiss, reflc [nprof][nwn];
 * outputs [nprof][nwn]: RUP, RDN, TRTOT, RAD, TB, TMR (TMR may be NULL to skip CALCTMR). */
int monortm_hip_rtm(void *ctx, int nprof, int nwn, const double *wn, const int *nlay, int nlay_max,
                    const int *irt, int iout, const monortm_real *T, const monortm_real *TZ,
                    const monortm_real *O, monortm_real *tmpsfc, const monortm_real *emiss,
                    const monortm_real *reflc, monortm_real *RUP, monortm_real *RDN, monortm_real *TRTOT,
                    monortm_real *RAD, monortm_real *TB, monortm_real *TMR);

/* Same operations on DEVICE pointers, asynchronous on `stream` (hipStream_t, may be NULL).
 * nlay / irt are device int arrays, tmpsfc a device monortm_real array.  The context's device must be the calling
 * thread's current device (checked: MONORTM_EARG otherwise); the host-buffer entry points select it themselves.
 * wn_ends: HOST array {wn[0], wn[nwn-1]} (they size the continuum grid, modm.f90:180-185), or NULL - then the two
 * values are read back from device memory, which synchronises `stream` once per call. */
int monortm_hip_modm_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay,
                         int nlay_max, int nmol, const monortm_real *P, const monortm_real *T,
                         const monortm_real *CLW, const monortm_real *WKL, const monortm_real *WBRODL,
                         const double *cntnm_fac /*host*/, double sclcpl, double sclhw, double y0res, int ibrd,
                         int ixsect, monortm_real *O, monortm_real *O_BY_MOL, monortm_real *OC,
                         monortm_real *O_CLW, const double *wn_ends, void *stream);

int monortm_hip_modm_xs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay,
                            int nlay_max, int nmol, const monortm_real *P, const monortm_real *T,
                            const monortm_real *CLW, const monortm_real *WKL, const monortm_real *WBRODL,
                            const double *cntnm_fac /*host*/, double sclcpl, double sclhw, double y0res, int ibrd,
                            int ixsect, const monortm_real *XAMNT, monortm_real *ODXSEC, monortm_real *O,
                            monortm_real *O_BY_MOL, monortm_real *OC, monortm_real *O_CLW, const double *wn_ends,
                            void *stream);

int monortm_hip_rtm_dev(void *ctx, int nprof, int nwn, const double *wn, const int *nlay, int nlay_max,
                        const int *irt, int iout, const monortm_real *T, const monortm_real *TZ,
                        const monortm_real *O, monortm_real *tmpsfc, const monortm_real *emiss,
                        const monortm_real *reflc, monortm_real *RUP, monortm_real *RDN, monortm_real *TRTOT,
                        monortm_real *RAD, monortm_real *TB, monortm_real *TMR, void *stream);

/* CALCTMR + RTM along npath paths per profile from ONE set of optical depths.  No reference counterpart: the reference gets every
 * path from a new LBLATM + MODM run.  path [nprof][npath][nlay_max] (monortm_real) = the factor by which every amount of the layer
 * (WKL, WBRODL, CLW, XAMNT) along that path exceeds the amounts O was computed for; finite, >= 0; entries of layers >= nlay[p] are
 * ignored.  Exact while the layers' P and T are those O was computed with (plane-parallel secants: exact; refracted / spherical
 * geometry: the caller's layer means).  irt, T, TZ, tmpsfc (IN/OUT as in monortm_hip_rtm) are per profile;
 * emiss, reflc: [nprof][nwn] (sfc_per_path = 0) or [nprof][npath][nwn] (1).  Outputs [nprof][npath][nwn]; TMR may be NULL.
 * 1 <= npath <= 16384, nlay_max <= 603 (the bound of monortm_hip_modm).  Host buffers: a negative or non-finite factor of an active
 * layer is MONORTM_EARG and nothing is launched; a multi-device context shards the profiles like monortm_hip_rtm; when O is what the
 * preceding monortm_hip_modm call returned it is read where it lies on the device (counted by monortm_hip_counter(ctx, 1)). */
int monortm_hip_rtm_scan(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max,
                         const int *irt, int iout, const monortm_real *T, const monortm_real *TZ, const monortm_real *O,
                         const monortm_real *path, monortm_real *tmpsfc, int sfc_per_path, const monortm_real *emiss,
                         const monortm_real *reflc, monortm_real *RUP, monortm_real *RDN, monortm_real *TRTOT,
                         monortm_real *RAD, monortm_real *TB, monortm_real *TMR);
/* The same on device pointers (nlay, irt int arrays, the others monortm_real), asynchronous on `stream`; one-device context, which
 * must be the current device.  Allocates nothing.  A bad factor of an active layer surfaces through monortm_hip_check
 * (MONORTM_EARG); the kernel still finishes. */
int monortm_hip_rtm_scan_dev(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max,
                             const int *irt, int iout, const monortm_real *T, const monortm_real *TZ, const monortm_real *O,
                             const monortm_real *path, monortm_real *tmpsfc, int sfc_per_path, const monortm_real *emiss,
                             const monortm_real *reflc, monortm_real *RUP, monortm_real *RDN, monortm_real *TRTOT,
                             monortm_real *RAD, monortm_real *TB, monortm_real *TMR, void *stream);

/* ---- Jacobians for retrievals (no reference counterpart: "CURRENTLY MONORTM DOES NOT HANDLE DERIVATIVES",
 * src/monortm_sub.F90:199).  DESIGN.md section 3.6 has the method and the error budget.
 *   Inputs: the arguments of monortm_hip_modm / monortm_hip_rtm.  K holds PARTIAL derivatives with respect to them, every other
 *   input fixed (d/dT_k holds WKL, P and TZ constant); callers chain to their own state vector (monortm_hip_oe_step reads the
 *   per-measurement K of monortm_hip_obs_jacobian through a state map and returns the retrieval's update).
 *   quantity = 1: q = TB (needs RAD > 0);  quantity = 0: q = RAD.
 *   K_T   [nprof][nlay_max][nwn]     dq/dT_k, layer temperature: the Planck term of RTM and, in monortm_hip_jacobian, its effect on O
 *                                    through MODM (lines, continuum, cloud);  monortm_hip_rtm_jac: the Planck term only
 *   K_TZ  [nprof][nlay_max + 1][nwn] dq/dTZ_j, level temperature (RTM only, analytic; TZ_0 enters only RDN of layer 1, TZ_nlay only
 *                                    RUP: 0 for irt = 3)
 *   K_W   [nprof][nlay_max][njac][nwn] dq/d ln WKL_k,jac_mol[i] = WKL dq/dWKL (0 where WKL = 0); for the other Jacobian variables
 *                                    (MONORTM_JVAR_*, below): what their table says
 *   K_CLW [nprof][nlay_max][nwn]     dq/dCLW_k; the cloud optical depth is linear in CLW (ODCLW_TKC, src/CloudOptProp.f90:18-20,49),
 *                                    dO_k/dCLW_k = ODCLW_TKC(wn, T_k, 1) in closed form (right at CLW = 0 too)
 *   K_O   [nprof][nlay_max][nwn]     dq/dO_k, the optical-depth Jacobian (to chain cross sections or species outside jac_mol)
 *   K_SFC [nprof][3][nwn]            dq/dTMPSFC, dq/dEMISS, dq/dREFLC; the TMPSFC term is 0 for irt = 2, 3 (RTM replaces TMPSFC by
 *                                    2.75 K there, RTMmono.f90:113-124)
 *   Wavenumber axis fastest; entries of layers >= nlay[p] and levels > nlay[p] are 0.  tmpsfc is input only (not set to 2.75).
 * The derivatives of RTM are the exact adjoint of RAD_UP_DN + RTM.  Those of MODM are central differences: layers do not interact
 * in MODM (src/modm.f90:200-272), so ONE MODM evaluation with every layer's T shifted by +h gives O(T_k + h) for all k at once -
 * 2 evaluations per variable, not 2 nlay.  Half-steps (monortm_hip_set_option "jac_dt" / "jac_dlnw"): */
#define MONORTM_JAC_DT 1e-2   /* K: T +- h */
#define MONORTM_JAC_DLNW 1e-4 /* WKL (1 +- eps) */
/* O is only piecewise smooth in T (line-shape switches at zeta > 0.99 and |v - v0| > 100 HWHM_D, src/modm.f90:427): a difference
 * across a switch reports the switch.  T +- h must stay within 70-3000 K (MONORTM_ETEMP otherwise).
 * Cross-section molecules (IXSECT = 1): the *_xs entries below (monortm_hip_jacobian_xs, _scan_jacobian_xs, _obs_jacobian_xs and
 * their _dev variants) - DESIGN.md section 3.12.
 *
 * Jacobian variables: an entry of jac_mol[] is a 1-based molecule (1..nmol) or one of the codes below, in any
 * mix; slot i of K_W belongs to jac_mol[i].  eps is the "jac_dlnw" half-step for every one of them.
 *   per layer   MONORTM_JVAR_P, _WBROD: P_k, WBRODL_k x (1 +- eps); the slot holds dq/d ln P_k, dq/d ln WBRODL_k (0 where WBRODL = 0),
 *               T, WKL and every other input fixed
 *   scalar      MONORTM_JVAR_CNTNM0 + i (cntnm_fac[i], i = 0..6: XSELF, XFRGN, XCO2C, XO3CN, XO2CN, XN2CN, XRAYL), _SCLCPL, _SCLHW,
 *               _Y0RES: the argument +- eps (additive); slot [k] holds the part of dq/dtheta that acts through layer k, and the SUM
 *               of the slots over the layers is dq/dtheta.  MODM switches a continuum off at a factor <= 0, so where fac - eps <= 0
 *               the difference is one-sided, (O(fac + 2 eps) - O(fac)) / (2 eps): exact as well, O being linear in the factor.
 *   per layer   MONORTM_JVAR_XS0 + x, x = 0 .. nxs - 1: cross-section molecule x - the 0-based position in the cross-section request,
 *               i.e. the `molecule` column of monortm_hip_xsec_tables and the second axis of XAMNT (at most 38, MX_XS).  The *_xs
 *               entries with ixsect = 1 only.  The slot holds dq/d ln XAMNT_k,x, exactly 0 where XAMNT = 0; O is linear in XAMNT, so
 *               this is K_O times the molecule's own term and nothing is differenced. */
#define MONORTM_JVAR_P 1001
#define MONORTM_JVAR_WBROD 1002
#define MONORTM_JVAR_CNTNM0 1011 /* + i, i = 0..6 */
#define MONORTM_JVAR_SCLCPL 1021
#define MONORTM_JVAR_SCLHW 1022
#define MONORTM_JVAR_Y0RES 1023
#define MONORTM_JVAR_XS0 (1101) /* + x, x = 0 .. nxs - 1: the base of a family of codes, not a variable of its own */
/*
 * RTM adjoint only, given O (e.g. from monortm_hip_modm): RAD, TB, K_O, K_T (Planck terms only), K_TZ, K_SFC.  real_kind 8 and 4
 * (double arithmetic either way).  Host buffers; a multi-device context shards the profiles like monortm_hip_rtm. */
int monortm_hip_rtm_jac(void *ctx, int nprof, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                        int quantity, const monortm_real *T, const monortm_real *TZ, const monortm_real *O,
                        const monortm_real *tmpsfc, const monortm_real *emiss, const monortm_real *reflc,
                        monortm_real *RAD, monortm_real *TB, monortm_real *K_O, monortm_real *K_T, monortm_real *K_TZ,
                        monortm_real *K_SFC);
/* The same on device pointers (nlay, irt, tmpsfc device arrays), asynchronous on `stream`; one-device context. */
int monortm_hip_rtm_jac_dev(void *ctx, int nprof, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                            int quantity, const monortm_real *T, const monortm_real *TZ, const monortm_real *O,
                            const monortm_real *tmpsfc, const monortm_real *emiss, const monortm_real *reflc,
                            monortm_real *RAD, monortm_real *TB, monortm_real *K_O, monortm_real *K_T, monortm_real *K_TZ,
                            monortm_real *K_SFC, void *stream);

/* MODM + RTM with Jacobians: the forward outputs of the base state (O, RAD, TB) and K_T (total), K_TZ, K_W, K_CLW, K_O (may be
 * NULL), K_SFC.  jac_mol[njac]: HOST array of 1-based molecules (<= nmol) and MONORTM_JVAR_* codes (no duplicates, njac <= 39;
 * njac = 0: no K_W, which may then be NULL) in both variants.  real_kind 8 only (MONORTM_EUNSUPPORTED otherwise).  Host buffers: shards like monortm_hip_modm.
 * Errors: MONORTM_EARG for a NULL required array, a bad quantity, a bad jac_mol; MONORTM_ETEMP when T +- h leaves 70-3000 K. */
int monortm_hip_jacobian(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                         int nmol, const monortm_real *P, const monortm_real *T, const monortm_real *CLW,
                         const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac, double sclcpl,
                         double sclhw, double y0res, int ibrd, const int *irt, const monortm_real *TZ,
                         const monortm_real *tmpsfc, const monortm_real *emiss, const monortm_real *reflc, int quantity,
                         int njac, const int *jac_mol, monortm_real *O, monortm_real *RAD, monortm_real *TB,
                         monortm_real *K_T, monortm_real *K_TZ, monortm_real *K_W, monortm_real *K_CLW, monortm_real *K_O,
                         monortm_real *K_SFC);
/* The same on device pointers, asynchronous on `stream`; one-device context.  wn_ends as for monortm_hip_modm_dev (given: no
 * synchronisation).  Device-side failures (temperature range) surface through monortm_hip_check.  After one call, a second of the
 * same shapes allocates nothing (graph capture). */
int monortm_hip_jacobian_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                             int nmol, const monortm_real *P, const monortm_real *T, const monortm_real *CLW,
                             const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac /*host*/,
                             double sclcpl, double sclhw, double y0res, int ibrd, const int *irt, const monortm_real *TZ,
                             const monortm_real *tmpsfc, const monortm_real *emiss, const monortm_real *reflc, int quantity,
                             int njac, const int *jac_mol /*host*/, monortm_real *O, monortm_real *RAD, monortm_real *TB,
                             monortm_real *K_T, monortm_real *K_TZ, monortm_real *K_W, monortm_real *K_CLW,
                             monortm_real *K_O, monortm_real *K_SFC, const double *wn_ends, void *stream);

/* ---- Jacobians of path scans: K for npath paths per profile from ONE set of optical depths and ONE set of perturbed MODM states
 * (no reference counterpart; the radiance recurrence differentiated is src/RTMmono.f90:13-221).  DESIGN.md section 3.8.
 * path, sfc_per_path, emiss, reflc as in monortm_hip_rtm_scan; quantity and the meaning of K as in monortm_hip_rtm_jac.  Along path j
 * the optical depth of layer k is tau_jk = path_jk O_k; with ko_jk = dq_j / dtau_jk:
 *   RAD, TB [nprof][npath][nwn]
 *   K_O    [nprof][npath][nlay_max][nwn]       path_jk ko_jk = dq_j / dO_k of the vertical O (may be NULL)
 *   K_PATH [nprof][npath][nlay_max][nwn]       O_k ko_jk = dq_j / dpath_jk, to chain with d path / d angle (may be NULL)
 *   K_T    [nprof][npath][nlay_max][nwn]       the Planck term; monortm_hip_scan_jacobian adds K_O dO_k/dT_k
 *   K_TZ   [nprof][npath][nlay_max + 1][nwn],  K_SFC [nprof][npath][3][nwn]
 *   K_W    [nprof][npath][nlay_max][njac][nwn] K_O dO_k / d ln WKL_k of the batch's own (vertical) amounts
 *   K_CLW  [nprof][npath][nlay_max][nwn]       K_O ODCLW_TKC(wn, T_k, 1): with respect to the batch's own (vertical) CLW_k
 * Entries of layers >= nlay[p] and levels > nlay[p] are 0; tmpsfc is input only.  1 <= npath <= 16384, nlay_max <= 603.
 *
 * RTM adjoint only, given O: real_kind 8 and 4.  Host buffers: nlay and the factors of the whole call are checked before anything is
 * staged on any device (MONORTM_EARG, nothing is launched); a multi-device context shards the profiles like monortm_hip_rtm_scan. */
int monortm_hip_rtm_scan_jac(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max,
                             const int *irt, int quantity, const monortm_real *T, const monortm_real *TZ, const monortm_real *O,
                             const monortm_real *path, const monortm_real *tmpsfc, int sfc_per_path, const monortm_real *emiss,
                             const monortm_real *reflc, monortm_real *RAD, monortm_real *TB, monortm_real *K_O,
                             monortm_real *K_PATH, monortm_real *K_T, monortm_real *K_TZ, monortm_real *K_SFC);
/* The same on device pointers, asynchronous on `stream`; one-device context.  Allocates nothing.  A bad factor of an active layer
 * surfaces through monortm_hip_check (MONORTM_EARG). */
int monortm_hip_rtm_scan_jac_dev(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max,
                                 const int *irt, int quantity, const monortm_real *T, const monortm_real *TZ,
                                 const monortm_real *O, const monortm_real *path, const monortm_real *tmpsfc, int sfc_per_path,
                                 const monortm_real *emiss, const monortm_real *reflc, monortm_real *RAD, monortm_real *TB,
                                 monortm_real *K_O, monortm_real *K_PATH, monortm_real *K_T, monortm_real *K_TZ,
                                 monortm_real *K_SFC, void *stream);

/* MODM + RTM with Jacobians along npath paths: the 3 + 2 njac MODM passes of monortm_hip_jacobian ONCE (their differences do not depend
 * on the path), then one adjoint launch for all paths.  O returns the vertical optical depths.  real_kind 8 only
 * (MONORTM_EUNSUPPORTED otherwise); jac_mol, the half-steps and the errors as monortm_hip_jacobian, the factors as above.  Cross-section
 * molecules: monortm_hip_scan_jacobian_xs. */
int monortm_hip_scan_jacobian(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                              int nmol, const monortm_real *P, const monortm_real *T, const monortm_real *CLW,
                              const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac, double sclcpl,
                              double sclhw, double y0res, int ibrd, const int *irt, const monortm_real *TZ,
                              const monortm_real *tmpsfc, const monortm_real *emiss, const monortm_real *reflc, int quantity,
                              int njac, const int *jac_mol, int npath, const monortm_real *path, int sfc_per_path,
                              monortm_real *O, monortm_real *RAD, monortm_real *TB, monortm_real *K_T, monortm_real *K_TZ,
                              monortm_real *K_W, monortm_real *K_CLW, monortm_real *K_O, monortm_real *K_PATH,
                              monortm_real *K_SFC);
/* The same on device pointers, asynchronous on `stream`; one-device context.  wn_ends as for monortm_hip_modm_dev.  Device-side
 * failures (temperature range, bad factors) surface through monortm_hip_check.  After one call, a second of the same shapes
 * allocates nothing (graph capture). */
int monortm_hip_scan_jacobian_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                                  int nmol, const monortm_real *P, const monortm_real *T, const monortm_real *CLW,
                                  const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac /*host*/,
                                  double sclcpl, double sclhw, double y0res, int ibrd, const int *irt, const monortm_real *TZ,
                                  const monortm_real *tmpsfc, const monortm_real *emiss, const monortm_real *reflc,
                                  int quantity, int njac, const int *jac_mol /*host*/, int npath, const monortm_real *path,
                                  int sfc_per_path, monortm_real *O, monortm_real *RAD, monortm_real *TB, monortm_real *K_T,
                                  monortm_real *K_TZ, monortm_real *K_W, monortm_real *K_CLW, monortm_real *K_O,
                                  monortm_real *K_PATH, monortm_real *K_SFC, const double *wn_ends, void *stream);

/* ---- Channel- and beam-averaged Jacobians of path scans: K per MEASUREMENT (no reference counterpart).  DESIGN.md section 3.9.
 * An instrument measures a passband, sampled by several wavenumbers, through a beam, sampled by several paths of a scan:
 *   y[p][v][c] = sum_{j in view v} wpath[j] sum_{i: chan[i] = c} wchan[i] q[p][j][i],   q = RAD or TB by `quantity`.
 * Every derivative below is taken with respect to a per-layer or per-profile variable that all samples of a measurement share, so
 * the contraction is exact; it happens inside the kernel that forms the monochromatic per-path terms (rtm_obs_jac_kernel.hip), and
 * none of those reaches memory.
 *
 * The measurement operator is defined once per context: the paths of view v are view_start[v] .. view_start[v + 1] - 1 (CSR: the
 * paths of a view are adjacent; view_start[0] = 0, non-decreasing, view_start[nview] = npath; an empty view is allowed, its outputs
 * are 0).  chan[i] in [-1, nchan) is an arbitrary map of wavenumber i to its channel (-1: unused; sidebands may nest, a channel may
 * have no sample: 0).  The weights are finite doubles of any sign; normalisation is the caller's.  1 <= npath <= 16384, nwn <= 80000,
 * nview <= 65535, nchan <= 65536.  Everything is checked here, on the host: bad shapes, bad indices or non-finite weights return
 * MONORTM_EARG with a message and create nothing.  The tables go to the device (of a multi-device context: to every device) once;
 * the calls below take the handle and copy nothing.  A context holds up to 16 operators; all are released by monortm_hip_finalize.
 * A stale or foreign handle: MONORTM_EARG.  monortm_hip_obs_destroy waits for the device before it frees the tables. */
int monortm_hip_obs_create(void *ctx, int npath, int nwn, int nview, int nchan, const int *view_start /*[nview + 1]*/,
                           const double *wpath /*[npath]*/, const int *chan /*[nwn]*/, const double *wchan /*[nwn]*/, int *handle);
int monortm_hip_obs_destroy(void *ctx, int handle);

/* Outputs, in the context's real type (arguments, refusals and the meaning of K as monortm_hip_rtm_scan_jac / monortm_hip_scan_jacobian;
 * npath and nwn must be the operator's, MONORTM_EARG otherwise):
 *   Y            [nprof][nview][nchan]
 *   K_T, K_CLW   [nprof][nview][nlay_max][nchan]
 *   K_TZ         [nprof][nview][nlay_max + 1][nchan]
 *   K_W          [nprof][nview][nlay_max][njac][nchan]
 *   K_SFC        [nprof][nview][3][nchan]      dy/dTMPSFC; rows 1, 2: the derivative with respect to a COMMON shift of EMISS (REFLC) of
 *                                              all samples of the measurement - every wavenumber (and, with sfc_per_path, path) of it
 * Entries of layers >= nlay[p] and levels > nlay[p] are 0.  There is no K_O and no K_PATH: their variables are per wavenumber or per
 * path, a contraction over them means nothing (use monortm_hip_scan_jacobian).  The sums are formed in a fixed order - paths ascending
 * within a tile of 4, wavenumbers ascending within a block of 64, then tiles ascending and blocks ascending within a tile - without
 * atomics: repeated calls give the same bits, and a profile gives the same bits alone and inside a batch.
 *
 * RTM adjoint only, given O: real_kind 8 and 4.  Host buffers: sharded by profile like monortm_hip_rtm_scan_jac, nlay and the factors
 * of the whole call checked first; with real_kind 4 the sums are held in double and rounded once. */
int monortm_hip_rtm_obs_jac(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max,
                            const int *irt, int quantity, const monortm_real *T, const monortm_real *TZ, const monortm_real *O,
                            const monortm_real *path, const monortm_real *tmpsfc, int sfc_per_path, const monortm_real *emiss,
                            const monortm_real *reflc, int obs, monortm_real *Y, monortm_real *K_T, monortm_real *K_TZ,
                            monortm_real *K_SFC);
/* The same on device pointers, asynchronous on `stream`; one-device context.  Allocates and copies nothing.  A bad factor of an active
 * layer surfaces through monortm_hip_check (MONORTM_EARG).  With real_kind 4 the outputs themselves hold the running sums: one float
 * rounding per (tile of paths, block of wavenumbers) that contributes to an element. */
int monortm_hip_rtm_obs_jac_dev(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max,
                                const int *irt, int quantity, const monortm_real *T, const monortm_real *TZ, const monortm_real *O,
                                const monortm_real *path, const monortm_real *tmpsfc, int sfc_per_path, const monortm_real *emiss,
                                const monortm_real *reflc, int obs, monortm_real *Y, monortm_real *K_T, monortm_real *K_TZ,
                                monortm_real *K_SFC, void *stream);

/* MODM + RTM with Jacobians per measurement: the 3 + 2 njac MODM passes of monortm_hip_jacobian ONCE, then one launch of the contracting
 * adjoint.  O returns the vertical optical depths exactly as monortm_hip_scan_jacobian does.  real_kind 8 only (MONORTM_EUNSUPPORTED
 * otherwise); jac_mol, the half-steps, the factors and the errors as monortm_hip_scan_jacobian.  Cross-section molecules:
 * monortm_hip_obs_jacobian_xs. */
int monortm_hip_obs_jacobian(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                             int nmol, const monortm_real *P, const monortm_real *T, const monortm_real *CLW,
                             const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac, double sclcpl,
                             double sclhw, double y0res, int ibrd, const int *irt, const monortm_real *TZ,
                             const monortm_real *tmpsfc, const monortm_real *emiss, const monortm_real *reflc, int quantity,
                             int njac, const int *jac_mol, int npath, const monortm_real *path, int sfc_per_path, int obs,
                             monortm_real *O, monortm_real *Y, monortm_real *K_T, monortm_real *K_TZ, monortm_real *K_W,
                             monortm_real *K_CLW, monortm_real *K_SFC);
/* The same on device pointers, asynchronous on `stream`; one-device context.  wn_ends as for monortm_hip_modm_dev.  Device-side
 * failures (temperature range, bad factors) surface through monortm_hip_check.  After one call, a second of the same shapes
 * allocates nothing (graph capture); the launch of the adjoint itself never allocates. */
int monortm_hip_obs_jacobian_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                                 int nmol, const monortm_real *P, const monortm_real *T, const monortm_real *CLW,
                                 const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac /*host*/,
                                 double sclcpl, double sclhw, double y0res, int ibrd, const int *irt, const monortm_real *TZ,
                                 const monortm_real *tmpsfc, const monortm_real *emiss, const monortm_real *reflc,
                                 int quantity, int njac, const int *jac_mol /*host*/, int npath, const monortm_real *path,
                                 int sfc_per_path, int obs, monortm_real *O, monortm_real *Y, monortm_real *K_T,
                                 monortm_real *K_TZ, monortm_real *K_W, monortm_real *K_CLW, monortm_real *K_SFC,
                                 const double *wn_ends, void *stream);

/* ---- The Jacobians with the cross-section molecules (IXSECT = 1; no reference counterpart).  DESIGN.md section 3.12.
 * The six entries above with two more arguments behind ibrd, as monortm_hip_modm_xs has them: ixsect and XAMNT [nprof][nlay_max][nxs]
 * (read with ixsect = 1 only).  With ixsect = 0 they ARE the entries above (which call them), bit for bit.  With ixsect = 1:
 *   O, K_O and through them every slot include the cross sections: O is what monortm_hip_modm_xs returns.
 *   K_T and the MONORTM_JVAR_P slot include the cross sections' own dependence on T and P.  MONORTM_XSEC_SUB resamples every spectrum
 *   on a grid whose point count, and a handful of branches besides, jump with P and T, so its ODXSEC is not differentiable as it
 *   stands; the derivative here is that of the BASE state's finite sum - grid, temperature bracket, branches and stopping trip held
 *   as the base state has them - evaluated at T +- h, P (1 +- eps) (xsec_jac_kernel.hip).  A layer exactly at a table temperature
 *   takes the bracket the reference's `tave <= tx` picks: the derivative is one-sided there.
 *   MONORTM_JVAR_XS0 + x names molecule x of the request as a Jacobian variable (table above).
 *   States of molecules, WBRODL and the scalars are differenced without the cross sections, which would cancel.
 *   Along a scan a path factor multiplies XAMNT like every other amount; K is with respect to the batch's own vertical XAMNT.
 * Refused before anything is launched: real_kind 4 (MONORTM_EUNSUPPORTED); ixsect outside 0, 1, a MONORTM_JVAR_XS0 code with
 * ixsect = 0 or with x >= the nxs of the context's tables, ixsect = 1 without tables (monortm_hip_xsec_tables) or with XAMNT NULL
 * (MONORTM_EARG).  njac <= 39 as ever.  Host entries shard by profile as their parents do. */
int monortm_hip_jacobian_xs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                            int nmol, const monortm_real *P, const monortm_real *T, const monortm_real *CLW, const
                            monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac, double sclcpl, double
                            sclhw, double y0res, int ibrd, int ixsect, const monortm_real *XAMNT, const int *irt, const
                            monortm_real *TZ, const monortm_real *tmpsfc, const monortm_real *emiss, const monortm_real
                            *reflc, int quantity, int njac, const int *jac_mol, monortm_real *O, monortm_real *RAD,
                            monortm_real *TB, monortm_real *K_T, monortm_real *K_TZ, monortm_real *K_W, monortm_real
                            *K_CLW, monortm_real *K_O, monortm_real *K_SFC);
int monortm_hip_jacobian_xs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int
                                nlay_max, int nmol, const monortm_real *P, const monortm_real *T, const monortm_real *CLW,
                                const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac /*host*/,
                                double sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const monortm_real
                                *XAMNT, const int *irt, const monortm_real *TZ, const monortm_real *tmpsfc, const
                                monortm_real *emiss, const monortm_real *reflc, int quantity, int njac, const int *jac_mol
                                /*host*/, monortm_real *O, monortm_real *RAD, monortm_real *TB, monortm_real *K_T,
                                monortm_real *K_TZ, monortm_real *K_W, monortm_real *K_CLW, monortm_real *K_O,
                                monortm_real *K_SFC, const double *wn_ends, void *stream);
int monortm_hip_scan_jacobian_xs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int
                                 nlay_max, int nmol, const monortm_real *P, const monortm_real *T, const monortm_real
                                 *CLW, const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac,
                                 double sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const monortm_real
                                 *XAMNT, const int *irt, const monortm_real *TZ, const monortm_real *tmpsfc, const
                                 monortm_real *emiss, const monortm_real *reflc, int quantity, int njac, const int
                                 *jac_mol, int npath, const monortm_real *path, int sfc_per_path, monortm_real *O,
                                 monortm_real *RAD, monortm_real *TB, monortm_real *K_T, monortm_real *K_TZ, monortm_real
                                 *K_W, monortm_real *K_CLW, monortm_real *K_O, monortm_real *K_PATH, monortm_real *K_SFC);
int monortm_hip_scan_jacobian_xs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int
                                     nlay_max, int nmol, const monortm_real *P, const monortm_real *T, const monortm_real
                                     *CLW, const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac
                                     /*host*/, double sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const
                                     monortm_real *XAMNT, const int *irt, const monortm_real *TZ, const monortm_real
                                     *tmpsfc, const monortm_real *emiss, const monortm_real *reflc, int quantity, int
                                     njac, const int *jac_mol /*host*/, int npath, const monortm_real *path, int
                                     sfc_per_path, monortm_real *O, monortm_real *RAD, monortm_real *TB, monortm_real
                                     *K_T, monortm_real *K_TZ, monortm_real *K_W, monortm_real *K_CLW, monortm_real *K_O,
                                     monortm_real *K_PATH, monortm_real *K_SFC, const double *wn_ends, void *stream);
int monortm_hip_obs_jacobian_xs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int
                                nlay_max, int nmol, const monortm_real *P, const monortm_real *T, const monortm_real *CLW,
                                const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac, double
                                sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const monortm_real *XAMNT, const
                                int *irt, const monortm_real *TZ, const monortm_real *tmpsfc, const monortm_real *emiss,
                                const monortm_real *reflc, int quantity, int njac, const int *jac_mol, int npath, const
                                monortm_real *path, int sfc_per_path, int obs, monortm_real *O, monortm_real *Y,
                                monortm_real *K_T, monortm_real *K_TZ, monortm_real *K_W, monortm_real *K_CLW,
                                monortm_real *K_SFC);
int monortm_hip_obs_jacobian_xs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int
                                    nlay_max, int nmol, const monortm_real *P, const monortm_real *T, const monortm_real
                                    *CLW, const monortm_real *WKL, const monortm_real *WBRODL, const double *cntnm_fac
                                    /*host*/, double sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const
                                    monortm_real *XAMNT, const int *irt, const monortm_real *TZ, const monortm_real
                                    *tmpsfc, const monortm_real *emiss, const monortm_real *reflc, int quantity, int njac,
                                    const int *jac_mol /*host*/, int npath, const monortm_real *path, int sfc_per_path,
                                    int obs, monortm_real *O, monortm_real *Y, monortm_real *K_T, monortm_real *K_TZ,
                                    monortm_real *K_W, monortm_real *K_CLW, monortm_real *K_SFC, const double *wn_ends,
                                    void *stream);

/* ---- The forward measurement operator: channel- and beam-averaged scans, y = F(x) without K (no reference counterpart; the radiance
 * recurrence along every path is RTM's, src/RTMmono.f90:13-221).  DESIGN.md section 3.10.
 *   Y[p][v][c] = sum_{j in view v} wpath[j] sum_{i: chan[i] = c} wchan[i] q[p][j][i]
 * for a measurement operator of monortm_hip_obs_create, contracted inside the kernel that forms the monochromatic radiances
 * (rtm_obs_kernel.hip): none of them reaches memory.  The forward half of the entries above - the same owner thread per element, the
 * same fixed order of additions (paths ascending within a tile of 4, wavenumbers ascending within a block of 64, tiles ascending,
 * blocks ascending within a tile), no atomics: repeated calls give the same bits, and a profile gives the same bits alone and inside
 * a batch.  Empty views and channels without a sample are 0.
 *   quantity 0: q = RAD;  1: q = TB, the mean of the monochromatic brightness temperatures;
 *   quantity 2: the band brightness temperature - RAD is contracted (the power a radiometer integrates over its passband and beam)
 *     and the finished element converted at the channel's nominal wavenumber,
 *       Y = RADCN2 vcen[c] / log(RADCN1 vcen[c]^3 / Y_rad + 1).
 *     The conversion takes the contracted radiance as the band's MEAN radiance: normalising the weights (sum of wpath x wchan = 1 per
 *     measurement) is the caller's business, as everywhere for these operators.  An element without a sample stays 0; one whose
 *     contracted radiance is <= 0 or not finite (weights of mixed sign) is NaN.
 * vcen [nchan] doubles: read for quantity 2 only (may be NULL otherwise).  Host entries check it for the whole call - every value finite
 * and > 0, MONORTM_EARG otherwise, nothing launched; device entries take a device pointer, a bad value surfaces through
 * monortm_hip_check (MONORTM_EARG).  Y [nprof][nview][nchan] in the context's real type; tmpsfc is input only; npath and nwn must be
 * the operator's; the other arguments and refusals as monortm_hip_rtm_scan.
 *
 * From a given O: real_kind 8 and 4.  Host buffers: sharded by profile like monortm_hip_rtm_scan, nlay, the factors, the handle and
 * vcen of the whole call checked first; with real_kind 4 the sums are held (and the band temperature formed) in double and rounded
 * once.  O is always uploaded: the one-call entry below is the route without a copy. */
int monortm_hip_rtm_obs(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                        int quantity, const monortm_real *T, const monortm_real *TZ, const monortm_real *O, const monortm_real *path,
                        const monortm_real *tmpsfc, int sfc_per_path, const monortm_real *emiss, const monortm_real *reflc, int obs,
                        const double *vcen, monortm_real *Y);
/* The same on device pointers, asynchronous on `stream`; one-device context.  Allocates and copies nothing.  A bad factor of an active
 * layer or a bad vcen surfaces through monortm_hip_check (MONORTM_EARG).  With real_kind 4, Y itself holds the running sum: one float
 * rounding per (tile of paths, block of wavenumbers) that contributes to an element, then (quantity 2) the conversion. */
int monortm_hip_rtm_obs_dev(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                            int quantity, const monortm_real *T, const monortm_real *TZ, const monortm_real *O,
                            const monortm_real *path, const monortm_real *tmpsfc, int sfc_per_path, const monortm_real *emiss,
                            const monortm_real *reflc, int obs, const double *vcen, monortm_real *Y, void *stream);

/* MODM + the forward operator (no reference counterpart; MODM as monortm_hip_modm, the recurrence src/RTMmono.f90:13-221): ONE MODM
 * pass, then ONE launch of the forward kernel.  O returns the vertical optical depths exactly as monortm_hip_modm does.  real_kind 8
 * AND 4: nothing is perturbed, so none of the Jacobian entries' refusals applies.  Cross-section molecules: run monortm_hip_modm_xs
 * and hand its O to monortm_hip_rtm_obs. */
int monortm_hip_obs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                    const monortm_real *P, const monortm_real *T, const monortm_real *CLW, const monortm_real *WKL,
                    const monortm_real *WBRODL, const double *cntnm_fac, double sclcpl, double sclhw, double y0res, int ibrd,
                    const int *irt, const monortm_real *TZ, const monortm_real *tmpsfc, const monortm_real *emiss,
                    const monortm_real *reflc, int quantity, int npath, const monortm_real *path, int sfc_per_path, int obs,
                    const double *vcen, monortm_real *O, monortm_real *Y);
/* The same on device pointers, asynchronous on `stream`; one-device context, nprof <= 65535.  wn_ends as for monortm_hip_modm_dev.
 * Device-side failures (temperature range, bad factors, bad vcen) surface through monortm_hip_check.  After one call, a second of the
 * same shapes allocates nothing (graph capture); the launch of the forward kernel itself never allocates. */
int monortm_hip_obs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                        const monortm_real *P, const monortm_real *T, const monortm_real *CLW, const monortm_real *WKL,
                        const monortm_real *WBRODL, const double *cntnm_fac /*host*/, double sclcpl, double sclhw, double y0res,
                        int ibrd, const int *irt, const monortm_real *TZ, const monortm_real *tmpsfc, const monortm_real *emiss,
                        const monortm_real *reflc, int quantity, int npath, const monortm_real *path, int sfc_per_path, int obs,
                        const double *vcen, monortm_real *O, monortm_real *Y, const double *wn_ends, void *stream);

/* ---- The optimal-estimation step: a batched Gauss-Newton / Levenberg-Marquardt update from K (no reference counterpart; Rodgers,
 * Inverse Methods for Atmospheric Sounding, eq. 5.10).  DESIGN.md section 3.13.
 * Per profile, with m = nview x nchan measurements (measurement j = v nchan + c, the order of Y) and n = nstate state elements:
 *   d' = (xa - x) / (1 + gamma)
 *   W  = Sa K^T / (1 + gamma)                  [n][m]
 *   M  = K W + diag(se) = L L^T                [m][m], Cholesky
 *   r  = (y_obs - Y) - K d'
 *   z  = M^-1 r
 *   x_new = x + d' + W z
 *   post_var_i = Sa_ii / (1 + gamma) - |L^-1 W_i|^2      the diagonal of the posterior covariance of the damped problem
 *   avk_diag_i = (L^-1 W_i) . (L^-1 K_:,i)               the diagonal of the averaging kernel; its sum: the degrees of freedom for signal
 *   chi2 = sum_j (y_obs_j - Y_j)^2 / se_j
 * gamma = 0 is Rodgers (5.10); gamma > 0 equals the n-form x + [(1 + gamma) Sa^-1 + K^T Se^-1 K]^-1 [K^T Se^-1 (y_obs - Y) - Sa^-1 (x - xa)].
 * Sa^-1 never appears (nmeas << nstate for radiometers).
 *
 * K [m][n] is read IN PLACE from the outputs of monortm_hip_obs_jacobian[_xs][_dev], [nprof][nview][rows][nchan], through the state map:
 * state s is row state_row[s] of the array state_kind[s] names -
 *   0: K_T, layer k;  1: K_TZ, level;  2: K_W, k njac + i;  3: K_CLW, layer k;  4: K_SFC, 0..2.
 * Any order, repeats allowed; an array no state names may be NULL.  Rows of layers >= nlay[p] are 0 in K: their states relax to the prior.
 *   Y, y_obs        [nprof][nview][nchan]
 *   x, xa           [nprof][nstate]
 *   Sa              [nstate][nstate], or [nprof][nstate][nstate] with sa_per_profile = 1.  ONLY THE LOWER TRIANGLE IS READ (row >= column).
 *   se              [nmeas], or [nprof][nmeas] with se_per_profile = 1: the diagonal of the measurement-error covariance
 *   gamma           [nprof], or NULL: 0
 *   x_new           [nprof][nstate]                 post_var, avk_diag  [nprof][nstate], may be NULL
 *   chi2            [nprof], may be NULL            status  int [nprof]
 * A profile whose Cholesky meets a pivot <= 0 or not finite, whose r is not finite (a non-finite K, Sa, se, x, xa, Y or y_obs), or whose
 * gamma is negative or not finite has status 1, x_new = x and post_var = avk_diag = chi2 = 0; every other profile has status 0 and is
 * unaffected, bit for bit.  This is NOT an error of monortm_hip_check: one bad prior does not fail a batch.
 * One launch (oe_kernel.hip), one workgroup per profile, no atomics, every sum in ascending order of its index: repeated calls give the
 * same bits, and a profile gives the same bits alone and inside a batch.
 * Refused before anything is launched: real_kind 4 (MONORTM_EUNSUPPORTED); nmeas outside 1..128, nstate outside 1..2048, a kind outside
 * 0..4, a row outside its array, a kind whose array is NULL (MONORTM_EARG).  state_kind, state_row: host int [nstate].
 * Host buffers: sharded by profile like monortm_hip_obs_jacobian. */
int monortm_hip_oe_step(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind,
                        const int *state_row, const monortm_real *K_T, const monortm_real *K_TZ, const monortm_real *K_W,
                        const monortm_real *K_CLW, const monortm_real *K_SFC, const monortm_real *Y, const monortm_real *y_obs,
                        const monortm_real *x, const monortm_real *xa, const monortm_real *Sa, int sa_per_profile,
                        const monortm_real *se, int se_per_profile, const monortm_real *gamma, monortm_real *x_new,
                        monortm_real *post_var, monortm_real *avk_diag, monortm_real *chi2, int *status);
/* The same on device pointers (the state map stays on the host), asynchronous on `stream`; one-device context.  The workspace
 * ([nprof][2][nmeas][nstate] doubles) and the device copy of the state map are sized at the first call of a shape and kept: after one
 * call, a second of the same shapes and the same map allocates and copies nothing (graph capture).  A call with another map waits for
 * the stream before it replaces the device copy. */
int monortm_hip_oe_step_dev(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate,
                            const int *state_kind /*host*/, const int *state_row /*host*/, const monortm_real *K_T,
                            const monortm_real *K_TZ, const monortm_real *K_W, const monortm_real *K_CLW, const monortm_real *K_SFC,
                            const monortm_real *Y, const monortm_real *y_obs, const monortm_real *x, const monortm_real *xa,
                            const monortm_real *Sa, int sa_per_profile, const monortm_real *se, int se_per_profile,
                            const monortm_real *gamma, monortm_real *x_new, monortm_real *post_var, monortm_real *avk_diag,
                            monortm_real *chi2, int *status, void *stream);

/* ---- The optimal-estimation step with a full Se and the full diagnostics (Rodgers, sections 2.4 and 3.2).  DESIGN.md section 3.14.
 * Everything monortm_hip_oe_step computes, computed the same way, with
 *   Se, se_kind     se_kind 0: [nmeas] variances - exactly the se of monortm_hip_oe_step.
 *                   se_kind 1: [nmeas][nmeas], the measurement-error covariance (e.g. S_y + K_b S_b K_b^T).  ONLY THE LOWER TRIANGLE IS
 *                   READ.  M = K W + Se;  chi2 = (y_obs - Y)^T Se^-1 (y_obs - Y), from a Cholesky factor of Se.
 *                   With se_per_profile = 1: [nprof][nmeas] or [nprof][nmeas][nmeas].
 * and, with a = L^-1 W^T and b = L^-1 K ([nmeas][nstate] each; g = 1 / (1 + gamma)), four more outputs, each of which may be NULL:
 *   gain_t          [nprof][nmeas][nstate]   G^T = L^-T a = M^-1 W^T: row j is the response of every state element to measurement j
 *                                            (G = S_hat K^T Se^-1; measurement-major like K)
 *   avk             [nprof][nstate][nstate]  A = a^T b = G K: avk[i][i'] = d x_hat_i / d x_true_i'
 *   post_cov        [nprof][nstate][nstate]  S_hat = g Sa - a^T a = [(1 + gamma) Sa^-1 + K^T Se^-1 K]^-1, stored symmetric bit for bit
 *   dofs            [nprof]                  tr A, the sum of avk_diag in ascending i
 * diag(avk) is avk_diag and diag(post_cov) is post_var, bit for bit.  With se_kind 0 and the four outputs NULL the call launches what
 * monortm_hip_oe_step launches: the same bits.  With se_kind 1 and Se = diag(se), x_new, post_var and avk_diag are still the same bits;
 * chi2 differs by rounding.
 * A profile fails (status 1) as in monortm_hip_oe_step, and also when the Cholesky of Se meets a pivot <= 0 or not finite: x_new = x and
 * every diagnostic is 0, the three matrices included.  Other profiles are unaffected, bit for bit; no error of monortm_hip_check.
 * The step kernel (gain_t: one more phase of it, the back substitution in place) and, for avk / post_cov, one second launch of
 * oe_cov_kernel over (64 x 64 output tiles, profiles); no atomics, every element one thread's sum in ascending k: the same bits on
 * repeated calls, alone and in a batch.  The matrices are the caller's memory: 32 MB each per profile at nstate = 2048.
 * Refused before anything is launched: whatever monortm_hip_oe_step refuses, and se_kind outside 0..1 (MONORTM_EARG).
 * Host buffers: sharded by profile like monortm_hip_oe_step. */
int monortm_hip_oe_step_full(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind,
                             const int *state_row, const monortm_real *K_T, const monortm_real *K_TZ, const monortm_real *K_W,
                             const monortm_real *K_CLW, const monortm_real *K_SFC, const monortm_real *Y, const monortm_real *y_obs,
                             const monortm_real *x, const monortm_real *xa, const monortm_real *Sa, int sa_per_profile,
                             const monortm_real *Se, int se_kind, int se_per_profile, const monortm_real *gamma, monortm_real *x_new,
                             monortm_real *post_var, monortm_real *avk_diag, monortm_real *chi2, int *status, monortm_real *gain_t,
                             monortm_real *avk, monortm_real *post_cov, monortm_real *dofs);
/* The same on device pointers, asynchronous on `stream`; one-device context.  Workspace and state map as monortm_hip_oe_step_dev (they
 * are shared with it); a call that asks for dofs without avk_diag keeps a diagonal [nprof][nstate] of its own.  After one call, a second
 * of the same shapes, map and outputs allocates and copies nothing (graph capture). */
int monortm_hip_oe_step_full_dev(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate,
                                 const int *state_kind /*host*/, const int *state_row /*host*/, const monortm_real *K_T,
                                 const monortm_real *K_TZ, const monortm_real *K_W, const monortm_real *K_CLW, const monortm_real *K_SFC,
                                 const monortm_real *Y, const monortm_real *y_obs, const monortm_real *x, const monortm_real *xa,
                                 const monortm_real *Sa, int sa_per_profile, const monortm_real *Se, int se_kind, int se_per_profile,
                                 const monortm_real *gamma, monortm_real *x_new, monortm_real *post_var, monortm_real *avk_diag,
                                 monortm_real *chi2, int *status, monortm_real *gain_t, monortm_real *avk, monortm_real *post_cov,
                                 monortm_real *dofs, void *stream);

/* ---- The adaptive retrieval loop: Levenberg-Marquardt step acceptance per profile, on the device.  DESIGN.md section 3.15.
 * The cost J(x) = (y_obs - F(x))^T Se^-1 (y_obs - F(x)) + (x - xa)^T Sa^-1 (x - xa) needs Sa^-1, which never appears here: the iterate
 * carries its dual vector c = Sa^-1 (x - xa) instead.  monortm_hip_oe_step_lm is monortm_hip_oe_step_full with three more arrays:
 *   c               [nprof][nstate], or NULL: 0 (exact at x = xa)
 *   c_new           [nprof][nstate], may be NULL; not c itself.  c_new = (gamma c + K^T M^-1 r) / (1 + gamma) = Sa^-1 (x_new - xa), by
 *                   the step's own algebra; K^T M^-1 r is one more dot product (L^-1 K_:,i) . (L^-1 r) per state, in the order of the others
 *   cost            [nprof], may be NULL: chi2 + sum_i c_i (x_i - xa_i), the cost at x, summed in ascending i
 * A failed profile (status 1) has c_new = c (0 where c is NULL) and cost = 0.  Every other output is what monortm_hip_oe_step_full gives
 * on the same inputs, bit for bit; with c, c_new and cost all NULL the call launches what that entry launches.  c = NULL and c = 0 give
 * the same bits.  Refusals, sharding, workspace and state map as monortm_hip_oe_step_full[_dev]; c_new == c is refused (MONORTM_EARG). */
int monortm_hip_oe_step_lm(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind,
                           const int *state_row, const monortm_real *K_T, const monortm_real *K_TZ, const monortm_real *K_W,
                           const monortm_real *K_CLW, const monortm_real *K_SFC, const monortm_real *Y, const monortm_real *y_obs,
                           const monortm_real *x, const monortm_real *xa, const monortm_real *Sa, int sa_per_profile,
                           const monortm_real *Se, int se_kind, int se_per_profile, const monortm_real *gamma, monortm_real *x_new,
                           monortm_real *post_var, monortm_real *avk_diag, monortm_real *chi2, int *status, monortm_real *gain_t,
                           monortm_real *avk, monortm_real *post_cov, monortm_real *dofs, const monortm_real *c, monortm_real *c_new,
                           monortm_real *cost);
int monortm_hip_oe_step_lm_dev(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate,
                               const int *state_kind /*host*/, const int *state_row /*host*/, const monortm_real *K_T,
                               const monortm_real *K_TZ, const monortm_real *K_W, const monortm_real *K_CLW, const monortm_real *K_SFC,
                               const monortm_real *Y, const monortm_real *y_obs, const monortm_real *x, const monortm_real *xa,
                               const monortm_real *Sa, int sa_per_profile, const monortm_real *Se, int se_kind, int se_per_profile,
                               const monortm_real *gamma, monortm_real *x_new, monortm_real *post_var, monortm_real *avk_diag,
                               monortm_real *chi2, int *status, monortm_real *gain_t, monortm_real *avk, monortm_real *post_cov,
                               monortm_real *dofs, const monortm_real *c, monortm_real *c_new, monortm_real *cost, void *stream);

/* A state vector written into the resident inputs of a batch, checked against a box first.  Device pointers only, asynchronous on
 * `stream`, one launch, one workgroup per profile.  The write map (host int [nstate] each) names the target of every state column:
 *   map_kind        0: T[p][index]   1: TZ[p][index]   2: WKL[p][index][map_mol] = exp(x)   3: CLW[p][index]   4: TMPSFC[p]
 *                   -1: checked against the box but not written (a variable that a later column names again)
 *   map_index       layer (kinds 0, 2, 3) or level (kind 1).  A column is LIVE for profile p where index < nlay[p] (kind 1: index <=
 *                   nlay[p]; kind 4: always).  For kind -1 live means index < nlay[p]: give level - 1 for a level, -1 for TMPSFC.
 *   map_mol         0-based molecule of a kind-2 column
 *   x_src           [nprof][nstate]
 *   x_fallback      [nprof][nstate] or NULL;  done  int [nprof] or NULL
 *   lo, hi          [nstate], or [nprof][nstate] with box_per_profile = 1; each may be NULL (no bound on that side)
 *   nlay            int [nprof]
 *   T, TZ, WKL, CLW with the elements per profile of each (WKL is [..][nmol] within a profile); an array no column writes may be NULL
 *   tmpsfc_a, _b    [nprof] each: both are written by a kind-4 column (one may be NULL)
 *   trial_ok        int [nprof], may be NULL
 * trial_ok[p] = every live element of x_src[p] is finite and inside [lo, hi].  Then the live columns of kind >= 0 are written from
 * x_fallback[p] where that is given and (trial_ok[p] == 0 or done[p] != 0), from x_src[p] otherwise.  Nothing else in the arrays changes.
 * Refused before the launch (MONORTM_EARG): a kind outside -1..4, an index or molecule outside its array or the stride, a written array
 * that is NULL, two written columns with one target, nstate outside 1..2048; real_kind 4 (MONORTM_EUNSUPPORTED).  The device copy of
 * the map is kept like the state map of monortm_hip_oe_step_dev: after one call, a second of the same map allocates and copies nothing.
 * ONE MAP PER CONTEXT, like the state map: a call with another map waits for `stream` (only), replaces the device copy with a blocking
 * copy and may reallocate it.  A captured graph holds the pointer and reads whatever map is there when it replays: while a capture of
 * this entry (or of monortm_hip_oe_step*_dev) is alive, call it on that context with the captured map only.  Callers that alternate
 * between state vectors use one context per state vector. */
int monortm_hip_oe_scatter_dev(void *ctx, int nprof, int nstate, const int *map_kind /*host*/, const int *map_index /*host*/,
                               const int *map_mol /*host*/, const monortm_real *x_src, const monortm_real *x_fallback, const int *done,
                               const monortm_real *lo, const monortm_real *hi, int box_per_profile, const int *nlay, int nlay_max,
                               int nmol, monortm_real *T, long long t_stride, monortm_real *TZ, long long tz_stride, monortm_real *WKL,
                               long long wkl_stride, monortm_real *CLW, long long clw_stride, monortm_real *tmpsfc_a,
                               monortm_real *tmpsfc_b, int *trial_ok, void *stream);

/* The decision on a trial step, per profile: device pointers only, asynchronous on `stream`, one launch, one workgroup per profile, no
 * atomics.  Y_trial [nprof][nmeas] is the forward model at the state the scatter wrote; Se, se_kind, se_per_profile as in
 * monortm_hip_oe_step_full; x_trial, c_trial (the step's x_new, c_new), xa [nprof][nstate]; step_status, trial_ok int [nprof].
 * Loop state, updated in place: x_cur, c_cur [nprof][nstate]; J_cur, gamma [nprof]; done, n_acc, n_rej int [nprof].  Per profile:
 *   done != 0                nothing of the profile changes, bit for bit
 *   step_status == 1         done = 2
 *   otherwise  J_trial = chi2(Y_trial) + sum_i c_trial_i (x_trial_i - xa_i); chi2 as the step forms it (se_kind 1: a bad pivot of Se
 *              gives done = 2); accept = trial_ok && isfinite(J_trial) && J_trial <= J_cur
 *   accept     x_cur = x_trial, c_cur = c_trial, J_cur = J_trial, gamma = gamma down (0 where that is below gamma_floor), n_acc + 1,
 *              done = 1 where the decrease of J is <= conv nmeas
 *   reject     gamma = max(gamma up, gamma_first), n_rej + 1, done = 4 where gamma > gamma_max
 *   last != 0 and done still 0: done = 3
 * done: 0 running, 1 converged, 2 failed step, 3 out of iterations, 4 stalled at gamma_max.  No error of monortm_hip_check.
 * Refused (MONORTM_EARG): nmeas outside 1..128, nstate outside 1..2048, se_kind outside 0..1, a NULL array, up < 1, down outside 0..1,
 * gamma_first <= 0, a negative gamma_floor, gamma_max or conv, a NaN among them; real_kind 4 (MONORTM_EUNSUPPORTED). */
int monortm_hip_oe_accept_dev(void *ctx, int nprof, int nmeas, int nstate, const monortm_real *Y_trial, const monortm_real *y_obs,
                              const monortm_real *Se, int se_kind, int se_per_profile, const monortm_real *x_trial,
                              const monortm_real *c_trial, const monortm_real *xa, const int *step_status, const int *trial_ok, double up,
                              double down, double gamma_first, double gamma_floor, double gamma_max, double conv, int last,
                              monortm_real *x_cur, monortm_real *c_cur, monortm_real *J_cur, monortm_real *gamma, int *done, int *n_acc,
                              int *n_rej, void *stream);

/* Device-side failure flags raised by the kernels of earlier *_dev calls (temperature range, SD-Voigt
 * sign): synchronises `stream`, returns MONORTM_OK or the first error and clears the flags. */
int monortm_hip_check(void *ctx, void *stream);

/* Kernel timing: HIP events recorded on the launch stream around the kernel launches selected by the bit mask
 * `enable` (bit 0 = line sum, bit 1 = continuum+cloud+total, bit 2 = rtm; 0 = off).  Bits 8 and up: sample stride n -
 * only every n-th launch of a selected kernel is bracketed (an event pair keeps the next launch from being queued behind
 * the running kernel, a few microseconds per step; 0 or 1 = every launch).
 * monortm_hip_kernel_time(kernel = 0,1,2) synchronises the recorded events and returns the running totals. */
int monortm_hip_profile(void *ctx, int enable);

/* Measurement switches of a context - how the line-sum launch is shaped.  No reference counterpart (the reference has no
 * tuning knobs on this path); results are the same to rounding whatever is chosen.  The environment variables
 * MONORTM_NSLICE / MONORTM_FAIR / MONORTM_TILE_WAVES / MONORTM_FAR_LEVELS give the defaults once, at monortm_hip_init (a value
 * that does not parse fails the init with MONORTM_EARG).
 *   "nslice" = "auto" | 1..16;  "fair" = "auto" | 0 | 1;  "tile_waves" = "auto" | 1 | 2 | 4;
 *   "far_levels" = "auto" | 0..6: dense grids (>= 4 tiles of wavenumbers) - levels of intervals (tiles, pairs of tiles, fours, eights ...)
 *       whose far lines far_kernel expands before the line sum; 0 = the far field of a tile is formed inside the line-sum kernel;
 *   "lines_kernel" = "auto" | "wn" (the one kernel; the round-3 alternatives "state" / "p" were removed in round 5).
 *   "jac_dt" = "auto" | a finite double > 0 (K; MONORTM_JAC_DT), "jac_dlnw" = "auto" | a finite double in (0, 1) (MONORTM_JAC_DLNW):
 *       the half-steps of the Jacobian's central differences (monortm_hip_jacobian).
 *   "finish" = "auto" | "generic": generic = finish_kernel forms the continuum, cloud and total optical depths also where
 *       finish_mw_kernel would (last wavenumber < 820 cm-1): the A/B switch between the two; MONORTM_FINISH_GENERIC (set to anything)
 *       makes generic the default at monortm_hip_init.
 *   "finish_mw" = "auto" | "layer" | "column" (MONORTM_FINISH_MW): the layout of finish_mw_kernel - a workgroup per (profile, layer), or
 *       per (profile, block of 64 layers) wherever that layout can run (not with line slices summed in the finish kernel, not beyond
 *       40 KB of LDS); auto chooses by batch size.  The outputs are bitwise the same.
 * Values are parsed strictly (whole string, in range).  Unknown names / values: MONORTM_EARG. */
int monortm_hip_set_option(void *ctx, const char *name, const char *value);
int monortm_hip_kernel_time(void *ctx, int kernel, double *total_ms, long long *launches);

#ifdef __cplusplus
}
#endif
#endif
