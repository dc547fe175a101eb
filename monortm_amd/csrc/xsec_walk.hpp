// xsec_walk.hpp - one (layer, spectral region) of the cross-section molecules: the plan MONORTM_XSEC_SUB and convolve of the reference
// make from the layer's (P, T) (src/monortm_sub.F90:1645-1716, :1762-1777) and the walk over the resampled spectrum (:1788-1828).
// The ONE definition behind xsec_kernel.hip (NX = 0) and xsec_jac_kernel.hip (NX = 2, 4): xs_region<NX> sums the base state exactly as
// xsec_kernel always has - the same expressions in the same order, so the same bits and the same stopping trip - and, for NX > 0, the
// same finite sum at NX further states (P', T') ON THE BASE STATE'S PLAN: every discrete decision - region
// processed and in range, temperature bracket, the two clamps of hwd, step against delvx, npts, walk or linear branch, ind, the trip
// at which the walk stops - is taken once, from the base (P, T); a further state only changes the continuous quantities coef1 / coef2,
// hwb and the Lorentz weight.  With the discretisation frozen the sum is an analytic function of (P', T'), which is what a
// difference quotient needs; the kernel's own states re-planned at T +- h, P (1 +- eps) are not (npts alone re-grids the spectrum).
//
// 64 lanes take 64 consecutive trips; an inclusive scan gives every lane the running sum of the base state before its trip, the first
// lane that meets the reference's criterion ends the walk (xsec_kernel.hip's header).  A further state keeps one partial sum per
// lane over exactly the trips the base state summed, reduced across the wave once, after the walk.  The two table terms of a grid
// value, d1 / radfn(vv, xkt1) and d2 / radfn(vv, xkt2), do not depend on the state: they are read and divided once per lane and trip;
// a state then costs its coef1 / coef2 and its Lorentz weight.
#pragma once
#include "lineshape.hpp"

namespace monortm_dev {

__device__ __forceinline__ double xs_wave_bcast(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double xs_wave_sum(double v) {   // the same order in every lane and run: lane i + lane i ^ d, d = 32 .. 1
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

struct XsLayer {  // one (layer, region): what :1677-1716 and :1762-1777 leave behind
    double coef1, coef2, xkt1, xkt2, v1x, delvx, step;
    const double *d1, *d2;
    int nptsx;
};
// xspd(i1), i1 1-based (:1711-1715); beyond the data the reference reads static storage that nothing has written: zero
__device__ __forceinline__ double xs_xspd(const XsLayer &q, int i1) {
    if (i1 < 1 || i1 > q.nptsx) return 0.;
    const double vv = q.v1x + (double)(i1 - 1) * q.delvx;
    return q.coef1 * q.d1[i1 - 1] / radfn(vv, q.xkt1) + q.coef2 * q.d2[i1 - 1] / radfn(vv, q.xkt2);
}
// xspd_int(i) = (1-coef) xspd(ind+1) + coef xspd(ind+2), ind = int(i step / delvx)   (:1779-1785)
__device__ __forceinline__ double xs_int(const XsLayer &q, int i) {
    const double vv = q.v1x + (double)i * q.step;
    const double delvv = vv - q.v1x;
    const int ind = (int)(delvv / q.delvx);
    const double cf = (delvv - (double)ind * q.delvx) / q.delvx;
    return (1. - cf) * xs_xspd(q, ind + 1) + cf * xs_xspd(q, ind + 2);
}

// The state-independent halves of the two functions above, for the further states: xspd = coef1 t1 + coef2 t2 with
// t1 = d1 / radfn(vv, xkt1), t2 = d2 / radfn(vv, xkt2).  bracket = false (one table temperature in play: coef2 = 0, d2 = d1): t2 is
// not read and stays 0.
__device__ __forceinline__ void xs_xspd_terms(const XsLayer &q, bool bracket, int i1, double &t1, double &t2) {
    t1 = 0.; t2 = 0.;
    if (i1 < 1 || i1 > q.nptsx) return;
    const double vv = q.v1x + (double)(i1 - 1) * q.delvx;
    t1 = q.d1[i1 - 1] / radfn(vv, q.xkt1);
    if (bracket) t2 = q.d2[i1 - 1] / radfn(vv, q.xkt2);
}
__device__ __forceinline__ void xs_int_terms(const XsLayer &q, bool bracket, int i, double &t1, double &t2) {
    const double vv = q.v1x + (double)i * q.step;
    const double delvv = vv - q.v1x;
    const int ind = (int)(delvv / q.delvx);
    const double cf = (delvv - (double)ind * q.delvx) / q.delvx;
    double a1, a2, b1, b2;
    xs_xspd_terms(q, bracket, ind + 1, a1, a2);
    xs_xspd_terms(q, bracket, ind + 2, b1, b2);
    t1 = (1. - cf) * a1 + cf * b1;
    t2 = (1. - cf) * a2 + cf * b2;
}

// The further states of a cell: their (P', T'), and what xs_region leaves per state
template <int NX>
struct XsStates {
    double p[NX > 0 ? NX : 1], t[NX > 0 ? NX : 1];     // in
    double res[NX > 0 ? NX : 1];                        // out: the region's term at (p, t) on the base plan (0 when out of range)
};

// Region r of the tables for the wavenumber wnv of a layer at (pave, tave).  false: the region is not processed in this call (no
// wavenumber within 1 cm-1 of its FSCDXS bounds, :1645-1653).  true: res = its term of the molecule's sum - 0 where wnv lies outside
// the header's range (:1789-1792) - and, NX > 0, xs.res likewise.  Wave-uniform in everything but the lane.
template <int NX>
__device__ __forceinline__ bool xs_region(const DevXsec &x, int r, const double *wn, int nwn, double wnv, double pave, double tave, int lane,
                                          double &res, XsStates<NX> &xs) {
    const double dvbuf = 1.0, p0 = 1013.;
    const double *rg = x.reg + (size_t)r * 8;
    const double v1fx = rg[1], v2fx = rg[2];   // FSCDXS entry: is the region processed at all (:1645)
    const double v1x = rg[6], v2x = rg[7];     // header of the last file read: the grid and the in-range test (:1663-1666)
    const int nptsx = (int)rg[3], ntemp = (int)rg[4];
    const double xdoplr = rg[5];
    // the region is processed when SOME wavenumber of the call lies within 1 cm-1 of it (:1645-1653)
    // (the wavenumbers ascend - modm.f90:180-181, checked by lines_kernel - so the first one at or above the lower bound
    // decides: a binary search instead of a scan of all nwn values per workgroup and region)
    int lo = 0, hi = nwn;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (wn[mid] < v1fx - dvbuf) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= nwn || !(wn[lo] <= v2fx + dvbuf)) return false;
    res = 0.;
    if constexpr (NX > 0) {
#pragma unroll
        for (int s = 0; s < NX; s++) xs.res[s] = 0.;
    }
    if (!(wnv < v1x || wnv > v2x)) {  // (:1789-1792)
        const double *tx = x.temps + (size_t)r * 6, *pdx = x.pres + (size_t)r * 6;
        // temperature bracket, the tables are in ascending temperature (:1677-1704)
        double coef1 = 1., coef2 = 0.;
        int ind1, ind2 = 1, it = 1;
        bool bracket = false;
        if (ntemp == 1 || tave <= tx[it - 1]) ind1 = 1;
        else {
            for (;;) {
                it = it + 1;
                if (it > ntemp) { ind1 = ntemp; ind2 = ntemp; break; }
                else if (tave <= tx[it - 1]) {
                    ind1 = it - 1; ind2 = it;
                    coef1 = (tave - tx[it - 1]) / (tx[it - 2] - tx[it - 1]);
                    coef2 = 1. - coef1;
                    bracket = true;
                    break;
                }
            }
        }
        const double pd = coef1 * pdx[ind1 - 1] + coef2 * pdx[ind2 - 1];
        XsLayer q;
        q.coef1 = coef1; q.coef2 = coef2;
        q.xkt1 = tx[ind1 - 1] / K_RADCN2; q.xkt2 = tx[ind2 - 1] / K_RADCN2;
        q.v1x = v1x; q.nptsx = nptsx;
        q.delvx = (v2x - v1x) / (double)(nptsx - 1);
        q.d1 = x.pool + x.offs[(size_t)r * 6 + ind1 - 1];
        q.d2 = x.pool + x.offs[(size_t)r * 6 + ind2 - 1];
        const double hwdop = xdoplr * sqrt(tave / 296.);
        // convolve: half widths, step of the resampled grid (:1762-1777)
        double hwpave = 0.1 * (pave / p0) * (273.15 / tave);
        double hwd = 0.1 * (pd / p0) * (273.15 / tave);
        const bool dop = hwdop > hwd;            // the two clamps, as decisions: what a further state keeps
        hwd = fmax(hwd, hwdop);
        const bool widen = hwd > hwpave;
        if (hwd > hwpave) hwpave = 1.001 * hwd;
        const double hwb = hwpave - hwd;
        double ratio = 0.25, step = ratio * hwb;
        if (step > q.delvx) step = q.delvx;
        const int npts = (int)((v2x - v1x) / step);
        step = (v2x - v1x) / (double)npts;
        ratio = step / hwb;
        q.step = step;
        // the further states on this plan: the bracket's linear form at T' (extrapolated where T' leaves it, constant where the base
        // has none), the clamps as the base took them; step, npts and ind are the base's
        double c1x[NX > 0 ? NX : 1], c2x[NX > 0 ? NX : 1], hwbx[NX > 0 ? NX : 1];
        if constexpr (NX > 0) {
#pragma unroll
            for (int s = 0; s < NX; s++) {
                const double ts = xs.t[s], ps = xs.p[s];
                c1x[s] = 1.; c2x[s] = 0.;
                if (bracket) {
                    c1x[s] = (ts - tx[ind2 - 1]) / (tx[ind1 - 1] - tx[ind2 - 1]);
                    c2x[s] = 1. - c1x[s];
                }
                const double pds = c1x[s] * pdx[ind1 - 1] + c2x[s] * pdx[ind2 - 1];
                double hwps = 0.1 * (ps / p0) * (273.15 / ts);
                double hwds = 0.1 * (pds / p0) * (273.15 / ts);
                if (dop) hwds = xdoplr * sqrt(ts / 296.);
                if (widen) hwps = 1.001 * hwds;
                hwbx[s] = hwps - hwds;
            }
        }
        if (hwb / hwd > 0.1) {
            // Lorentzian of width hwb over the resampled spectrum (:1788-1821)
            const double hwb2 = hwb * hwb;
            const double wn_v1x = wnv - v1x;
            const int ind = (int)(wn_v1x / step);
            const double dvlo0 = wnv - (v1x + (double)ind * step), dvhi0 = wnv - (v1x + (double)(ind + 1) * step);
            double answer = (hwb / (hwb2 + dvlo0 * dvlo0)) * xs_int(q, ind) + (hwb / (hwb2 + dvhi0 * dvhi0)) * xs_int(q, ind + 1);
            double ans0x[NX > 0 ? NX : 1], accx[NX > 0 ? NX : 1];   // a further state: the first pair (uniform), this lane's trips
            if constexpr (NX > 0) {
                double a1, a2, b1, b2;
                xs_int_terms(q, bracket, ind, a1, a2);
                xs_int_terms(q, bracket, ind + 1, b1, b2);
#pragma unroll
                for (int s = 0; s < NX; s++) {
                    const double h = hwbx[s], h2 = h * h;
                    ans0x[s] = (h / (h2 + dvlo0 * dvlo0)) * (c1x[s] * a1 + c2x[s] * a2) + (h / (h2 + dvhi0 * dvhi0)) * (c1x[s] * b1 + c2x[s] * b2);
                    accx[s] = 0.;
                }
            }
            const double thr = ratio * 1e-6;
            for (int jb = 0;; jb += 64) {
                const int j = jb + lane + 1;
                double contlo = 0., conthi = 0.;
                double incx[NX > 0 ? NX : 1];
                if constexpr (NX > 0) {
#pragma unroll
                    for (int s = 0; s < NX; s++) incx[s] = 0.;
                }
                const double vlo = v1x + (double)(ind - j) * step;
                if (vlo > v1x) {
                    const double dvlo = wnv - vlo;
                    contlo = (hwb / (hwb2 + dvlo * dvlo)) * xs_int(q, ind - j);
                    if constexpr (NX > 0) {
                        double t1, t2;
                        xs_int_terms(q, bracket, ind - j, t1, t2);
#pragma unroll
                        for (int s = 0; s < NX; s++) incx[s] += (hwbx[s] / (hwbx[s] * hwbx[s] + dvlo * dvlo)) * (c1x[s] * t1 + c2x[s] * t2);
                    }
                }
                const double vhi = v1x + (double)(ind + j + 1) * step;
                if (vhi < v2x) {
                    const double dvhi = wnv - vhi;
                    conthi = (hwb / (hwb2 + dvhi * dvhi)) * xs_int(q, ind + j + 1);
                    if constexpr (NX > 0) {
                        double t1, t2;
                        xs_int_terms(q, bracket, ind + j + 1, t1, t2);
#pragma unroll
                        for (int s = 0; s < NX; s++) incx[s] += (hwbx[s] / (hwbx[s] * hwbx[s] + dvhi * dvhi)) * (c1x[s] * t1 + c2x[s] * t2);
                    }
                }
                const double xincr = contlo + conthi;
                // running sum BEFORE this lane's trip: answer + the trips of the lanes below (inclusive scan, then shift)
                double incl = xincr;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const double up = __shfl_up(incl, d);
                    if (lane >= d) incl += up;
                }
                const double before = answer + (incl - xincr);
                const unsigned long long stop = __ballot((xincr / before) < thr);
                if (stop != 0ull) {
                    const int first = (int)__builtin_ctzll(stop);
                    answer = xs_wave_bcast(before, first);
                    if constexpr (NX > 0) {   // the trips the base state summed: those of the lanes below the first that stops
#pragma unroll
                        for (int s = 0; s < NX; s++)
                            if (lane < first) accx[s] += incx[s];
                    }
                    break;
                }
                answer = xs_wave_bcast(answer + incl, 63);
                if constexpr (NX > 0) {
#pragma unroll
                    for (int s = 0; s < NX; s++) accx[s] += incx[s];
                }
                // past both ends of the spectrum every later pair is zero: the reference would spin on 0/0 when the sum
                // itself is zero (no data) - every wave leaves here
                if (ind - (jb + 64) < 0 && ind + jb + 65 > npts) break;
            }
            res = answer * step / 3.14159;   // (:1820; the reference's own value of pi here)
            if constexpr (NX > 0) {
#pragma unroll
                for (int s = 0; s < NX; s++) xs.res[s] = (ans0x[s] + xs_wave_sum(accx[s])) * step / 3.14159;
            }
        } else {
            // linearly interpolated values (:1822-1828) - with xspd(ind), xspd(ind+1): one element below the convention of
            // the resampling above, as the reference has it
            const double wn_v1x = wnv - v1x;
            const int ind = (int)(wn_v1x / q.delvx);
            const double coef = (wn_v1x - (double)ind * q.delvx) / q.delvx;
            res = (1. - coef) * xs_xspd(q, ind) + coef * xs_xspd(q, ind + 1);
            if constexpr (NX > 0) {
                double a1, a2, b1, b2;
                xs_xspd_terms(q, bracket, ind, a1, a2);
                xs_xspd_terms(q, bracket, ind + 1, b1, b2);
#pragma unroll
                for (int s = 0; s < NX; s++) xs.res[s] = (1. - coef) * (c1x[s] * a1 + c2x[s] * a2) + coef * (c1x[s] * b1 + c2x[s] * b2);
            }
        }
    }
    return true;
}

}  // namespace monortm_dev
