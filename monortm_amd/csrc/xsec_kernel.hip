// xsec_kernel.hip - optical depth of the cross-section molecules (IXSECT = 1) for gfx950: MONORTM_XSEC_SUB and convolve of the
// reference (src/monortm_sub.F90:1540-1750, :1751-1834) with the tables already parsed (monortm_hip_xsec_tables).
//
// grid = (wavenumbers, layers, profiles); block = one wave.  Everything about a (layer, spectral region) - the temperature
// bracket, the pressure of the blended measurement, the extra Lorentz width hwb, the step of the resampled grid - is
// wave-uniform.  The reference then walks outwards from the wavenumber, one pair of grid points per trip, until a pair adds
// less than ratio x 1e-6 of the running sum (:1797-1817): here the 64 lanes take 64 consecutive trips at once, an inclusive
// scan gives every lane the running sum the sequential walk would hold before its trip, and the first lane whose pair meets
// the criterion ends the walk - the same stopping point (the tail that is cut is NOT negligible, so it has to be the same).
// The resampled spectrum xspd_int (:1779-1785, up to 10^7 points per layer and region in the reference) is never stored:
// a grid value is two table reads per temperature, formed where it is needed.
// The plan and the walk of one (layer, region) are xs_region<0> of xsec_walk.hpp - shared with xsec_jac_kernel.hip, which sums further
// states on the same plan.
#include "xsec_walk.hpp"

namespace {
using namespace monortm_dev;

template <typename R>
__global__ __launch_bounds__(64) void xsec_kernel(ModmArgs a, DevXsec x) {
    const int iw = blockIdx.x, lay = blockIdx.y, prof = blockIdx.z, lane = threadIdx.x;
    const int nwn = a.nwn;
    const size_t pl = (size_t)prof * a.nlay_max + lay;
    R *out = wp<R>(a.ODXSEC) + pl * (size_t)nwn + iw;
    if (lay >= a.nlay[prof]) {
        if (lane == 0) *out = (R)0;
        return;
    }
    const double pave = (double)rp<R>(a.P)[pl], tave = (double)rp<R>(a.T)[pl];
    const double wnv = a.wn[iw];
    const R *xam = rp<R>(a.XAMNT) + pl * (size_t)x.nxs;
    double xstot = 0.;
    XsStates<0> none;
    for (int ixmol = 0; ixmol < x.nxs; ixmol++) {
        double xsmol = 0.;
        for (int r = 0; r < x.nreg; r++) {
            if ((int)x.reg[(size_t)r * 8] != ixmol) continue;
            double res;
            if (!xs_region<0>(x, r, a.wn, nwn, wnv, pave, tave, lane, res, none)) continue;
            xsmol += res;
        }
        xstot += (double)xam[ixmol] * xsmol;   // (:1729-1733)
    }
    if (lane == 0) *out = (R)(xstot * radfn(wnv, tave / K_RADCN2));   // the radiation term back in (:1738-1744)
}

}  // namespace

namespace monortm_dev {
void launch_xsec(const ModmArgs &a, const DevXsec &x, hipStream_t s) {
    const dim3 grid((unsigned)a.nwn, (unsigned)a.nlay_max, (unsigned)a.nprof);
    if (a.real_kind == 4) hipLaunchKernelGGL(xsec_kernel<float>, grid, dim3(64), 0, s, a, x);
    else hipLaunchKernelGGL(xsec_kernel<double>, grid, dim3(64), 0, s, a, x);
}
}  // namespace monortm_dev
