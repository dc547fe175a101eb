// xsec_jac_kernel.hip - the cross-section molecules in the Jacobians, gfx950, real_kind 8.
//
// ODXSEC of the states T +- h and P (1 +- eps) of a full Jacobian call, and each named molecule's own term, in ONE pass over the base
// state's walk.  Differences of xsec_kernel re-run at the perturbed states are unusable: npts = int((v2x - v1x) / step) re-grids the
// whole spectrum when P or T moves, the stopping trip, the temperature bracket, the two clamps of hwd, the walk / linear branch and
// step > delvx move with them, and central differences at h and 2h then disagree in 36 - 58 % of the cells.  Here every one of those
// decisions is taken once, from the base (P, T), by the very code xsec_kernel runs (xs_region of xsec_walk.hpp, NX = 0 there); the
// further states are the same finite sum evaluated at (P', T'), an analytic function of them.
//
// grid = (wavenumbers, layers, profiles); block = one wave, as xsec_kernel.  Outputs, lane 0:
//   ODX [slot][nprof][nlay_max][nwn]   the sum over all molecules at each further state, times that state's radfn(wn, T' / RADCN2)
//   xO + kplus[x] stride               for a named molecule x: 2 eps XAMNT(k, x) sigma_x radfn of the BASE state - O is linear in the
//                                      amounts, so d O / d ln XAMNT is the molecule's own term and nothing is differenced; the adjoint
//                                      kernels form (O+ - O-) / (2 eps), and the caller clears O- (the XRAYL pattern, section 3.11)
// Padding layers: 0 everywhere.  No atomics, no LDS.
#include "xsec_walk.hpp"

namespace {
using namespace monortm_dev;

template <int NX>
__global__ __launch_bounds__(64) void xsec_jac_kernel(XsecJacArgs a, DevXsec x) {
    const int iw = blockIdx.x, lay = blockIdx.y, prof = blockIdx.z, lane = threadIdx.x;
    const int nwn = a.nwn;
    const size_t npl = (size_t)a.nprof * a.nlay_max, pl = (size_t)prof * a.nlay_max + lay, cell = pl * (size_t)nwn + iw;
    if (lay >= a.nlay[prof]) {
        if (lane == 0) {
#pragma unroll
            for (int s = 0; s < NX; s++) a.ODX[(size_t)a.oslot[s] * a.stride + cell] = 0.;
            for (int m = 0; m < x.nxs; m++)
                if (a.kplus[m]) a.xO[(size_t)a.kplus[m] * a.stride + cell] = 0.;
        }
        return;
    }
    const double pave = a.P[pl], tave = a.T[pl];
    const double wnv = a.wn[iw];
    const double *xam = a.XAMNT + pl * (size_t)x.nxs;
    XsStates<NX> xs;
#pragma unroll
    for (int s = 0; s < NX; s++) {
        xs.p[s] = a.xP[(size_t)a.pstate[s] * npl + pl];
        xs.t[s] = a.xT[(size_t)a.pstate[s] * npl + pl];
    }
    const double rf = radfn(wnv, tave / K_RADCN2);
    double tot[NX];
#pragma unroll
    for (int s = 0; s < NX; s++) tot[s] = 0.;
    for (int ixmol = 0; ixmol < x.nxs; ixmol++) {
        double xsmol = 0., xsm[NX];
#pragma unroll
        for (int s = 0; s < NX; s++) xsm[s] = 0.;
        for (int r = 0; r < x.nreg; r++) {
            if ((int)x.reg[(size_t)r * 8] != ixmol) continue;
            double res;
            if (!xs_region<NX>(x, r, a.wn, nwn, wnv, pave, tave, lane, res, xs)) continue;
            xsmol += res;
#pragma unroll
            for (int s = 0; s < NX; s++) xsm[s] += xs.res[s];
        }
        const double xa = xam[ixmol];
#pragma unroll
        for (int s = 0; s < NX; s++) tot[s] += xa * xsm[s];
        if (a.kplus[ixmol] && lane == 0) a.xO[(size_t)a.kplus[ixmol] * a.stride + cell] = a.two_eps * (xa * xsmol * rf);
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NX; s++) a.ODX[(size_t)a.oslot[s] * a.stride + cell] = tot[s] * radfn(wnv, xs.t[s] / K_RADCN2);
    }
}

}  // namespace

namespace monortm_dev {
void launch_xsec_jac(const XsecJacArgs &a, const DevXsec &x, hipStream_t s) {
    const dim3 grid((unsigned)a.nwn, (unsigned)a.nlay_max, (unsigned)a.nprof);
    if (a.nx == 4) hipLaunchKernelGGL(xsec_jac_kernel<4>, grid, dim3(64), 0, s, a, x);
    else hipLaunchKernelGGL(xsec_jac_kernel<2>, grid, dim3(64), 0, s, a, x);
}
}  // namespace monortm_dev
