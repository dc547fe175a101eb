// cloud_tkc.hpp - ODCLW_TKC (src/CloudOptProp.f90:29-157): optical depth of cloud liquid, linear in CLW.  Used by the finish
// kernels of MODM (continuum_kernel.hip) and, with CLW = 1, as dO/dCLW by the Jacobian (jacobian_kernel.hip).  Internal linkage in
// every translation unit that includes it, as when it was defined inside continuum_kernel.hip.
#pragma once
#include "lineshape.hpp"

namespace {
using namespace monortm_dev;

__device__ double odclw_tkc(double WN, double TEMP, double CLW) {  // src/CloudOptProp.f90:29-157
    const double Hz_per_GHz = 1.e9, cm_per_m = 100.;
    const double a_1 = 8.110808E+01, b_1 = 4.433736E-03, c_1 = 1.301700E-13, d_1 = 6.627126E+02, a_2 = 2.025164E+00,
                 b_2 = 1.072976E-02, c_2 = 1.011945E-14, d_2 = 6.089168E+02, t_c = 1.342433E+02;
    double freq = WN * K_CLIGHT / Hz_per_GHz;
    double temp = TEMP - 273.15;
    double frq = freq * Hz_per_GHz;
    double cl = K_CLIGHT / cm_per_m;
    double eps_s = 87.9144 - 0.404399 * temp + 9.58726e-4 * (temp * temp) - 1.32802e-6 * (temp * temp * temp);
    double delta_1 = a_1 * exp(-b_1 * temp), tau_1 = c_1 * exp(d_1 / (temp + t_c));
    double delta_2 = a_2 * exp(-b_2 * temp), tau_2 = c_2 * exp(d_2 / (temp + t_c));
    double w1 = 2. * K_PI * frq * tau_1, w2 = 2. * K_PI * frq * tau_2, w = 2. * K_PI * frq;
    double t1 = (tau_1 * tau_1 * delta_1) / (1. + w1 * w1);
    double t2 = (tau_2 * tau_2 * delta_2) / (1. + w2 * w2);
    double eps1 = eps_s - (w * w) * (t1 + t2);
    t1 = (tau_1 * delta_1) / (1. + w1 * w1);
    t2 = (tau_2 * delta_2) / (1. + w2 * w2);
    double eps2 = w * (t1 + t2);
    cx eps = cmk(eps1, eps2);
    cx RE = (cmk(eps1 - 1., eps2)) / (2. + eps);
    double alpha = 6. * K_PI * RE.im * frq * 1.e-3 / cl;
    return alpha * CLW;
}

}  // namespace
