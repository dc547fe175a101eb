// obs_exchange.hpp - lanes -> channels: what the kernels that contract with a measurement operator share (rtm_obs_jac_kernel.hip,
// rtm_obs_kernel.hip; DESIGN.md sections 3.9 and 3.10).  One definition, so that the forward operator's Y and the adjoint's Y have the
// same owner thread and the same order of additions.
#pragma once
#include "device_common.hpp"

namespace {

constexpr int OBS_SLAB = 4;   // rows of a wave's LDS slab: fields that change lanes for channels in one exchange

// A wave is one layer group: what its lanes leave in the wave's own slab is read by other lanes of the SAME wave only.  The LDS serves a
// wave's accesses in program order, so a fence of wavefront scope (which keeps the compiler from moving the accesses) is all it takes.
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lanes -> channels.  Every lane leaves its NF values (sums over the tile's paths, one wavenumber each) in the wave's slab; the owner
// lane of channel c (c mod 64) adds the members of c in this wavenumber block, in ascending wavenumber, times wchan, and adds the sum
// to dst[f][c] - a plain read-modify-write by the one thread that owns the element for the whole launch.  ms: the block's row of the
// membership table (ms[c] .. ms[c + 1]: the members of c), mb = ms[0]; sMl / sMw: lane and weight of the block's members (LDS).
// Called by whole waves (all 64 lanes, wave-uniform control flow).
template <typename A, int NF>
__device__ __forceinline__ void to_channels(double *slab, const double (&v)[NF], int nchan, const int *ms, int mb, const int *sMl,
                                            const double *sMw, A *const (&dst)[NF], int lane) {
    static_assert(NF <= OBS_SLAB, "slab rows");
#pragma unroll
    for (int f = 0; f < NF; f++) slab[f * 64 + lane] = v[f];
    wave_fence();
    for (int c = lane; c < nchan; c += 64) {
        const int m0 = ms[c] - mb, m1 = ms[c + 1] - mb;
        if (m1 > m0) {
            double s[NF];
#pragma unroll
            for (int f = 0; f < NF; f++) s[f] = 0.;
            for (int m = m0; m < m1; m++) {
                const int ml = sMl[m];
                const double w = sMw[m];
#pragma unroll
                for (int f = 0; f < NF; f++) s[f] = fma(w, slab[f * 64 + ml], s[f]);
            }
#pragma unroll
            for (int f = 0; f < NF; f++) dst[f][c] = (A)((double)dst[f][c] + s[f]);
        }
    }
    wave_fence();
}

}  // namespace
