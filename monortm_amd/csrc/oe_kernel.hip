// oe_kernel.hip - the optimal-estimation step, gfx950, real_kind 8.  No reference counterpart.
//
// One Gauss-Newton / Levenberg-Marquardt update of Rodgers' m-form per profile, from the K arrays of monortm_hip_obs_jacobian read in
// place through a state map (n states, m = nview x nchan measurements, g = 1 / (1 + gamma)):
//   d' = (xa - x) g,  W = g Sa K^T,  M = K W + diag(se) = L L^T,  u = L^-1 ((y - F) - K d'),
//   a_i = L^-1 W_i,  b_i = L^-1 K_:,i,   x_new_i = x_i + d'_i + a_i . u   ( = x + d' + W M^-1 r: the back substitution is never formed),
//   post_var_i = Sa_ii g - a_i . a_i,  avk_diag_i = a_i . b_i,  chi2 = sum_j (y_j - F_j)^2 / se_j.
//
// grid = profiles, block = 256 threads, one launch.  Nothing leaves the workgroup, there are no atomics, and every sum is formed by ONE
// thread in ascending order of its index: the same bits on repeated calls, and for a profile alone and inside a batch.
//   0  gather    K^T -> B [m][n] of the profile's workspace (thread per element; reads contiguous in the channel)
//   1  W         thread per state i, OE_JB measurements in registers: W[j][i] = g sum_s Sa(i, s) B[j][s], s ascending.  Sa(i, s) is read
//                from the lower triangle only - row i up to the diagonal, column i of the rows below it (those reads are coalesced)
//   2  M, r      M[j][j'] = sum_i B[j][i] W[j'][i] (+ se_j) into the packed lower triangle in LDS: a 16 x 16 thread block, up to 36
//                elements per thread in registers, B and W through LDS in tiles of 16 states; thread per r_j
//   3  Cholesky  right-looking, in LDS, two barriers per column; r rides along as one more row, which leaves u = L^-1 r.  A pivot that is
//                <= 0 or not finite, a non-finite r_j, a negative or non-finite gamma: the profile is marked (status 1, x_new = x, the
//                diagnostics 0) and the arithmetic runs on with harmless values - no barrier is skipped
//   4  solves    thread per state i: a_i and b_i by forward substitution, OE_KB rows at a time, in place over W and B (coalesced in i), L
//                broadcast from LDS; the three dot products are accumulated as the rows are finished
// Workspace: [nprof][2][m][n] doubles (B and W; W does not fit LDS - 2048 x 128 doubles - and phase 4 needs the history of both).
#include <algorithm>

#include "device_common.hpp"

namespace {
using namespace monortm_dev;

constexpr int OE_THREADS = 256, OE_ST = 8, OE_JB = 16, OE_KB = 4, OE_IT = 16, OE_ITP = OE_IT + 1, OE_MB = 8;   // (16 OE_MB = the largest m)

__device__ __forceinline__ int tri(int i) { return i * (i + 1) / 2; }

__global__ __launch_bounds__(OE_THREADS) void oe_step_kernel(OeArgs a) {
    extern __shared__ __attribute__((aligned(16))) double oe_lds[];
    __shared__ int sBad;
    const int p = blockIdx.x, tid = threadIdx.x, m = a.nmeas, n = a.nstate;
    const int ntri = tri(m);
    double *sM = oe_lds;         // [m (m + 1) / 2] packed lower triangle: M, then L
    double *sU = sM + ntri;      // [m] r, then u = L^-1 r
    int *sJo = reinterpret_cast<int *>(sM);   // phase 0 only: [5][m] offset of measurement j within a profile's K array of each kind
    const size_t mn = (size_t)m * n;
    double *B = a.ws + (size_t)p * 2 * mn, *W = B + mn;
    const double gam = a.gamma ? a.gamma[p] : 0.;
    const bool gam_ok = gam >= 0. && isfinite(gam);
    const double ginv = gam_ok ? 1. / (1. + gam) : 1.;
    const double *x = a.x + (size_t)p * n, *xa = a.xa + (size_t)p * n;
    const double *Sa = a.Sa + (a.sa_per_profile ? (size_t)p * n * n : 0);
    const double *se = a.se + (a.se_per_profile ? (size_t)p * m : 0);
    const double *Y = a.Y + (size_t)p * m, *yo = a.y_obs + (size_t)p * m;
    if (tid == 0) sBad = gam_ok ? 0 : 1;

    // ---- 0: gather K through the state map
    for (int e = tid; e < 5 * m; e += OE_THREADS) {
        const int k = e / m, j = e - k * m;
        sJo[e] = (j / a.nchan) * a.vstride[k] + j % a.nchan;
    }
    __syncthreads();
    for (size_t e = tid; e < mn; e += OE_THREADS) {
        const int s = (int)(e / m), j = (int)(e - (size_t)s * m);
        const int k = a.map[s];
        B[(size_t)j * n + s] = a.K[k][(size_t)p * a.kstride[k] + a.map[n + s] + sJo[k * m + j]];
    }
    __syncthreads();

    // ---- 1: W = g Sa K^T
    for (int i0 = 0; i0 < n; i0 += OE_THREADS) {
        const int i = i0 + tid;
        if (i >= n) break;   // (no barrier inside this phase)
        for (int j0 = 0; j0 < m; j0 += OE_JB) {
            double acc[OE_JB];
#pragma unroll
            for (int r = 0; r < OE_JB; r++) acc[r] = 0.;
            for (int s0 = 0; s0 < n; s0 += OE_ST) {
                const int sn = min(OE_ST, n - s0);
                double sa[OE_ST];
#pragma unroll
                for (int q = 0; q < OE_ST; q++) {
                    const int s = min(s0 + q, n - 1);
                    sa[q] = Sa[s <= i ? (size_t)i * n + s : (size_t)s * n + i];
                }
#pragma unroll
                for (int q = 0; q < OE_ST; q++) {
                    if (q < sn) {
#pragma unroll
                        for (int r = 0; r < OE_JB; r++) acc[r] += sa[q] * B[(size_t)min(j0 + r, m - 1) * n + s0 + q];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < OE_JB; r++)
                if (j0 + r < m) W[(size_t)(j0 + r) * n + i] = acc[r] * ginv;
        }
    }
    __syncthreads();

    // ---- 2: M = K W + diag(se), r = (y - F) - K d'
    // Thread (ty, tx) of the 16 x 16 block owns M[ty + 16 a][tx + 16 b], b <= a, in registers; B and W pass through LDS in tiles of OE_IT
    // states (rows padded to OE_ITP doubles: the 16 rows a wave reads of W fall into 16 different bank pairs).  The tiles lie where M
    // will: M is written when the last tile has been consumed.  Every element is still one thread's sum in ascending i.
    const int tx = tid & 15, ty = tid >> 4;
    {
        double acc[OE_MB * (OE_MB + 1) / 2];
#pragma unroll
        for (int q = 0; q < OE_MB * (OE_MB + 1) / 2; q++) acc[q] = 0.;
        double *sB = oe_lds, *sW = oe_lds + m * OE_ITP;
        for (int i0 = 0; i0 < n; i0 += OE_IT) {
            __syncthreads();   // the tile before is consumed
            for (int e = tid; e < m * OE_IT; e += OE_THREADS) {
                const int j = e / OE_IT, ii = e % OE_IT, i = i0 + ii;
                sB[j * OE_ITP + ii] = i < n ? B[(size_t)j * n + i] : 0.;
                sW[j * OE_ITP + ii] = i < n ? W[(size_t)j * n + i] : 0.;
            }
            __syncthreads();
            for (int ii = 0; ii < OE_IT; ii++) {
                double bv[OE_MB], wv[OE_MB];
#pragma unroll
                for (int a2 = 0; a2 < OE_MB; a2++) {
                    if (16 * a2 < m) {
                        bv[a2] = sB[min(ty + 16 * a2, m - 1) * OE_ITP + ii];
                        wv[a2] = sW[min(tx + 16 * a2, m - 1) * OE_ITP + ii];
#pragma unroll
                        for (int b2 = 0; b2 <= a2; b2++) acc[a2 * (a2 + 1) / 2 + b2] += bv[a2] * wv[b2];
                    }
                }
            }
        }
        __syncthreads();   // the last tile is consumed: M may take its place
#pragma unroll
        for (int a2 = 0; a2 < OE_MB; a2++)
#pragma unroll
            for (int b2 = 0; b2 <= a2; b2++) {
                const int j = ty + 16 * a2, jp = tx + 16 * b2;
                if (j < m && jp <= j) sM[tri(j) + jp] = j == jp ? acc[a2 * (a2 + 1) / 2 + b2] + se[j] : acc[a2 * (a2 + 1) / 2 + b2];
            }
    }
    if (tid < m) {
        const double *bj = B + (size_t)tid * n;
        double r = yo[tid] - Y[tid];
        for (int s = 0; s < n; s++) r -= bj[s] * ((xa[s] - x[s]) * ginv);
        sU[tid] = r;
        if (!isfinite(r)) sBad = 1;
    }
    __syncthreads();

    // ---- 3: Cholesky in place, u = L^-1 r as row m
    for (int k = 0; k < m; k++) {
        const int kk = tri(k) + k;
        double d = sM[kk];
        if (!(d > 0. && isfinite(d))) {
            if (tid == 0) sBad = 1;
            d = 1.;
        }
        const double lkk = sqrt(d);
        for (int i = k + 1 + tid; i < m; i += OE_THREADS) sM[tri(i) + k] /= lkk;
        if (tid == OE_THREADS - 1) sU[k] /= lkk;
        __syncthreads();   // column k of L and u_k are final; everyone has read the pivot
        if (tid == 0) sM[kk] = lkk;
        for (int i = k + 1 + ty; i < m; i += 16) {
            const double lik = sM[tri(i) + k];
            for (int j = k + 1 + tx; j <= i; j += 16) sM[tri(i) + j] -= lik * sM[tri(j) + k];
        }
        for (int j = k + 1 + tid; j < m; j += OE_THREADS) sU[j] -= sM[tri(j) + k] * sU[k];
        __syncthreads();
    }
    const bool bad = sBad != 0;
    if (tid == 0) {
        double c2 = 0.;
        if (!bad)
            for (int j = 0; j < m; j++) {
                const double dy = yo[j] - Y[j];
                c2 += dy * dy / se[j];
            }
        if (a.chi2) a.chi2[p] = c2;
        a.status[p] = bad ? 1 : 0;
    }

    // ---- 4: the states
    for (int i = tid; i < n; i += OE_THREADS) {
        const size_t o = (size_t)p * n + i;
        if (bad) {
            a.x_new[o] = x[i];
            if (a.post_var) a.post_var[o] = 0.;
            if (a.avk_diag) a.avk_diag[o] = 0.;
            continue;
        }
        double pv = 0., av = 0., dx = 0.;
        for (int kb = 0; kb < m; kb += OE_KB) {
            double aw[OE_KB], ab[OE_KB];
            int row[OE_KB];
#pragma unroll
            for (int r = 0; r < OE_KB; r++) {
                const int k = min(kb + r, m - 1);
                row[r] = tri(k);
                aw[r] = W[(size_t)k * n + i];
                ab[r] = B[(size_t)k * n + i];
            }
            for (int t = 0; t < kb; t++) {
                const double at = W[(size_t)t * n + i], bt = B[(size_t)t * n + i];
#pragma unroll
                for (int r = 0; r < OE_KB; r++) {
                    const double l = sM[row[r] + t];
                    aw[r] -= l * at;
                    ab[r] -= l * bt;
                }
            }
#pragma unroll
            for (int r = 0; r < OE_KB; r++) {
                if (kb + r < m) {
#pragma unroll
                    for (int q = 0; q < r; q++) {
                        const double l = sM[row[r] + kb + q];
                        aw[r] -= l * aw[q];
                        ab[r] -= l * ab[q];
                    }
                    const double lkk = sM[row[r] + kb + r];
                    aw[r] /= lkk;
                    ab[r] /= lkk;
                    W[(size_t)(kb + r) * n + i] = aw[r];
                    B[(size_t)(kb + r) * n + i] = ab[r];
                    pv += aw[r] * aw[r];
                    av += aw[r] * ab[r];
                    dx += aw[r] * sU[kb + r];
                }
            }
        }
        a.x_new[o] = x[i] + (xa[i] - x[i]) * ginv + dx;
        if (a.post_var) a.post_var[o] = Sa[(size_t)i * n + i] * ginv - pv;
        if (a.avk_diag) a.avk_diag[o] = av;
    }
}

}  // namespace

namespace monortm_dev {
// M - or, before it, the two tiles of phase 2 and the offset table of phase 0, whichever is largest - and r / u
static size_t oe_lds_bytes(int nmeas) {
    const size_t m = (size_t)nmeas;
    return sizeof(double) * (std::max(std::max(m * (m + 1) / 2, 2 * m * OE_ITP), (5 * m + 1) / 2) + m);
}

hipError_t launch_oe_step(const OeArgs &a, hipStream_t s) {
    const size_t lds = oe_lds_bytes(a.nmeas);
    if (lds > (64u << 10)) {   // m >= 127: beyond the default bound of a launch's dynamic LDS
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(oe_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(oe_step_kernel, dim3((unsigned)a.nprof), dim3(OE_THREADS), lds, s, a);
    return hipGetLastError();
}
}  // namespace monortm_dev
