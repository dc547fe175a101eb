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
//
// The full entries (monortm_hip_oe_step_full[_dev]) launch other instantiations of the same kernel:
//   SEFULL  Se [m][m], lower triangle read.  Between phases 0 and 1, while nothing else needs the LDS, Se is factored there by the
//           Cholesky of phase 3 with y - F as the extra row: chi2 = |L_e^-1 (y - F)|^2, summed by thread 0 in ascending j.  A bad pivot of
//           Se marks the profile like one of M.  Phase 2 adds Se[j][j'] to every element of M's triangle.
//   GAIN    5  gain  thread per state i, L still in LDS: G^T = L^-T a, gain_t[k][i] = (a[k][i] - sum_{t > k} L[t][k] gain_t[t][i]) / L[k][k]
//           for k = m - 1 .. 0, t descending, OE_KB rows at a time; a thread reads back only what it stored itself
// and, with dofs, thread 0 sums avk_diag in ascending i.  After the launch the workspace holds b = L^-1 K and a = L^-1 W^T.
// oe_cov_kernel, a second launch on the same stream, turns them into the matrices: avk = a^T b, post_cov = g Sa - a^T a.
// grid = (64 x 64 output tiles, profiles), 256 threads, a 4 x 4 register block per thread and matrix; the a- and b-rows pass through LDS
// in slabs of OE_CK measurements, laid out [k][64 states]: a wave reads 16 consecutive doubles of one slab row and 4 more as broadcasts,
// which fall into different bank pairs without the padding the [j][OE_ITP] tiles of phase 2 need.  Every element is one thread's sum in
// ascending k, formed with the fused multiply-adds phase 4 compiles to: diag(post_cov) and diag(avk) are post_var and avk_diag bit for
// bit.  post_cov is computed on and below the diagonal tiles and stored with its mirror image; Sa is read from its lower triangle.
//
// The adaptive loop (monortm_hip_oe_step_lm[_dev], monortm_hip_oe_scatter_dev, monortm_hip_oe_accept_dev):
//   DUAL    the iterate carries c = Sa^-1 (x - xa).  Phase 4 accumulates one more dot product, q_i = b_i . u = (K^T M^-1 r)_i, in the
//           order of the other three, and stores c_new_i = g (gamma c_i + q_i) = Sa^-1 (x_new - xa)_i; thread 0 stores the cost at x,
//           chi2 + sum_i c_i (x_i - xa_i), i ascending, behind the barrier of dofs.  A failed profile: c_new = c, cost = 0.  The
//           instantiations without DUAL compile from the expressions they had, in their order.
// oe_scatter_kernel writes a state vector into the resident inputs through a write map, after a box test; oe_accept_kernel forms the
// cost of the trial and decides per profile.  One workgroup per profile each, no atomics.
#include <algorithm>

#include "device_common.hpp"

namespace {
using namespace monortm_dev;

constexpr int OE_THREADS = 256, OE_ST = 8, OE_JB = 16, OE_KB = 4, OE_IT = 16, OE_ITP = OE_IT + 1, OE_MB = 8;   // (16 OE_MB = the largest m)
constexpr int OE_CT = 64, OE_CR = 4, OE_CK = 16;   // oe_cov_kernel: tile edge, register block edge (16 OE_CR = OE_CT), slab depth

__device__ __forceinline__ int tri(int i) { return i * (i + 1) / 2; }

// Cholesky in place on the packed lower triangle sM, right-looking, two barriers per column; sU rides along as row m, which leaves
// L^-1 sU.  A pivot that is <= 0 or not finite sets *sBad and is replaced by 1: no barrier is skipped.  Ends on a barrier.
__device__ __forceinline__ void oe_cholesky(double *sM, double *sU, int m, int tid, int tx, int ty, int *sBad) {
    for (int k = 0; k < m; k++) {
        const int kk = tri(k) + k;
        double d = sM[kk];
        if (!(d > 0. && isfinite(d))) {
            if (tid == 0) *sBad = 1;
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
}

template <bool SEFULL, bool GAIN, bool DUAL>
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
    const double *se = a.se + (a.se_per_profile ? (size_t)p * m * (SEFULL ? m : 1) : 0);   // SEFULL: Se [m][m]
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

    const int tx = tid & 15, ty = tid >> 4;
    double c2full = 0.;   // SEFULL, thread 0: (y - F)^T Se^-1 (y - F)
    if constexpr (SEFULL) {
        // ---- Se = L_e L_e^T in the LDS that phase 0 has released and phase 2 does not need yet; u_e = L_e^-1 (y - F) as the extra row
        for (int e = tid; e < m * m; e += OE_THREADS) {
            const int j = e / m, jp = e - j * m;
            if (jp <= j) sM[tri(j) + jp] = se[e];
        }
        if (tid < m) sU[tid] = yo[tid] - Y[tid];
        __syncthreads();
        oe_cholesky(sM, sU, m, tid, tx, ty, &sBad);
        if (tid == 0)
            for (int j = 0; j < m; j++) c2full += sU[j] * sU[j];
        // (thread 0 has read sU before it reaches the barrier behind phase 1; phase 2 writes the LDS behind that one)
    }

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
                if constexpr (SEFULL) {
                    if (j < m && jp <= j) sM[tri(j) + jp] = acc[a2 * (a2 + 1) / 2 + b2] + se[(size_t)j * m + jp];
                } else {
                    if (j < m && jp <= j) sM[tri(j) + jp] = j == jp ? acc[a2 * (a2 + 1) / 2 + b2] + se[j] : acc[a2 * (a2 + 1) / 2 + b2];
                }
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
    oe_cholesky(sM, sU, m, tid, tx, ty, &sBad);
    const bool bad = sBad != 0;
    double c2cost = 0.;   // DUAL, thread 0: chi2 again, for the cost
    if (tid == 0) {
        double c2 = 0.;
        if constexpr (SEFULL) {
            if (!bad) c2 = c2full;
        } else {
            if (!bad)
                for (int j = 0; j < m; j++) {
                    const double dy = yo[j] - Y[j];
                    c2 += dy * dy / se[j];
                }
        }
        if (a.chi2) a.chi2[p] = c2;
        a.status[p] = bad ? 1 : 0;
        if constexpr (DUAL) c2cost = c2;
    }

    // ---- 4: the states
    for (int i = tid; i < n; i += OE_THREADS) {
        const size_t o = (size_t)p * n + i;
        if (bad) {
            a.x_new[o] = x[i];
            if (a.post_var) a.post_var[o] = 0.;
            if (a.avk_diag) a.avk_diag[o] = 0.;
            if constexpr (DUAL) {
                if (a.c_new) a.c_new[o] = a.c ? a.c[o] : 0.;
            }
            continue;
        }
        double pv = 0., av = 0., dx = 0., q = 0.;   // (q: DUAL only)
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
                    if constexpr (DUAL) q += ab[r] * sU[kb + r];
                }
            }
        }
        a.x_new[o] = x[i] + (xa[i] - x[i]) * ginv + dx;
        if (a.post_var) a.post_var[o] = Sa[(size_t)i * n + i] * ginv - pv;
        if (a.avk_diag) a.avk_diag[o] = av;
        if constexpr (DUAL) {
            // c_new = Sa^-1 (x_new - xa) = g (gamma c + K^T M^-1 r), K^T M^-1 r = b . u
            if (a.c_new) a.c_new[o] = ginv * ((a.c ? gam * a.c[o] : 0.) + q);
        }
    }

    // ---- 5: the gain, G^T = L^-T a: back substitution from the last row up, OE_KB rows at a time (thread i reads the a[k][i] and the
    // gain_t[t][i] that it stored itself)
    if constexpr (GAIN) {
        double *G = a.gain_t + (size_t)p * mn;
        for (int i = tid; i < n; i += OE_THREADS) {
            if (bad) {
                for (int k = 0; k < m; k++) G[(size_t)k * n + i] = 0.;
                continue;
            }
            for (int kb = (m - 1) / OE_KB * OE_KB; kb >= 0; kb -= OE_KB) {
                double g[OE_KB];
#pragma unroll
                for (int r = 0; r < OE_KB; r++) g[r] = W[(size_t)min(kb + r, m - 1) * n + i];
                for (int t = m - 1; t >= kb + OE_KB; t--) {
                    const double gt = G[(size_t)t * n + i];
                    const double *lt = sM + tri(t) + kb;   // (t >= kb + OE_KB: columns kb .. kb + OE_KB - 1 of row t exist)
#pragma unroll
                    for (int r = 0; r < OE_KB; r++) g[r] -= lt[r] * gt;
                }
#pragma unroll
                for (int r = OE_KB - 1; r >= 0; r--) {
                    if (kb + r < m) {
#pragma unroll
                        for (int q = OE_KB - 1; q > r; q--)
                            if (kb + q < m) g[r] -= sM[tri(kb + q) + kb + r] * g[q];
                        g[r] /= sM[tri(kb + r) + kb + r];
                        G[(size_t)(kb + r) * n + i] = g[r];
                    }
                }
            }
        }
    }

    // ---- the degrees of freedom for signal: avk_diag (not null with dofs: the entry sees to that) summed by one thread, i ascending
    // DUAL: the cost of the iterate the step started from, chi2 + c . (x - xa), behind the same barrier, i ascending
    if (a.dofs || (DUAL && a.cost)) {
        __syncthreads();   // the block's stores to avk_diag are visible to thread 0
        if (tid == 0) {
            if (a.dofs) {
                double sum = 0.;
                for (int i = 0; i < n; i++) sum += a.avk_diag[(size_t)p * n + i];
                a.dofs[p] = sum;
            }
            if constexpr (DUAL) {
                if (a.cost) {
                    double sum = 0.;
                    if (a.c && !bad)
                        for (int i = 0; i < n; i++) sum += a.c[(size_t)p * n + i] * (x[i] - xa[i]);
                    a.cost[p] = bad ? 0. : c2cost + sum;
                }
            }
        }
    }
}

// The matrices of a profile from its a = L^-1 W^T and b = L^-1 K, [m][n] each in the workspace.  Tile (ti, tj) of 64 x 64 outputs:
// thread (ty, tx) owns rows i0 + ty + 16 r and columns j0 + tx + 16 c.  COV tiles above the diagonal have nothing to do: the tile below
// stores their elements as its mirror image.
template <bool AVK, bool COV>
__global__ __launch_bounds__(OE_THREADS) void oe_cov_kernel(OeCovArgs a, int p0) {
    __shared__ double sAi[OE_CK][OE_CT], sAj[COV ? OE_CK : 1][OE_CT], sBj[AVK ? OE_CK : 1][OE_CT];
    const int m = a.nmeas, n = a.nstate, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int nt = (n + OE_CT - 1) / OE_CT, ti = blockIdx.x / nt, tj = blockIdx.x - ti * nt;
    const int p = p0 + blockIdx.y, i0 = ti * OE_CT, j0 = tj * OE_CT;
    const bool cov = COV && ti >= tj;
    if (!AVK && !cov) return;
    const size_t mn = (size_t)m * n, nn = (size_t)n * n;
    const double *Bm = a.ws + (size_t)p * 2 * mn, *Am = Bm + mn;
    double *avk = AVK ? a.avk + (size_t)p * nn : nullptr, *pc = COV ? a.post_cov + (size_t)p * nn : nullptr;
    if (a.status[p] != 0) {   // a failed profile: zeros (its workspace holds no a and b)
#pragma unroll
        for (int r = 0; r < OE_CR; r++)
#pragma unroll
            for (int c = 0; c < OE_CR; c++) {
                const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
                if (i < n && j < n) {
                    if (AVK) avk[(size_t)i * n + j] = 0.;
                    if (cov) pc[(size_t)i * n + j] = pc[(size_t)j * n + i] = 0.;
                }
            }
        return;
    }
    double accA[OE_CR][OE_CR], accP[OE_CR][OE_CR];
#pragma unroll
    for (int r = 0; r < OE_CR; r++)
#pragma unroll
        for (int c = 0; c < OE_CR; c++) accA[r][c] = accP[r][c] = 0.;
    // A thread moves column ii of slab rows kq, kq + 4, ..: the next slab is fetched into registers while this one is consumed
    constexpr int OE_CQ = OE_CK * OE_CT / OE_THREADS;
    const int ii = tid & (OE_CT - 1), kq = tid / OE_CT;
    const bool in_i = i0 + ii < n, in_j = j0 + ii < n;
    double pa[OE_CQ], pj[OE_CQ], pb[OE_CQ];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < OE_CQ; q++) {
            const int k = k0 + kq + q * (OE_THREADS / OE_CT);
            const size_t row = (size_t)min(k, m - 1) * n;
            pa[q] = k < m && in_i ? Am[row + i0 + ii] : 0.;
            if (cov) pj[q] = k < m && in_j ? Am[row + j0 + ii] : 0.;
            if (AVK) pb[q] = k < m && in_j ? Bm[row + j0 + ii] : 0.;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < m; k0 += OE_CK) {
        const int kn = min(OE_CK, m - k0);
        __syncthreads();   // the slab before is consumed
#pragma unroll
        for (int q = 0; q < OE_CQ; q++) {
            const int kk = kq + q * (OE_THREADS / OE_CT);
            sAi[kk][ii] = pa[q];
            if (cov) sAj[kk][ii] = pj[q];
            if (AVK) sBj[kk][ii] = pb[q];
        }
        __syncthreads();
        if (k0 + OE_CK < m) fetch(k0 + OE_CK);
        for (int kk = 0; kk < kn; kk++) {
            double ai[OE_CR], aj[OE_CR], bj[OE_CR];
#pragma unroll
            for (int r = 0; r < OE_CR; r++) {
                ai[r] = sAi[kk][ty + 16 * r];
                if (cov) aj[r] = sAj[kk][tx + 16 * r];
                if (AVK) bj[r] = sBj[kk][tx + 16 * r];
            }
#pragma unroll
            for (int r = 0; r < OE_CR; r++)
#pragma unroll
                for (int c = 0; c < OE_CR; c++) {
                    if (AVK) accA[r][c] = fma(ai[r], bj[c], accA[r][c]);
                    if (cov) accP[r][c] = fma(ai[r], aj[c], accP[r][c]);
                }
        }
    }
    double ginv = 1.;
    const double *Sa = nullptr;
    if (COV) {
        const double gam = a.gamma ? a.gamma[p] : 0.;
        ginv = 1. / (1. + gam);   // (status 0: gamma is finite and >= 0)
        Sa = a.Sa + (a.sa_per_profile ? (size_t)p * nn : 0);
    }
#pragma unroll
    for (int r = 0; r < OE_CR; r++)
#pragma unroll
        for (int c = 0; c < OE_CR; c++) {
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            if (i < n && j < n) {
                if (AVK) avk[(size_t)i * n + j] = accA[r][c];
                if (cov) {
                    // (a diagonal tile holds both (i, j) and (j, i): the same products in the same order, the same Sa element)
                    const double v = fma(Sa[i >= j ? (size_t)i * n + j : (size_t)j * n + i], ginv, -accP[r][c]);
                    pc[(size_t)i * n + j] = v;
                    if (ti > tj) pc[(size_t)j * n + i] = v;
                }
            }
        }
}

// ---- the adaptive loop ---------------------------------------------------------------------------------------
// A state vector into the resident arrays.  Pass 1: ok = every live element of x_src is finite and inside [lo, hi], through one LDS flag
// (every thread that finds a violation stores the same 0).  Pass 2: the live elements of the source - x_fallback where it is given and
// the trial is not ok or the profile is done, x_src otherwise - are written, WKL as exp(x); nothing else is touched.  A column's target
// is its own (the host refuses a map with two written columns on one target): no two threads store to one address.
__global__ __launch_bounds__(OE_THREADS) void oe_scatter_kernel(OeScatterArgs a) {
    __shared__ int sOk;
    const int p = blockIdx.x, tid = threadIdx.x, n = a.nstate;
    const int *kind = a.wmap, *index = a.wmap + n, *mol = a.wmap + 2 * n;
    const int nl = a.nlay[p];
    const double *xs = a.x_src + (size_t)p * n;
    const double *lo = a.lo ? a.lo + (a.box_per_profile ? (size_t)p * n : 0) : nullptr;
    const double *hi = a.hi ? a.hi + (a.box_per_profile ? (size_t)p * n : 0) : nullptr;
    if (tid == 0) sOk = 1;
    __syncthreads();
    auto live = [&](int i) {
        const int k = kind[i];
        return k == 4 || (k == 1 ? index[i] <= nl : index[i] < nl);
    };
    bool out = false;
    for (int i = tid; i < n; i += OE_THREADS) {
        if (!live(i)) continue;
        const double v = xs[i];
        if (!isfinite(v) || (lo && !(v >= lo[i])) || (hi && !(v <= hi[i]))) out = true;
    }
    if (out) sOk = 0;
    __syncthreads();
    const bool ok = sOk != 0;
    if (tid == 0 && a.trial_ok) a.trial_ok[p] = ok ? 1 : 0;
    const bool fall = a.x_fallback && (!ok || (a.done && a.done[p] != 0));
    const double *src = fall ? a.x_fallback + (size_t)p * n : xs;
    for (int i = tid; i < n; i += OE_THREADS) {
        const int k = kind[i];
        if (k < 0 || !live(i)) continue;
        const double v = src[i];
        if (k == 0) a.T[(size_t)p * a.t_stride + index[i]] = v;
        else if (k == 1) a.TZ[(size_t)p * a.tz_stride + index[i]] = v;
        else if (k == 2) a.WKL[(size_t)p * a.wkl_stride + (size_t)index[i] * a.nmol + mol[i]] = exp(v);
        else if (k == 3) a.CLW[(size_t)p * a.clw_stride + index[i]] = v;
        else {
            if (a.tmpsfc_a) a.tmpsfc_a[p] = v;
            if (a.tmpsfc_b) a.tmpsfc_b[p] = v;
        }
    }
}

// The decision on a trial step.  J_trial = chi2(Y_trial) + sum_i c_trial_i (x_trial_i - xa_i): chi2 as the step kernel forms it (thread
// 0 in ascending j; SEFULL: the Cholesky of Se in LDS with y - Y_trial as the extra row), the prior sum by thread 0 in ascending i.
// Thread 0 decides and updates the profile's scalars; the block copies the trial into the iterate where it was accepted.  A profile
// that is done returns before it has read anything else: nothing of it changes.
template <bool SEFULL>
__global__ __launch_bounds__(OE_THREADS) void oe_accept_kernel(OeAcceptArgs a) {
    extern __shared__ __attribute__((aligned(16))) double oe_lds[];
    __shared__ int sBad, sAccept;
    const int p = blockIdx.x, tid = threadIdx.x, m = a.nmeas, n = a.nstate;
    if (a.done[p] != 0) return;   // (the whole workgroup: no barrier is left waiting)
    if (a.step_status[p] == 1) {
        if (tid == 0) a.done[p] = 2;
        return;
    }
    const double *se = a.se + (a.se_per_profile ? (size_t)p * m * (SEFULL ? m : 1) : 0);
    const double *Y = a.Y_trial + (size_t)p * m, *yo = a.y_obs + (size_t)p * m;
    const double *xt = a.x_trial + (size_t)p * n, *ct = a.c_trial + (size_t)p * n, *xa = a.xa + (size_t)p * n;
    if (tid == 0) sBad = 0, sAccept = 0;
    __syncthreads();
    if constexpr (SEFULL) {
        double *sM = oe_lds, *sU = sM + tri(m);
        for (int e = tid; e < m * m; e += OE_THREADS) {
            const int j = e / m, jp = e - j * m;
            if (jp <= j) sM[tri(j) + jp] = se[e];
        }
        if (tid < m) sU[tid] = yo[tid] - Y[tid];
        __syncthreads();
        oe_cholesky(sM, sU, m, tid, tid & 15, tid >> 4, &sBad);
    }
    if (tid == 0) {
        int done = 0;
        if (sBad) {
            done = 2;
        } else {
            double c2 = 0.;
            if constexpr (SEFULL) {
                const double *sU = oe_lds + tri(m);
                for (int j = 0; j < m; j++) c2 += sU[j] * sU[j];
            } else {
                for (int j = 0; j < m; j++) {
                    const double dy = yo[j] - Y[j];
                    c2 += dy * dy / se[j];
                }
            }
            double pr = 0.;
            for (int i = 0; i < n; i++) pr += ct[i] * (xt[i] - xa[i]);
            const double Jt = c2 + pr, Jc = a.J_cur[p];
            double gam = a.gamma[p];
            if (a.trial_ok[p] != 0 && isfinite(Jt) && Jt <= Jc) {
                sAccept = 1;
                a.J_cur[p] = Jt;
                gam *= a.down;
                if (gam < a.gamma_floor) gam = 0.;
                a.n_acc[p]++;
                if (Jc - Jt <= a.conv * m) done = 1;
            } else {
                gam = fmax(gam * a.up, a.gamma_first);
                a.n_rej[p]++;
                if (gam > a.gamma_max) done = 4;
            }
            a.gamma[p] = gam;
            if (a.last && done == 0) done = 3;
        }
        if (done) a.done[p] = done;
    }
    __syncthreads();
    if (sAccept) {
        double *xc = a.x_cur + (size_t)p * n, *cc = a.c_cur + (size_t)p * n;
        for (int i = tid; i < n; i += OE_THREADS) {
            xc[i] = xt[i];
            cc[i] = ct[i];
        }
    }
}

}  // namespace

namespace monortm_dev {
// M - or, before it, the two tiles of phase 2 and the offset table of phase 0, whichever is largest - and r / u
static size_t oe_lds_bytes(int nmeas) {
    const size_t m = (size_t)nmeas;
    return sizeof(double) * (std::max(std::max(m * (m + 1) / 2, 2 * m * OE_ITP), (5 * m + 1) / 2) + m);
}

template <bool SEFULL, bool GAIN, bool DUAL>
static hipError_t launch_oe_step_as(const OeArgs &a, hipStream_t s) {
    const size_t lds = oe_lds_bytes(a.nmeas);
    if (lds > (64u << 10)) {   // m >= 127: beyond the default bound of a launch's dynamic LDS
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(oe_step_kernel<SEFULL, GAIN, DUAL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((oe_step_kernel<SEFULL, GAIN, DUAL>), dim3((unsigned)a.nprof), dim3(OE_THREADS), lds, s, a);
    return hipGetLastError();
}

template <bool DUAL>
static hipError_t launch_oe_step_dual(const OeArgs &a, hipStream_t s) {
    if (a.se_kind) return a.gain_t ? launch_oe_step_as<true, true, DUAL>(a, s) : launch_oe_step_as<true, false, DUAL>(a, s);
    return a.gain_t ? launch_oe_step_as<false, true, DUAL>(a, s) : launch_oe_step_as<false, false, DUAL>(a, s);
}

hipError_t launch_oe_step(const OeArgs &a, hipStream_t s) {
    return a.c || a.c_new || a.cost ? launch_oe_step_dual<true>(a, s) : launch_oe_step_dual<false>(a, s);
}

hipError_t launch_oe_scatter(const OeScatterArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(oe_scatter_kernel, dim3((unsigned)a.nprof), dim3(OE_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_oe_accept(const OeAcceptArgs &a, hipStream_t s) {
    if (!a.se_kind) {
        hipLaunchKernelGGL(oe_accept_kernel<false>, dim3((unsigned)a.nprof), dim3(OE_THREADS), 0, s, a);
        return hipGetLastError();
    }
    const size_t m = (size_t)a.nmeas, lds = sizeof(double) * (m * (m + 1) / 2 + m);   // Se's triangle and y - Y_trial
    if (lds > (64u << 10)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(oe_accept_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(oe_accept_kernel<true>, dim3((unsigned)a.nprof), dim3(OE_THREADS), lds, s, a);
    return hipGetLastError();
}

template <bool AVK, bool COV>
static hipError_t launch_oe_cov_as(const OeCovArgs &a, hipStream_t s) {
    const unsigned nt = (unsigned)((a.nstate + OE_CT - 1) / OE_CT);
    for (int p0 = 0; p0 < a.nprof; p0 += 65535) {   // (the bound of a grid's second dimension)
        hipLaunchKernelGGL((oe_cov_kernel<AVK, COV>), dim3(nt * nt, (unsigned)std::min(65535, a.nprof - p0)), dim3(OE_THREADS), 0, s, a, p0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_oe_cov(const OeCovArgs &a, hipStream_t s) {
    if (a.avk && a.post_cov) return launch_oe_cov_as<true, true>(a, s);
    if (a.avk) return launch_oe_cov_as<true, false>(a, s);
    if (a.post_cov) return launch_oe_cov_as<false, true>(a, s);
    return hipSuccess;
}
}  // namespace monortm_dev
