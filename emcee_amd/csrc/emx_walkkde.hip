// WalkMove and KDEMove proposals on the device (native / Philox mode only): moves/walk.py, moves/kde.py.
//
// One half-step of either move is a short chain of kernels on the context stream; the evaluation of the proposals and the
// Metropolis commit that follow are the three-pass path's (emx.hip: MOVE_EVAL over qout, then k_wide_commit).
//   1. complement statistics (walk with s = 0, KDE): mean and covariance (ddof 1, np.cov) of the complement, two passes of
//      per-workgroup partial sums over fixed slices, added in slice order by one workgroup -- no float atomics, so a chain is
//      bit-reproducible run to run;
//   2. factor (one workgroup, the covariance in LDS): Cholesky L.  KDE: strict (a pivot <= 0 or not finite raises
//      ST_SINGULAR_COV, scipy's LinAlgError), scaled by the bandwidth factor h, and L_h^-1.  Walk: a pivot <= 1e-12 S_jj (that
//      column's variance before the factorisation: scale invariant) zeroes its column (the reference's SVD-based
//      multivariate_normal takes semidefinite matrices);
//   3. proposal, one wave per slot: walk s >= 2  q = x + sum_j w_j (c_hj - x), w_j = (z_j - mean z) / sqrt(s - 1), which is
//      exactly N(x, cov(c_h)) (sum_j w_j = 0; centred on x the rounding error scales with the helpers' spread, not with |x|);
//      walk s = 0  q = x + L z; KDE  q = c_k + L_h z;
//   4. KDE: whitened complement Y_C = (C - mu) L_h^-T, b_j = -|Y_C,j|^2 / 2, queries y_s = L_h^-1 (s - mu), y_q = Y_C[k] + z, and
//      factor = [LSE_j(y_s . Y_C,j + b_j) - |y_s|^2 / 2] - [LSE_j(y_q . Y_C,j + b_j) - |y_q|^2 / 2]  (the normalising constants of
//      the two Gaussian mixtures cancel).  The LSE is a tiled f64 GEMM with an online max / sum epilogue, split over the data
//      rows when the queries alone cannot fill the chip, the partial (max, sum) pairs combined in chunk order.
// The draws are emx_rng.hpp's (wk_*): a pure function of (seed, step, walker); emx_host_walk_kde_draws is their host twin.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "emx_kernels.hpp"
#include "emx_walkkde.hpp"

namespace emx {

namespace {

constexpr int WK_NT = 256;         // threads of every workgroup here
constexpr int WK_SLICE = 256;      // complement rows per partial-sum slice (a pure function of the shape: reproducible anywhere)
constexpr int WK_MAXP = 128;       // at most this many slices (more rows per slice beyond 32 768 complement rows)

__host__ __device__ inline int wk_slices(int64_t Nc) {
    int64_t p = (Nc + WK_SLICE - 1) / WK_SLICE;
    return (int)(p < 1 ? 1 : p > WK_MAXP ? WK_MAXP : p);
}

// complement rank r -> plan position: the split's own positions [pos0, pos0 + ns) are skipped (native_slot's partner map)
__device__ __forceinline__ int comp_walker(const WalkKdeArgs& A, int64_t r) {
    const int64_t pos = r < A.pos0 ? r : r + A.ns;
    return A.order[pos];
}

// work buffer layout (doubles); walk_kde_work_bytes sizes it
struct WkLayout {
    double *pmean, *pcov, *mu, *L, *Linv, *flag, *YC, *bC, *YQ, *pm, *ps;
};
__host__ __device__ inline WkLayout wk_layout(double* w, int64_t N, int D) {
    WkLayout l;
    const int64_t DD = (int64_t)D * D;
    l.pmean = w;
    l.pcov = l.pmean + (int64_t)WK_MAXP * D;
    l.mu = l.pcov + (int64_t)WK_MAXP * DD;
    l.L = l.mu + D;
    l.Linv = l.L + DD;
    l.flag = l.Linv + DD;
    l.YC = l.flag + 8;
    l.bC = l.YC + N * D;
    l.YQ = l.bC + N;
    l.pm = l.YQ + 2 * N * D;
    l.ps = l.pm + (int64_t)WK_LSE_MAXCH * 2 * N;
    return l;
}

// ---- 1. complement statistics ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void slice_of(int64_t Nc, int P, int b, int64_t& r0, int64_t& r1) {
    r0 = Nc * b / P;
    r1 = Nc * (b + 1) / P;
}

// partial column sums of slice b: thread (g, d) sums rows r0 + g, r0 + g + G, ...; the G partials added in g order
__global__ __launch_bounds__(WK_NT) void k_wk_mean_part(const WalkKdeArgs A) {
    __shared__ double red[WK_NT];
    const int D = A.D, G = WK_NT / D, tid = threadIdx.x, g = tid / D, d = tid % D;
    const int64_t Nc = (int64_t)A.N - A.ns;
    const int P = wk_slices(Nc);
    int64_t r0, r1;
    slice_of(Nc, P, blockIdx.x, r0, r1);
    double s = 0.0;
    if (g < G)
        for (int64_t r = r0 + g; r < r1; r += G) s += A.X[(size_t)comp_walker(A, r) * D + d];
    red[tid] = s;
    __syncthreads();
    if (tid < D) {
        double t = 0.0;
        for (int k = 0; k < G; ++k) t += red[k * D + tid];
        wk_layout(A.work, A.N, D).pmean[(size_t)blockIdx.x * D + tid] = t;
    }
}

__global__ __launch_bounds__(WK_NT) void k_wk_mean_fin(const WalkKdeArgs A) {
    const int D = A.D;
    const int64_t Nc = (int64_t)A.N - A.ns;
    const int P = wk_slices(Nc);
    const WkLayout l = wk_layout(A.work, A.N, D);
    for (int d = threadIdx.x; d < D; d += WK_NT) {
        double t = 0.0;
        for (int b = 0; b < P; ++b) t += l.pmean[(size_t)b * D + d];
        l.mu[d] = t / (double)Nc;
    }
}

// partial scatter matrix of slice b: 32 centred rows at a time in LDS, thread e owns entries e, e + 256, ... (lower triangle and
// diagonal are what the factor reads; the whole matrix is formed, it is the simpler loop)
__global__ __launch_bounds__(WK_NT) void k_wk_cov_part(const WalkKdeArgs A) {
    constexpr int RB = 32;
    __shared__ double rows[RB * WK_MAX_D];
    const int D = A.D, tid = threadIdx.x, DD = D * D;
    const int64_t Nc = (int64_t)A.N - A.ns;
    const int P = wk_slices(Nc);
    const WkLayout l = wk_layout(A.work, A.N, D);
    int64_t r0, r1;
    slice_of(Nc, P, blockIdx.x, r0, r1);
    constexpr int EMAX = WK_MAX_D * WK_MAX_D / WK_NT;     // 64 entries a thread at ndim 128
    double acc[EMAX];
#pragma unroll
    for (int m = 0; m < EMAX; ++m) acc[m] = 0.0;
    for (int64_t rb = r0; rb < r1; rb += RB) {
        const int nr = (int)((r1 - rb) < RB ? (r1 - rb) : RB);
        __syncthreads();
        for (int e = tid; e < nr * D; e += WK_NT) {
            const int r = e / D, d = e % D;
            rows[r * D + d] = A.X[(size_t)comp_walker(A, rb + r) * D + d] - l.mu[d];
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < EMAX; ++m) {
            const int e = tid + m * WK_NT;
            if (e < DD) {
                const int i = e / D, j = e % D;
                double a = acc[m];
                for (int r = 0; r < nr; ++r) a = fma(rows[r * D + i], rows[r * D + j], a);
                acc[m] = a;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < EMAX; ++m) {
        const int e = tid + m * WK_NT;
        if (e < DD) l.pcov[(size_t)blockIdx.x * DD + e] = acc[m];
    }
}

// ---- 2. factor ------------------------------------------------------------------------------------------------------------
// One workgroup: the covariance (slice partials added in order, / (Nc - 1)) in LDS, right-looking Cholesky in place.
// KDE: L_h = h L and L_h^-1 (column j of the inverse by forward substitution, thread j).  Walk: semidefinite-tolerant.
__global__ __launch_bounds__(WK_NT) void k_wk_factor(const WalkKdeArgs A) {
    extern __shared__ double S[];       // D x D
    __shared__ double tol[WK_MAX_D];    // walk: 1e-12 S_jj of the covariance before the factorisation
    __shared__ int bad;
    const int D = A.D, tid = threadIdx.x, DD = D * D;
    const int64_t Nc = (int64_t)A.N - A.ns;
    const int P = wk_slices(Nc);
    const WkLayout l = wk_layout(A.work, A.N, D);
    const bool kde = A.kind == MOVE_KDE;
    for (int e = tid; e < DD; e += WK_NT) {
        double t = 0.0;
        for (int b = 0; b < P; ++b) t += l.pcov[(size_t)b * DD + e];
        S[e] = t / (double)(Nc - 1);
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    // a column's own variance sets its threshold, so the rule commutes with scaling a coordinate (a trace-based threshold zeroed
    // the column of a coordinate far smaller than the others); a constant or exactly collinear coordinate still gives a pivot at
    // or below it
    for (int j = tid; j < D; j += WK_NT) tol[j] = 1e-12 * S[j * D + j];
    __syncthreads();
    for (int j = 0; j < D; ++j) {
        const double piv = S[j * D + j];
        bool zero = false;
        if (kde) {
            if (!(piv > 0.0) || !(piv < __builtin_inf())) {
                if (tid == 0) bad = 1;
                zero = true;
            }
        } else {
            zero = !(piv > tol[j]) || !(piv < __builtin_inf());
        }
        const double ljj = zero ? 0.0 : sqrt(piv);
        const double inv = zero ? 0.0 : 1.0 / ljj;
        __syncthreads();
        for (int i = j + 1 + tid; i < D; i += WK_NT) S[i * D + j] *= inv;
        if (tid == 0) S[j * D + j] = ljj;
        __syncthreads();
        // trailing update of the lower triangle: S[i][k] -= L[i][j] L[k][j], j < k <= i
        const int m = D - j - 1;
        for (int e = tid; e < m * m; e += WK_NT) {
            const int i = j + 1 + e / m, k = j + 1 + e % m;
            if (k <= i) S[i * D + k] -= S[i * D + j] * S[k * D + j];
        }
        __syncthreads();
    }
    double h = 1.0;
    if (kde) {
        const double dd = (double)D;
        h = A.bw_rule == 0 ? pow((double)Nc, -1.0 / (dd + 4.0))
            : A.bw_rule == 1 ? pow((double)Nc * (dd + 2.0) / 4.0, -1.0 / (dd + 4.0))
                             : A.bw;
    }
    for (int e = tid; e < DD; e += WK_NT) {
        const int i = e / D, k = e % D;
        l.L[e] = k <= i ? h * S[e] : 0.0;
    }
    if (tid == 0) l.flag[0] = bad ? 1.0 : 0.0;
    if (kde && bad && tid == 0) raise_status(A.status, ST_SINGULAR_COV);
    if (!kde) return;
    __syncthreads();
    for (int e = tid; e < DD; e += WK_NT) {
        const int i = e / D, k = e % D;
        if (k <= i) S[e] *= h;
    }
    __syncthreads();
    // column j of L_h^-1: x_i = (delta_ij - sum_{j <= k < i} L_ik x_k) / L_ii
    for (int j = tid; j < D; j += WK_NT) {
        for (int i = 0; i < j; ++i) l.Linv[(size_t)i * D + j] = 0.0;
        for (int i = j; i < D; ++i) {
            double t = i == j ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) t -= S[i * D + k] * l.Linv[(size_t)k * D + j];
            l.Linv[(size_t)i * D + j] = bad ? 0.0 : t / S[i * D + i];
        }
    }
}

// ---- 4a. KDE whitening: rows 0 .. Nc - 1 the complement (Y_C, b), rows Nc .. N - 1 the split's current positions (y_s) -------
__global__ __launch_bounds__(WK_NT) void k_wk_whiten(const WalkKdeArgs A) {
    __shared__ double cr[4][WK_MAX_D];
    const int D = A.D, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t Nc = (int64_t)A.N - A.ns;
    const WkLayout l = wk_layout(A.work, A.N, D);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < A.N; r += (int64_t)gridDim.x * 4) {
        const int w = r < Nc ? comp_walker(A, r) : A.order[A.pos0 + (r - Nc)];
        for (int d = lane; d < D; d += 64) cr[wv][d] = A.X[(size_t)w * D + d] - l.mu[d];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        double nrm = 0.0;
        double* out = r < Nc ? l.YC + (size_t)r * D : l.YQ + (size_t)(r - Nc) * D;
        for (int i = lane; i < D; i += 64) {
            double y = 0.0;
            for (int k = 0; k <= i; ++k) y = fma(l.Linv[(size_t)i * D + k], cr[wv][k], y);
            out[i] = y;
            nrm = fma(y, y, nrm);
        }
        for (int o = 32; o >= 1; o >>= 1) nrm += __shfl_xor(nrm, o);
        if (r < Nc && lane == 0) l.bC[r] = -0.5 * nrm;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

// ---- 3. proposals: one wave per slot ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(WK_NT) void k_wk_propose(const WalkKdeArgs A) {
    __shared__ double zs[4][WK_MAX_S > WK_MAX_D ? WK_MAX_S : WK_MAX_D];
    __shared__ int hs[4][WK_MAX_S];
    const int D = A.D, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t Nc = (int64_t)A.N - A.ns;
    const WkLayout l = wk_layout(A.work, A.N, D);
    const bool walk_s = A.kind == MOVE_WALK && A.s >= 2;
    const bool singular = A.kind == MOVE_KDE && l.flag[0] != 0.0;
    for (int t = A.t_lo + blockIdx.x * 4 + wv; t < A.t_hi; t += gridDim.x * 4) {
        const int i = A.order[A.pos0 + t];
        double* q = A.qout + (size_t)t * D;
        bool nonfinite = false;
        if (walk_s) {
            const int s = A.s;
            // Floyd: draw k picks r in [0, Nc - s + k]; a rank already taken is replaced by Nc - s + k
            for (int k0 = 0; k0 < s; k0 += 64) {
                const int k = k0 + lane;
                const int cand = k < s ? (int)wk_helper_draw(A.seed, A.step, (uint32_t)i, k, s, (uint64_t)Nc) : 0;
                for (int kk = k0; kk < k0 + 64 && kk < s; ++kk) {
                    const int c = __shfl(cand, kk - k0);
                    bool hit = false;
                    for (int m = lane; m < kk; m += 64) hit = hit || hs[wv][m] == c;
                    const bool taken = __any(hit);
                    __builtin_amdgcn_wave_barrier();
                    if (lane == 0) hs[wv][kk] = taken ? (int)(Nc - s + kk) : c;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            // normals, their mean (fixed-order wave reduction), the weights; then ranks -> walkers
            double zsum = 0.0;
            for (int k = lane; k < s; k += 64) {
                double n0, n1;
                wk_normal_pair(A.seed, A.step, (uint32_t)i, k >> 1, n0, n1);
                const double z = (k & 1) ? n1 : n0;
                zs[wv][k] = z;
                zsum += z;
            }
            for (int o = 32; o >= 1; o >>= 1) zsum += __shfl_xor(zsum, o);
            const double zbar = zsum / (double)s, rs = 1.0 / sqrt((double)(s - 1));
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int k = lane; k < s; k += 64) {
                zs[wv][k] = (zs[wv][k] - zbar) * rs;
                hs[wv][k] = comp_walker(A, hs[wv][k]);
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int d = lane; d < D; d += 64) {
                // sum_k w_k (c_k - x), not sum_k w_k c_k: the weights sum to zero only in exact arithmetic, so the raw form loses
                // eps |x| per step; centred on x the error is eps times the helpers' spread (a constant coordinate stays put)
                const double xd = A.X[(size_t)i * D + d];
                double dq = 0.0;
                int k = 0;
                for (; k + 4 <= s; k += 4) {            // four helper loads in flight, accumulated in draw order
                    const double c0 = A.X[(size_t)hs[wv][k] * D + d], c1 = A.X[(size_t)hs[wv][k + 1] * D + d];
                    const double c2 = A.X[(size_t)hs[wv][k + 2] * D + d], c3 = A.X[(size_t)hs[wv][k + 3] * D + d];
                    dq = fma(zs[wv][k], c0 - xd, dq);
                    dq = fma(zs[wv][k + 1], c1 - xd, dq);
                    dq = fma(zs[wv][k + 2], c2 - xd, dq);
                    dq = fma(zs[wv][k + 3], c3 - xd, dq);
                }
                for (; k < s; ++k) dq = fma(zs[wv][k], A.X[(size_t)hs[wv][k] * D + d] - xd, dq);
                const double acc = xd + dq;
                q[d] = acc;
                nonfinite = nonfinite || !(fabs(acc) < __builtin_inf());
            }
            if (lane == 0) A.fout[t] = 0.0;
        } else {
            for (int p = lane; 2 * p < D; p += 64) {
                double n0, n1;
                wk_normal_pair(A.seed, A.step, (uint32_t)i, p, n0, n1);
                zs[wv][2 * p] = n0;
                if (2 * p + 1 < D) zs[wv][2 * p + 1] = n1;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            int base = i;
            int64_t k = 0;
            if (A.kind == MOVE_KDE) {
                k = (int64_t)wk_centre_rank(A.seed, A.step, (uint32_t)i, (uint64_t)Nc);
                base = comp_walker(A, k);
            }
            for (int d = lane; d < D; d += 64) {
                double lz = 0.0;
                for (int m = 0; m <= d; ++m) lz = fma(l.L[(size_t)d * D + m], zs[wv][m], lz);
                const double v = A.X[(size_t)base * D + d] + lz;
                q[d] = v;
                nonfinite = nonfinite || !(fabs(v) < __builtin_inf());
                if (A.kind == MOVE_KDE) l.YQ[(size_t)(A.ns + t) * D + d] = l.YC[(size_t)k * D + d] + zs[wv][d];
            }
            if (lane == 0 && A.kind == MOVE_WALK) A.fout[t] = 0.0;
            if (lane == 0 && singular) A.fout[t] = -__builtin_inf();
        }
        if (__any(nonfinite) && lane == 0) raise_status(A.status, ST_BAD_COORD);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

// ---- 4b. log-sum-exp of 2 ns queries against Nc data rows ------------------------------------------------------------------
// Workgroup tile: 64 queries x 64 data rows, 16 x 16 threads each holding a 4 x 4 block of scores (queries ty + 16 a, rows
// tx + 16 b), ndim in chunks of 32 through LDS.  The epilogue folds a tile's scores into each thread's online (max, sum) per
// query; the 16 threads of a query are combined in tx order, the chunks later in chunk order (k_wk_lse_fin).
constexpr int LQ = 64, LR = 64, LK = 32;
__global__ __launch_bounds__(WK_NT) void k_wk_lse_part(const WalkKdeArgs A, int nch) {
    __shared__ double qT[LK][LQ + 1];
    __shared__ double yT[LK][LR + 1];
    __shared__ double cm[LQ][17], csum[LQ][17];
    const int D = A.D, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t Nc = (int64_t)A.N - A.ns, nq = 2 * (int64_t)A.ns;
    const WkLayout l = wk_layout(A.work, A.N, D);
    const int64_t q0 = (int64_t)blockIdx.x * LQ;
    const int ch = blockIdx.y;
    const int64_t d0 = Nc * ch / nch, d1 = Nc * (ch + 1) / nch;
    double m[4], sm[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        m[a] = -__builtin_inf();
        sm[a] = 0.0;
    }
    for (int64_t r0 = d0; r0 < d1; r0 += LR) {
        double acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
        for (int k0 = 0; k0 < D; k0 += LK) {
            __syncthreads();
            for (int e = tid; e < LK * LQ; e += WK_NT) {
                const int r = e / LK, kk = e % LK;
                const int64_t qq = q0 + r, rr = r0 + r;
                qT[kk][r] = (qq < nq && k0 + kk < D) ? l.YQ[(size_t)qq * D + k0 + kk] : 0.0;
                yT[kk][r] = (rr < d1 && k0 + kk < D) ? l.YC[(size_t)rr * D + k0 + kk] : 0.0;
            }
            __syncthreads();
            const int kn = D - k0 < LK ? D - k0 : LK;
            for (int kk = 0; kk < kn; ++kk) {
                double qa[4], yb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) qa[a] = qT[kk][ty + 16 * a];
#pragma unroll
                for (int b = 0; b < 4; ++b) yb[b] = yT[kk][tx + 16 * b];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = fma(qa[a], yb[b], acc[a][b]);
            }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double v[4], mt = -__builtin_inf();
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int64_t rr = r0 + tx + 16 * b;
                v[b] = rr < d1 ? acc[a][b] + l.bC[rr] : -__builtin_inf();
                mt = fmax(mt, v[b]);
            }
            const double mn = fmax(m[a], mt);
            if (mn > -__builtin_inf()) {
                double s = sm[a] * exp(m[a] - mn);
#pragma unroll
                for (int b = 0; b < 4; ++b) s += exp(v[b] - mn);
                sm[a] = s;
                m[a] = mn;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        cm[ty + 16 * a][tx] = m[a];
        csum[ty + 16 * a][tx] = sm[a];
    }
    __syncthreads();
    if (tid < LQ && q0 + tid < nq) {
        double mm = -__builtin_inf();
        for (int x = 0; x < 16; ++x) mm = fmax(mm, cm[tid][x]);
        double s = 0.0;
        if (mm > -__builtin_inf())
            for (int x = 0; x < 16; ++x) s += csum[tid][x] * exp(cm[tid][x] - mm);
        l.pm[(size_t)ch * nq + q0 + tid] = mm;
        l.ps[(size_t)ch * nq + q0 + tid] = s;
    }
}

__device__ __forceinline__ double wk_lse(const WkLayout& l, int nch, int64_t nq, int64_t q) {
    double mm = -__builtin_inf();
    for (int c = 0; c < nch; ++c) mm = fmax(mm, l.pm[(size_t)c * nq + q]);
    double s = 0.0;
    for (int c = 0; c < nch; ++c) {
        const double mc = l.pm[(size_t)c * nq + q];
        if (mc > -__builtin_inf()) s += l.ps[(size_t)c * nq + q] * exp(mc - mm);
    }
    return mm + log(s);
}

// factor_t = [LSE(y_s) - |y_s|^2 / 2] - [LSE(y_q) - |y_q|^2 / 2]: one wave per slot (the norms of the two query rows)
__global__ __launch_bounds__(WK_NT) void k_wk_lse_fin(const WalkKdeArgs A, int nch) {
    const int D = A.D, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nq = 2 * (int64_t)A.ns;
    const WkLayout l = wk_layout(A.work, A.N, D);
    if (l.flag[0] != 0.0) return;         // singular covariance: the proposal kernel rejected every slot already
    for (int t = A.t_lo + blockIdx.x * 4 + wv; t < A.t_hi; t += gridDim.x * 4) {
        const double* ys = l.YQ + (size_t)t * D;
        const double* yq = l.YQ + (size_t)(A.ns + t) * D;
        double ns2 = 0.0, nq2 = 0.0;
        for (int d = lane; d < D; d += 64) {
            ns2 = fma(ys[d], ys[d], ns2);
            nq2 = fma(yq[d], yq[d], nq2);
        }
        for (int o = 32; o >= 1; o >>= 1) {
            ns2 += __shfl_xor(ns2, o);
            nq2 += __shfl_xor(nq2, o);
        }
        if (lane == 0) {
            const double ls = wk_lse(l, nch, nq, t) - 0.5 * ns2;
            const double lq = wk_lse(l, nch, nq, A.ns + t) - 0.5 * nq2;
            A.fout[t] = ls - lq;
        }
    }
}

}  // namespace

size_t walk_kde_work_bytes(int64_t N, int D) {
    const int64_t DD = (int64_t)D * D;
    const int64_t n = (int64_t)WK_MAXP * D + (int64_t)WK_MAXP * DD + D + 2 * DD + 8 + N * D + N + 2 * N * D + 2 * (int64_t)WK_LSE_MAXCH * 2 * N;
    return (size_t)n * 8;
}

int walk_kde_lse_chunks(int64_t N, int64_t ns) {
    const int64_t Nc = N - ns, qblocks = (2 * ns + LQ - 1) / LQ;
    int64_t nch = (1024 + qblocks - 1) / qblocks;                   // ~1 024 workgroups: four per CU (a function of the shape only)
    const int64_t rmax = (Nc + LR - 1) / LR;
    if (nch > rmax) nch = rmax;
    if (nch > WK_LSE_MAXCH) nch = WK_LSE_MAXCH;
    return (int)(nch < 1 ? 1 : nch);
}

hipError_t launch_walk_kde(const WalkKdeArgs& A, hipStream_t st) {
    const int64_t Nc = (int64_t)A.N - A.ns;
    const bool stats = A.kind == MOVE_KDE || A.s == 0;
    if (stats) {
        const int P = wk_slices(Nc);
        hipLaunchKernelGGL(k_wk_mean_part, dim3((unsigned)P), dim3(WK_NT), 0, st, A);
        hipLaunchKernelGGL(k_wk_mean_fin, dim3(1), dim3(WK_NT), 0, st, A);
        hipLaunchKernelGGL(k_wk_cov_part, dim3((unsigned)P), dim3(WK_NT), 0, st, A);
        const size_t lds = (size_t)A.D * A.D * 8;
        static bool granted[64] = {};
        int dev = 0;
        if (lds > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && !granted[dev]) {
            const hipError_t e = hipFuncSetAttribute((const void*)k_wk_factor, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)((size_t)WK_MAX_D * WK_MAX_D * 8));
            if (e != hipSuccess) return e;
            granted[dev] = true;
        }
        hipLaunchKernelGGL(k_wk_factor, dim3(1), dim3(WK_NT), lds, st, A);
    }
    if (A.kind == MOVE_KDE) {
        const int64_t nb = (A.N + 3) / 4;
        hipLaunchKernelGGL(k_wk_whiten, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(WK_NT), 0, st, A);
    }
    const int64_t nslots = A.t_hi - A.t_lo;
    const int64_t pb = (nslots + 3) / 4;
    hipLaunchKernelGGL(k_wk_propose, dim3((unsigned)(pb < 8192 ? (pb < 1 ? 1 : pb) : 8192)), dim3(WK_NT), 0, st, A);
    if (A.kind == MOVE_KDE) {
        const int nch = walk_kde_lse_chunks(A.N, A.ns);
        const int64_t qb = (2 * (int64_t)A.ns + LQ - 1) / LQ;
        hipLaunchKernelGGL(k_wk_lse_part, dim3((unsigned)qb, (unsigned)nch), dim3(WK_NT), 0, st, A, nch);
        hipLaunchKernelGGL(k_wk_lse_fin, dim3((unsigned)(pb < 8192 ? (pb < 1 ? 1 : pb) : 8192)), dim3(WK_NT), 0, st, A, nch);
    }
    return hipGetLastError();
}

}  // namespace emx
