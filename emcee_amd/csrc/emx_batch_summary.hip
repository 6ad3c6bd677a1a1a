// libemx, emx_summary_batch: the posterior summaries of every member of an emx_batch, computed next to the member-major chain
// (B, cap, N, D) -- per member the mean, the ddof = 1 covariance, order statistics (from which the caller interpolates
// quantiles) and the stored sample of the largest log-prob, over rows t0, t0 + stride, ... (nt of them) and every walker:
// n = nt N samples.  Only O(members D^2) numbers cross to the host.  The kernels take (chain, cap, N, D, first member), not
// the handle, so that they can run on a single ensemble's chain (one member, cap = its capacity).
//
// A member's rows are cut into S slices of R rows, R and S fixed by nt alone.  Members go in passes of at most
// "batch_summary_members"; every member is reduced on its own.  Per pass
//   k_bsum_mean_part    slab[member][slice][j = w D + d]: sum over the slice's rows, lane = j (coalesced), the 4 waves of a
//                       workgroup sum consecutive quarters of the slice and are added in wave order
//   k_bsum_mean_fin     mean[d] = (sum over walkers in order of (sum over slices in order)) / n.  The two run twice: the second
//                       time on x - mean, which gives the residual sums r[d]; the mean reported is mean[d] + r[d] / n
//   k_bsum_gram_small   D < 16: centred Gram sum (x_j - m_j)(x_k - m_k), j <= k, per slice: 256 samples at a time are centred
//                       into LDS; thread (pair, group g) adds the samples g, g + G, ... of every tile with an explicit fma
//                       (the file is built with -ffp-contract=off: nothing else is fused), groups are added in order
//   k_bsum_gram_mfma    D >= 16: the same per slice on v_mfma_f64_16x16x4_f64, D padded to 16 Dp' with zero columns: a wave
//                       holds up to 8 of the 16 x 16 blocks (jb <= kb) and runs the tile's samples four at a time; a diagonal
//                       block's A and B operands are one LDS value
//   k_bsum_gram_fin_*   cov[j][k] = cov[k][j] = ((sum over slices in order) - r[j] r[k] / n) / (n - 1): the corrected two-pass
//                       form.  The first mean's rounding error is relative to |mean|, not to the spread; the plain form is off
//                       by n / (n - 1) times the product of two such errors, which exceeds the summation error once
//                       |mean| / sd is large (a posterior far from the origin)
//   k_bsum_map          arg-max of the member's selected log-probs, ties to the smallest (row, walker) index -- (value, index)
//                       pairs under that rule form a total order, so the reduction's shape does not matter; then the D coordinates
//   k_bsum_sel_init / k_bsum_hist / k_bsum_scan, 8 passes of 8 bits, most significant first: radix select of every requested
//                       rank of every series (member, d) in place.  A double maps to an order-preserving uint64 key; in a pass
//                       every element whose higher bits equal a rank's prefix counts into that rank's 256 bins (LDS uint32
//                       atomics, then one global 64-bit integer atomic per non-empty bin per workgroup); the scan picks the
//                       digit, lowers the remaining rank and extends the prefix.  Ranks with one prefix share one histogram
//                       (their "leader", the lowest such rank).  After the last pass the prefix is the key of the order
//                       statistic.  The key transform and the bin scan are shared with the host twin emx_host_order_stats.
// Floating-point sums run in an order fixed by (nt, N, D); the selection only counts integers: no bit depends on the member
// range, the pass size or the launch shape.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/emx.h"
#include "emx_internal.hpp"
#include "emx_rng.hpp"

namespace {

constexpr int SEL_MAX_RANKS = 32;
constexpr int SEL_PASSES = 8;
typedef unsigned long long u64;

// ---- shared with the host twin ----------------------------------------------------------------------------------------
// order-preserving key: negatives have every bit flipped, non-negatives the sign bit set (-0.0 sorts just below +0.0)
EMX_HD u64 sel_key(u64 bits) { return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull); }
EMX_HD u64 sel_unkey(u64 key) { return (key >> 63) ? (key ^ 0x8000000000000000ull) : ~key; }
// the digit holding the *rem-th smallest (0-based) of the elements counted in bins[256]; *rem becomes the rank inside that bin
EMX_HD int sel_scan_bins(const u64* bins, int64_t* rem) {
    u64 cum = 0;
    const u64 want = (u64)*rem;
    int digit = 255;
    for (int b = 0; b < 256; ++b) {
        const u64 c = bins[b];
        if (want < cum + c) {
            digit = b;
            break;
        }
        cum += c;
    }
    *rem = (int64_t)(want - cum);
    return digit;
}
// leader[r]: the lowest rank with r's prefix
EMX_HD void sel_leaders(const u64* prefix, int32_t* leader, int nr) {
    for (int r = 0; r < nr; ++r) {
        int l = r;
        for (int q = 0; q < r; ++q)
            if (prefix[q] == prefix[r]) {
                l = q;
                break;
            }
        leader[r] = l;
    }
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
// Selection of one launch: member m = m0 + blockIdx.z (scratch is indexed by blockIdx.z), slice s = blockIdx.y covers the
// selected rows [s R, min(s R + R, nt)); selected row t is stored row t0 + t stride.
struct Sel {
    const double* chain;       // (., cap, N, D)
    const double* chain_lp;    // (., cap, N)
    int64_t cap, N, ND, t0, stride, nt, R, m0;
    int32_t D, S;
};

// sub: nothing, or (mp, D) values (the first mean) subtracted from every sample before it is added: the residual pass
__global__ __launch_bounds__(256) void k_bsum_mean_part(const Sel g, const double* __restrict__ sub, double* __restrict__ mpart) {
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane, s = blockIdx.y, ml = blockIdx.z;
    const int64_t ra = s * g.R, rb = ra + g.R < g.nt ? ra + g.R : g.nt;
    const int64_t q = g.R / 4, ta = ra + wv * q, tb = ta + q < rb ? ta + q : rb;
    double acc = 0.0;
    if (j < g.ND) {
        const double* p = g.chain + ((g.m0 + ml) * g.cap + g.t0) * g.ND + j;
        const int64_t step = g.stride * g.ND;
        const double m = sub ? sub[ml * g.D + j % g.D] : 0.0;       // x - 0.0 is x
#pragma unroll 8
        for (int64_t t = ta; t < tb; ++t) acc += p[t * step] - m;
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && j < g.ND) mpart[(ml * g.S + s) * g.ND + j] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// one thread a (member, d) of the pass.  First pass (mu0 = nothing): out (mp, D) = sum / n, the mean the residuals and the Gram are
// centred on.  Residual pass: resid = sum = the sum of (x - mu0), out = mu0 + resid / n, the mean that is reported
__global__ __launch_bounds__(256) void k_bsum_mean_fin(const Sel g, const double* __restrict__ mpart, const double* __restrict__ mu0,
                                                       double* __restrict__ out, double* __restrict__ resid, int64_t mp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mp * g.D) return;
    const int64_t ml = i / g.D, d = i - ml * g.D;
    double acc = 0.0;
    for (int64_t w = 0; w < g.N; ++w) {
        double col = 0.0;
        for (int64_t s = 0; s < g.S; ++s) col += mpart[(ml * g.S + s) * g.ND + w * g.D + d];
        acc += col;
    }
    const double n = (double)(g.nt * g.N);
    if (!mu0) {
        out[i] = acc / n;
        return;
    }
    resid[i] = acc;
    out[i] = isfinite(mu0[i]) ? mu0[i] + acc / n : mu0[i];      // a column that holds inf keeps the mean NumPy gives it (x - inf is NaN)
}

// pair p of the upper triangle of an L x L matrix in row order -> (j, k), j <= k
__device__ __forceinline__ void tri_pair(int p, int L, int* j, int* k) {
    int row = 0, len = L;
    while (p >= len) {
        p -= len;
        ++row;
        --len;
    }
    *j = row;
    *k = row + p;
}

constexpr int GS_TILE = 256;       // samples a tile of k_bsum_gram_small
// D < 16.  gpart (mp, S, P), P = D (D + 1) / 2
__global__ __launch_bounds__(256) void k_bsum_gram_small(const Sel g, const double* __restrict__ mean, double* __restrict__ gpart) {
    __shared__ double tile[GS_TILE * 15];
    __shared__ double red[256];
    __shared__ double mu[16];
    const int tid = threadIdx.x, D = g.D, P = D * (D + 1) / 2, G = 256 / P;
    const int64_t s = blockIdx.y, ml = blockIdx.z;
    if (tid < D) mu[tid] = mean[ml * D + tid];
    const int p = tid % P, grp = tid / P;
    int j, k;
    tri_pair(p, D, &j, &k);
    const int64_t ra = s * g.R, rb = ra + g.R < g.nt ? ra + g.R : g.nt;
    const int64_t ns = (rb - ra) * g.N;                         // samples of the slice; its elements f = sample D + d = row ND + j
    const double* base = g.chain + ((g.m0 + ml) * g.cap + g.t0 + ra * g.stride) * g.ND;
    const int64_t rowstep = g.stride * g.ND;
    // this thread's next element f = tid + 256 it as (row, col, d), advanced without a division
    int64_t row = tid / g.ND, col = tid - row * g.ND;
    int d = tid % D;
    const int64_t qstep = 256 / g.ND, cstep = 256 - qstep * g.ND;
    const int dstep = 256 % D;
    double acc = 0.0;
    for (int64_t i0 = 0; i0 < ns; i0 += GS_TILE) {
        const int cnt = (int)(ns - i0 < GS_TILE ? ns - i0 : GS_TILE);
        const int nel = cnt * D;
        __syncthreads();                                        // the previous tile is consumed (and mu is written)
        for (int slot = tid; slot < nel; slot += 256) {
            tile[slot] = base[row * rowstep + col] - mu[d];
            row += qstep;
            col += cstep;
            if (col >= g.ND) {
                col -= g.ND;
                ++row;
            }
            d += dstep;
            if (d >= D) d -= D;
        }
        __syncthreads();
        if (grp < G)
            for (int i = grp; i < cnt; i += G) acc = fma(tile[i * D + j], tile[i * D + k], acc);
    }
    red[tid] = acc;
    __syncthreads();
    if (tid < P) {
        double tot = 0.0;
        for (int q = 0; q < G; ++q) tot += red[q * P + tid];
        gpart[(ml * g.S + s) * P + tid] = tot;
    }
}

// cov (mp, D, D) of the pass from gpart (mp, S, P) and the residual sums r (mp, D): the corrected two-pass form
// (G_jk - r_j r_k / n) / (n - 1), G being centred on the first mean, whose rounding error the second term takes out
__global__ __launch_bounds__(256) void k_bsum_gram_fin_small(const Sel g, const double* __restrict__ gpart, const double* __restrict__ resid,
                                                             double* __restrict__ cov, int64_t mp) {
    const int D = g.D, P = D * (D + 1) / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mp * P) return;
    const int64_t ml = i / P;
    const int p = (int)(i - ml * P);
    int j, k;
    tri_pair(p, D, &j, &k);
    double acc = 0.0;
    for (int64_t s = 0; s < g.S; ++s) acc += gpart[(ml * g.S + s) * P + p];
    const double n = (double)(g.nt * g.N);
    const double c = (acc - resid[ml * D + j] * resid[ml * D + k] / n) / (n - 1.0);
    cov[(ml * D + j) * D + k] = c;
    cov[(ml * D + k) * D + j] = c;
}

constexpr int GM_TILE_DOUBLES = 4608;      // T (Dp + 2) <= 4096 + 2 T, T <= 256
constexpr int GM_PAIRS_WAVE = 8, GM_PAIRS_WG = 4 * GM_PAIRS_WAVE;
__host__ __device__ constexpr int gm_tile_samples(int Dp) { return (4096 / Dp) & ~3; }

// D >= 16.  Block pairs (jb <= kb) of the Dp / 16 column blocks; workgroup blockIdx.x holds pairs [32 x, 32 x + 32), pair
// 32 x + 4 a + wave in accumulator a of that wave.  gpart (mp, S, NP, 4, 64): the accumulators as the MFMA leaves them,
// register r of lane l being C[row = (l >> 4) + 4 r][col = l & 15] of the block.
__global__ __launch_bounds__(256) void k_bsum_gram_mfma(const Sel g, const double* __restrict__ mean, double* __restrict__ gpart, int Dp, int NP) {
    typedef double d4 __attribute__((ext_vector_type(4)));
    __shared__ double tile[GM_TILE_DOUBLES];
    __shared__ double mu[256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, D = g.D;
    const int T = gm_tile_samples(Dp), LS = Dp + 2, DPB = Dp / 16;
    const int64_t s = blockIdx.y, ml = blockIdx.z;
    for (int c = tid; c < Dp; c += 256) mu[c] = c < D ? mean[ml * D + c] : 0.0;
    int ja[GM_PAIRS_WAVE], ka[GM_PAIRS_WAVE];
    bool live[GM_PAIRS_WAVE];
    d4 acc[GM_PAIRS_WAVE];
#pragma unroll
    for (int a = 0; a < GM_PAIRS_WAVE; ++a) {
        const int pi = blockIdx.x * GM_PAIRS_WG + 4 * a + wv;
        live[a] = pi < NP;
        int jb = 0, kb = 0;
        if (live[a]) tri_pair(pi, DPB, &jb, &kb);
        ja[a] = jb * 16 + (lane & 15);
        ka[a] = kb * 16 + (lane & 15);
        acc[a] = d4{0.0, 0.0, 0.0, 0.0};
    }
    const int64_t ra = s * g.R, rb = ra + g.R < g.nt ? ra + g.R : g.nt;
    const int64_t ns = (rb - ra) * g.N;
    const double* base = g.chain + ((g.m0 + ml) * g.cap + g.t0 + ra * g.stride) * g.ND;
    const int64_t rowstep = g.stride * g.ND;
    // staging: a wave's lanes cover CPL columns of 64 / CPL samples at a time
    const int CPL = Dp <= 16 ? 16 : Dp <= 32 ? 32 : 64, SPW = 64 / CPL;
    const int ls = lane / CPL, c0 = lane - ls * CPL;
    __syncthreads();
    for (int64_t i0 = 0; i0 < ns; i0 += T) {
        for (int i = wv * SPW + ls; i < T; i += 4 * SPW) {
            const int64_t si = i0 + i;
            const bool in = si < ns;
            const int64_t row = in ? si / g.N : 0, w = si - row * g.N;
            const double* src = base + row * rowstep + w * D;
            for (int c = c0; c < Dp; c += CPL) tile[i * LS + c] = (in && c < D) ? src[c] - mu[c] : 0.0;
        }
        __syncthreads();
        for (int ks = 0; ks < T / 4; ++ks) {
            const double* trow = tile + (ks * 4 + (lane >> 4)) * LS;
#pragma unroll
            for (int a = 0; a < GM_PAIRS_WAVE; ++a)
                if (live[a]) acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(trow[ja[a]], trow[ka[a]], acc[a], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < GM_PAIRS_WAVE; ++a) {
        if (!live[a]) continue;
        const int pi = blockIdx.x * GM_PAIRS_WG + 4 * a + wv;
        double* out = gpart + ((ml * g.S + s) * NP + pi) * 256;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r * 64 + lane] = acc[a][r];
    }
}

__global__ __launch_bounds__(256) void k_bsum_gram_fin_mfma(const Sel g, const double* __restrict__ gpart, const double* __restrict__ resid,
                                                            double* __restrict__ cov, int64_t mp, int Dp, int NP) {
    const int D = g.D;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mp * NP * 256) return;
    const int e = (int)(i & 255), lane = e & 63, r = e >> 6;
    const int64_t mpi = i >> 8, ml = mpi / NP;
    const int pi = (int)(mpi - ml * NP);
    int jb, kb;
    tri_pair(pi, Dp / 16, &jb, &kb);
    const int j = jb * 16 + (lane >> 4) + 4 * r, k = kb * 16 + (lane & 15);
    if (j >= D || k >= D || j > k) return;
    double acc = 0.0;
    for (int64_t s = 0; s < g.S; ++s) acc += gpart[((ml * g.S + s) * NP + pi) * 256 + e];
    const double n = (double)(g.nt * g.N);
    const double c = (acc - resid[ml * D + j] * resid[ml * D + k] / n) / (n - 1.0);
    cov[(ml * D + j) * D + k] = c;
    cov[(ml * D + k) * D + j] = c;
}

// a better than b: larger value, then smaller index; an index < 0 marks "nothing seen"
__device__ __forceinline__ bool map_better(double va, int64_t ia, double vb, int64_t ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    return va > vb || (va == vb && ia < ib);
}

// one workgroup a member: map_lp (mp), map_x (mp, D)
__global__ __launch_bounds__(256) void k_bsum_map(const Sel g, double* __restrict__ map_x, double* __restrict__ map_lp) {
    __shared__ double bv[256];
    __shared__ int64_t bi[256];
    const int tid = threadIdx.x;
    const int64_t ml = blockIdx.x, m = g.m0 + ml, total = g.nt * g.N;
    const double* base = g.chain_lp + (m * g.cap + g.t0) * g.N;
    const int64_t rowstep = g.stride * g.N;
    int64_t row = tid / g.N, w = tid - row * g.N;
    const int64_t qstep = 256 / g.N, wstep = 256 - qstep * g.N;
    double best = 0.0;
    int64_t idx = -1;
    for (int64_t e = tid; e < total; e += 256) {
        const double v = base[row * rowstep + w];
        if (idx < 0 || v > best) {
            best = v;
            idx = e;
        }
        row += qstep;
        w += wstep;
        if (w >= g.N) {
            w -= g.N;
            ++row;
        }
    }
    bv[tid] = best;
    bi[tid] = idx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h && map_better(bv[tid + h], bi[tid + h], bv[tid], bi[tid])) {
            bv[tid] = bv[tid + h];
            bi[tid] = bi[tid + h];
        }
        __syncthreads();
    }
    const int64_t e = bi[0], r = e / g.N, ww = e - r * g.N;
    if (tid == 0) map_lp[ml] = bv[0];
    const double* x = g.chain + ((m * g.cap + g.t0 + r * g.stride) * g.N + ww) * g.D;
    for (int d = tid; d < g.D; d += 256) map_x[ml * g.D + d] = x[d];
}

// selection state of the pass: prefix / rem / leader (mp, D, nr); hist (mp, D, nr, 256)
__global__ __launch_bounds__(256) void k_bsum_sel_init(u64* __restrict__ prefix, int64_t* __restrict__ rem, int32_t* __restrict__ leader,
                                                       const int64_t* __restrict__ ranks, int nr, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    prefix[i] = 0;
    rem[i] = ranks[i % nr];
    leader[i] = 0;               // every rank starts with the empty prefix: rank 0 leads
}

// pass `pass` (digit = bits [shift, shift + 8), shift = 56 - 8 pass).  grid (dim tiles of DT dims, S, mp)
__global__ __launch_bounds__(256) void k_bsum_hist(const Sel g, const u64* __restrict__ prefix, const int32_t* __restrict__ leader,
                                                   u64* __restrict__ hist, int nr, int DT, int pass) {
    __shared__ uint32_t h[SEL_MAX_RANKS * 256];
    __shared__ u64 pf[SEL_MAX_RANKS];
    __shared__ int32_t lead[SEL_MAX_RANKS];
    const int tid = threadIdx.x, D = g.D;
    const int d0 = blockIdx.x * DT, dc = D - d0 < DT ? D - d0 : DT;          // this workgroup's dims [d0, d0 + dc)
    const int64_t s = blockIdx.y, ml = blockIdx.z;
    const int nslot = dc * nr, shift = 56 - 8 * pass;
    for (int i = tid; i < nslot * 256; i += 256) h[i] = 0;
    if (tid < nslot) {
        const int64_t at = (ml * D + d0) * nr + tid;
        pf[tid] = pass ? prefix[at] >> (shift + 8) : 0;
        lead[tid] = leader[at];
    }
    __syncthreads();
    const int64_t ra = s * g.R, rb = ra + g.R < g.nt ? ra + g.R : g.nt;
    const int64_t nel = (rb - ra) * g.ND;
    const double* base = g.chain + ((g.m0 + ml) * g.cap + g.t0 + ra * g.stride) * g.ND;
    const int64_t rowstep = g.stride * g.ND;
    int64_t row = tid / g.ND, col = tid - row * g.ND;
    int d = tid % D;
    const int64_t qstep = 256 / g.ND, cstep = 256 - qstep * g.ND;
    const int dstep = 256 % D;
    for (int64_t f = tid; f < nel; f += 256) {
        const int dl = d - d0;
        if (dl >= 0 && dl < dc) {
            const u64 key = sel_key((u64)__double_as_longlong(base[row * rowstep + col]));
            const u64 hi = pass ? key >> (shift + 8) : 0;
            const uint32_t digit = (uint32_t)(key >> shift) & 255u;
            for (int r = 0; r < nr; ++r) {
                const int sl = dl * nr + r;
                if (lead[sl] == r && pf[sl] == hi) atomicAdd(&h[sl * 256 + digit], 1u);
            }
        }
        row += qstep;
        col += cstep;
        if (col >= g.ND) {
            col -= g.ND;
            ++row;
        }
        d += dstep;
        if (d >= D) d -= D;
    }
    __syncthreads();
    u64* out = hist + ((ml * D + d0) * nr) * 256;
    for (int i = tid; i < nslot * 256; i += 256)
        if (h[i]) atomicAdd(&out[i], (u64)h[i]);
}

// one thread a series (member, d): every rank takes its digit from its leader's bins; after the last pass order (mp, nr, D)
__global__ __launch_bounds__(64) void k_bsum_scan(u64* __restrict__ prefix, int64_t* __restrict__ rem, int32_t* __restrict__ leader,
                                                  const u64* __restrict__ hist, double* __restrict__ order, int nr, int D, int64_t nseries,
                                                  int pass) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= nseries) return;
    const int shift = 56 - 8 * pass;
    u64 pfx[SEL_MAX_RANKS];
    int32_t ld[SEL_MAX_RANKS];
    for (int r = 0; r < nr; ++r) {
        int64_t want = rem[i * nr + r];
        const int digit = sel_scan_bins(hist + (i * nr + leader[i * nr + r]) * 256, &want);
        rem[i * nr + r] = want;
        pfx[r] = prefix[i * nr + r] | ((u64)digit << shift);
        prefix[i * nr + r] = pfx[r];
    }
    sel_leaders(pfx, ld, nr);
    for (int r = 0; r < nr; ++r) leader[i * nr + r] = ld[r];
    if (pass == SEL_PASSES - 1) {
        const int64_t ml = i / D, d = i - ml * D;
        for (int r = 0; r < nr; ++r) order[(ml * nr + r) * D + d] = __longlong_as_double((long long)sel_unkey(pfx[r]));
    }
}

// ---- one ensemble's chain (emx_summary) -----------------------------------------------------------------------------------
#include "emx_summary_single.hpp"

// ---- one ensemble's histograms (emx_chain_minmax, emx_histograms) ---------------------------------------------------------
#include "emx_hist.hpp"

// ---- every member's histograms (emx_chain_minmax_batch, emx_histograms_batch) ---------------------------------------------
#include "emx_batch_hist.hpp"

// ---- host -----------------------------------------------------------------------------------------------------------
int sfail(emx_batch* b, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int sfail(emx_batch* b, int code, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return emx_internal_batch_fail(b, code, buf);
}

struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
};

int grow(emx_batch* b, Buf& u, size_t bytes, const char* what) {
    if (bytes <= u.bytes) return 0;
    if (u.p) hipFree(u.p);
    u.p = nullptr;
    u.bytes = 0;
    const hipError_t e = hipMalloc(&u.p, bytes);
    if (e != hipSuccess) return sfail(b, -2, "emx_summary_batch: %s allocation (%zu bytes): %s", what, bytes, hipGetErrorString(e));
    u.bytes = bytes;
    return 0;
}

int efail(emx_ctx* c, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int efail(emx_ctx* c, int code, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return emx_internal_fail(c, code, buf);
}

int egrow(emx_ctx* c, Buf& u, size_t bytes, const char* what, const char* fn = "emx_summary") {
    if (bytes <= u.bytes) return 0;
    if (u.p) hipFree(u.p);
    u.p = nullptr;
    u.bytes = 0;
    const hipError_t e = hipMalloc(&u.p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return efail(c, -2, "%s: %s allocation (%zu bytes): %s", fn, what, bytes, hipGetErrorString(e));
    }
    u.bytes = bytes;
    return 0;
}

#define ESUM_HIP(what, expr)                                                                                           \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) return efail(c, -2, "emx_summary: %s: %s", what, hipGetErrorString(e_));                 \
    } while (0)

#define SUM_HIP(what, expr)                                                                                            \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) return sfail(b, -2, "emx_summary_batch: %s: %s", what, hipGetErrorString(e_));           \
    } while (0)

}  // namespace

struct BatchSummary {
    Buf mpart, gpart, mean, meanc, resid, cov, order, map_x, map_lp, hist, prefix, rem, leader, ranks;
    // emx_chain_minmax_batch / emx_histograms_batch
    Buf h_plo, h_phi, h_pnf, h_lo, h_hi, h_nf, h_edges, h_pedges, h_eoff, h_poff, h_pairs, h_pairoff, h_counts, h_pcounts, h_codes;
    int64_t h_launches = 0;      // kernel launches of the last emx_histograms_batch call (emx_histograms_batch_info)
};

void emx_internal_batch_summary_release(BatchSummary* s) {
    if (!s) return;
    for (Buf* u : {&s->mpart, &s->gpart, &s->mean, &s->meanc, &s->resid, &s->cov, &s->order, &s->map_x, &s->map_lp, &s->hist, &s->prefix, &s->rem, &s->leader,
                   &s->ranks, &s->h_plo, &s->h_phi, &s->h_pnf, &s->h_lo, &s->h_hi, &s->h_nf, &s->h_edges, &s->h_pedges, &s->h_eoff, &s->h_poff,
                   &s->h_pairs, &s->h_pairoff, &s->h_counts, &s->h_pcounts, &s->h_codes})
        if (u->p) hipFree(u->p);
    delete s;
}

struct EnsSummary {
    Buf part, fold, gpart, gfold, mean, meanc, resid, cov, order, map_x, map_lp, map_pv, map_pi, hist, prefix, rem, slotof, slotpf, nlead, info, ranks, lkey, ldim;
    int64_t sel_reads = 0, listed = -1, list_reads = 0;      // the last call's selection (emx_summary_info)
    // emx_chain_minmax / emx_histograms
    Buf h_plo, h_phi, h_pnf, h_lo, h_hi, h_nf, h_edges, h_pedges, h_eoff, h_poff, h_pairs, h_pairoff, h_counts, h_pcounts, h_codes;
};

void emx_internal_ens_summary_release(EnsSummary* s) {
    if (!s) return;
    for (Buf* u : {&s->part, &s->fold, &s->gpart, &s->gfold, &s->mean, &s->meanc, &s->resid, &s->cov, &s->order, &s->map_x, &s->map_lp, &s->map_pv, &s->map_pi,
                   &s->hist, &s->prefix, &s->rem, &s->slotof, &s->slotpf, &s->nlead, &s->info, &s->ranks, &s->lkey, &s->ldim, &s->h_plo,
                   &s->h_phi, &s->h_pnf, &s->h_lo, &s->h_hi, &s->h_nf, &s->h_edges, &s->h_pedges, &s->h_eoff, &s->h_poff, &s->h_pairs,
                   &s->h_pairoff, &s->h_counts, &s->h_pcounts, &s->h_codes})
        if (u->p) hipFree(u->p);
    delete s;
}

namespace {

// `count` partials of `width` doubles in a -> one, by k_esum_fold levels between a and b; *out: where it is
int es_fold(emx_ctx* c, hipStream_t st, double* a, double* b, int64_t count, int64_t width, const double** out) {
    while (count > 1) {
        const int64_t groups = (count + ES_FOLD - 1) / ES_FOLD;
        hipLaunchKernelGGL(k_esum_fold, dim3((unsigned)((width + 255) / 256), (unsigned)groups), dim3(256), 0, st, (const double*)a, b, count, width);
        ESUM_HIP("fold launch", hipGetLastError());
        std::swap(a, b);
        count = groups;
    }
    *out = a;
    return 0;
}

#define EHIST_HIP(what, expr)                                                                                          \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) return efail(c, -2, "%s: %s: %s", fn, what, hipGetErrorString(e_));                      \
    } while (0)

// the rows start, start + stride, ... < stop of plane 0 / 2 as an ESel; the checks of emx_summary
int eh_selection(emx_ctx* c, const char* fn, const EmxChainView& v, int32_t plane, int64_t start, int64_t stop, int64_t stride, ESel* g) {
    if (plane != 0 && plane != 2) return efail(c, -1, "%s: plane 0 (coordinates) or 2 (blobs); got %d", fn, plane);
    const double* X = v.chain;
    int64_t W = v.D;
    if (plane == 2) {
        if (v.nblobs < 1) return efail(c, -1, "%s: the context's target has no blobs", fn);
        X = v.chain_blobs;
        W = v.nblobs;
    }
    if (!X || !v.chain_lp || v.stored <= 0) return efail(c, -1, "%s: no stored chain (emx_chain_config + stored steps)", fn);
    if (stride < 1 || start < 0 || stop > v.stored) return efail(c, -1, "%s: rows need 0 <= start, stop <= stored, stride >= 1", fn);
    const int64_t nt = start < stop ? (stop - start + stride - 1) / stride : 0;
    if (nt < 1) return efail(c, -1, "%s: the selection is empty", fn);
    g->x = X + start * v.N * W;
    g->lp = v.chain_lp + start * v.N;
    g->N = v.N;
    g->NW = v.N * W;
    g->rowstep = stride * v.N * W;
    g->lprowstep = stride * v.N;
    g->n = nt * v.N;
    g->nt = nt;
    g->W = (int32_t)W;
    return 0;
}

// off[0 ... W] and the edges they cut: 0 first, 1 ... maxbins bins a column, strictly increasing, no NaN
int eh_check_edges(emx_ctx* c, const char* fn, const char* what, const int64_t* off, const double* e, int64_t W, int maxbins) {
    if (!off || !e) return efail(c, -1, "%s: the %s edges and their offsets are needed", fn, what);
    if (off[0] != 0) return efail(c, -1, "%s: the %s edge offsets start at 0", fn, what);
    for (int64_t d = 0; d < W; ++d) {
        const int64_t nb = off[d + 1] - off[d] - 1;
        if (nb < 1 || nb > maxbins) return efail(c, -1, "%s: column %lld has %lld %s bins; 1 ... %d", fn, (long long)d, (long long)nb, what, maxbins);
        for (int64_t i = off[d]; i < off[d + 1]; ++i)
            if (e[i] != e[i] || (i > off[d] && !(e[i] > e[i - 1])))
                return efail(c, -1, "%s: the %s edges of column %lld are not strictly increasing", fn, what, (long long)d);
    }
    return 0;
}

struct EHTileSpan {
    int d0, dc;
    size_t lds;
};

constexpr int EH_MAX_DEVICES = 64;      // function attributes are per device: one process may drive several GPUs

// raises a kernel's dynamic LDS limit to `lds` on device `dev`; granted[]: the largest size set so far per device, shared by
// every context of the process, as the attribute is the function's and not a context's
hipError_t eh_grant_lds(const void* kern, size_t* granted, int dev, size_t lds) {
    const bool known = dev >= 0 && dev < EH_MAX_DEVICES;
    if (known && lds <= granted[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess && known) granted[dev] = lds;
    return e;
}

size_t es_hist_lds(int DT, int ns) { return (size_t)((DT * ns * 257 + 1) & ~1) * 4 + (size_t)DT * ns * 8; }

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int emx_summary(emx_ctx* c, int32_t plane, int64_t start, int64_t stop, int64_t stride, double* mean_out, double* cov_out, int32_t nranks,
                const int64_t* ranks, double* order_out, double* map_coords_out, double* map_log_prob_out, int64_t* nsamples_out) {
    if (const int rc = emx_internal_settle(c)) return rc;
    EmxChainView v;
    if (const int rc = emx_internal_chain_view(c, &v)) return rc;
    if (plane != 0 && plane != 2) return efail(c, -1, "emx_summary: plane 0 (coordinates) or 2 (blobs); got %d", plane);
    const double* X = v.chain;
    int64_t W = v.D;
    if (plane == 2) {
        if (v.nblobs < 1) return efail(c, -1, "emx_summary: the context's target has no blobs");
        X = v.chain_blobs;
        W = v.nblobs;
    }
    if (!X || !v.chain_lp || v.stored <= 0) return efail(c, -1, "emx_summary: no stored chain (emx_chain_config + stored steps)");
    if (stride < 1 || start < 0 || stop > v.stored) return efail(c, -1, "emx_summary: rows need 0 <= start, stop <= stored, stride >= 1");
    const int64_t nt = start < stop ? (stop - start + stride - 1) / stride : 0;
    const int64_t N = v.N, NW = N * W, n = nt * N;
    if (nsamples_out) *nsamples_out = n;
    if (nt < 1) return efail(c, -1, "emx_summary: the selection is empty");
    if (nranks < 0 || nranks > SEL_MAX_RANKS || (nranks > 0 && !ranks)) return efail(c, -1, "emx_summary: 0 ... %d ranks", SEL_MAX_RANKS);
    for (int r = 0; r < nranks; ++r)
        if (ranks[r] < 0 || ranks[r] >= n) return efail(c, -1, "emx_summary: rank %lld outside [0, %lld)", (long long)ranks[r], (long long)n);
    const bool want_cov = cov_out != nullptr, want_mean = mean_out != nullptr || want_cov;
    const bool want_sel = order_out != nullptr && nranks > 0, want_map = map_coords_out != nullptr || map_log_prob_out != nullptr;
    if (want_cov && W > ES_COV_MAX_W) return efail(c, -1, "emx_summary: the covariance is computed for at most %d columns; got %lld", ES_COV_MAX_W, (long long)W);
    const int nr = want_sel ? nranks : 0;

    ESUM_HIP("hipSetDevice", hipSetDevice(v.device));
    if (!*v.summary) *v.summary = new EnsSummary();
    EnsSummary* a = *v.summary;
    const hipStream_t st = v.stream;
    ESel g;
    g.x = X + start * NW;
    g.lp = v.chain_lp + start * N;
    g.N = N;
    g.NW = NW;
    g.rowstep = stride * NW;
    g.lprowstep = stride * N;
    g.n = n;
    g.nt = nt;
    g.W = (int32_t)W;
    Sel fin;                   // what the batch's finishing kernels read: one member, one slice
    std::memset(&fin, 0, sizeof fin);
    fin.N = N;
    fin.nt = nt;
    fin.D = (int32_t)W;
    fin.S = 1;

    if (want_mean) {
        const int64_t C = es_chunk(n, ES_MAX_CHUNKS), G = (n + C - 1) / C;
        const int CW = (int)std::min<int64_t>(W, 256);
        if (int rc = egrow(c, a->part, (size_t)G * W * 8, "mean partials")) return rc;
        if (int rc = egrow(c, a->fold, (size_t)((G + ES_FOLD - 1) / ES_FOLD) * W * 8, "mean partials")) return rc;
        if (int rc = egrow(c, a->mean, (size_t)W * 8, "mean")) return rc;
        if (int rc = egrow(c, a->resid, (size_t)W * 8, "residual sums")) return rc;
        if (int rc = egrow(c, a->meanc, (size_t)W * 8, "mean")) return rc;
        // pass 0: mean = the first mean mu0; pass 1: resid = the sum of (x - mu0) in the same order, meanc = mu0 + resid / n
        for (int pass = 0; pass < 2; ++pass) {
            const double* mu0 = pass ? (const double*)a->mean.p : nullptr;
            hipLaunchKernelGGL(k_esum_mean_part, dim3((unsigned)G, (unsigned)((W + CW - 1) / CW)), dim3(256), 0, st, g, C, CW, mu0, (double*)a->part.p);
            ESUM_HIP("mean launch", hipGetLastError());
            const double* sum = nullptr;
            if (int rc = es_fold(c, st, (double*)a->part.p, (double*)a->fold.p, G, W, &sum)) return rc;
            hipLaunchKernelGGL(k_esum_mean_fin, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, sum, mu0, (double*)(pass ? a->meanc.p : a->mean.p),
                               (double*)a->resid.p, (int)W, n);
            ESUM_HIP("mean launch", hipGetLastError());
        }
        if (mean_out) ESUM_HIP("copy", hipMemcpyAsync(mean_out, a->meanc.p, (size_t)W * 8, hipMemcpyDeviceToHost, st));
    }
    if (want_cov) {
        const bool mfma = W >= 16;
        const int Dp = (int)((W + 15) / 16 * 16), DPB = Dp / 16, NP = DPB * (DPB + 1) / 2, P = (int)(W * (W + 1) / 2);
        const int64_t width = mfma ? (int64_t)NP * 256 : P;
        const int64_t gmax = std::min<int64_t>(ES_MAX_CHUNKS, std::max<int64_t>(64, ((int64_t)256 << 20) / (width * 8)));
        const int64_t C = es_chunk(n, gmax), G = (n + C - 1) / C;
        if (int rc = egrow(c, a->gpart, (size_t)G * width * 8, "Gram partials")) return rc;
        if (int rc = egrow(c, a->gfold, (size_t)((G + ES_FOLD - 1) / ES_FOLD) * width * 8, "Gram partials")) return rc;
        if (int rc = egrow(c, a->cov, (size_t)W * W * 8, "covariance")) return rc;
        if (mfma)
            hipLaunchKernelGGL(k_esum_gram_mfma, dim3((unsigned)((NP + GM_PAIRS_WG - 1) / GM_PAIRS_WG), (unsigned)G), dim3(256), 0, st, g, C,
                               (const double*)a->mean.p, (double*)a->gpart.p, Dp, NP);
        else
            hipLaunchKernelGGL(k_esum_gram_small, dim3((unsigned)G), dim3(256), 0, st, g, C, (const double*)a->mean.p, (double*)a->gpart.p);
        ESUM_HIP("Gram launch", hipGetLastError());
        const double* sum = nullptr;
        if (int rc = es_fold(c, st, (double*)a->gpart.p, (double*)a->gfold.p, G, width, &sum)) return rc;
        if (mfma)
            hipLaunchKernelGGL(k_bsum_gram_fin_mfma, dim3((unsigned)NP), dim3(256), 0, st, fin, sum, (const double*)a->resid.p, (double*)a->cov.p,
                               (int64_t)1, Dp, NP);
        else
            hipLaunchKernelGGL(k_bsum_gram_fin_small, dim3(1), dim3(256), 0, st, fin, sum, (const double*)a->resid.p, (double*)a->cov.p, (int64_t)1);
        ESUM_HIP("Gram launch", hipGetLastError());
        ESUM_HIP("copy", hipMemcpyAsync(cov_out, a->cov.p, (size_t)W * W * 8, hipMemcpyDeviceToHost, st));
    }
    if (want_map) {
        const int np = (int)std::min<int64_t>((n + 4095) / 4096, 2048);
        if (int rc = egrow(c, a->map_pv, (size_t)2048 * 8, "MAP partials")) return rc;
        if (int rc = egrow(c, a->map_pi, (size_t)2048 * 8, "MAP partials")) return rc;
        if (int rc = egrow(c, a->map_x, (size_t)W * 8, "MAP coordinates")) return rc;
        if (int rc = egrow(c, a->map_lp, 8, "MAP log-prob")) return rc;
        hipLaunchKernelGGL(k_esum_map_part, dim3((unsigned)np), dim3(256), 0, st, g, (double*)a->map_pv.p, (int64_t*)a->map_pi.p);
        ESUM_HIP("MAP launch", hipGetLastError());
        hipLaunchKernelGGL(k_esum_map_fin, dim3(1), dim3(256), 0, st, g, (const double*)a->map_pv.p, (const int64_t*)a->map_pi.p, np,
                           (double*)a->map_x.p, (double*)a->map_lp.p);
        ESUM_HIP("MAP launch", hipGetLastError());
        if (map_coords_out) ESUM_HIP("copy", hipMemcpyAsync(map_coords_out, a->map_x.p, (size_t)W * 8, hipMemcpyDeviceToHost, st));
        if (map_log_prob_out) ESUM_HIP("copy", hipMemcpyAsync(map_log_prob_out, a->map_lp.p, 8, hipMemcpyDeviceToHost, st));
    }
    if (want_sel) {
        const int64_t slots = W * nr, nel = n * W;
        if (int rc = egrow(c, a->hist, (size_t)slots * 256 * 8, "histograms")) return rc;
        if (int rc = egrow(c, a->prefix, (size_t)slots * 8, "prefixes")) return rc;
        if (int rc = egrow(c, a->rem, (size_t)slots * 8, "ranks left")) return rc;
        if (int rc = egrow(c, a->slotof, (size_t)slots * 4, "slots")) return rc;
        if (int rc = egrow(c, a->slotpf, (size_t)slots * 8, "slot prefixes")) return rc;
        if (int rc = egrow(c, a->nlead, (size_t)W * 4, "slot counts")) return rc;
        if (int rc = egrow(c, a->info, 16, "counters")) return rc;
        if (int rc = egrow(c, a->order, (size_t)slots * 8, "order statistics")) return rc;
        if (int rc = egrow(c, a->ranks, (size_t)SEL_MAX_RANKS * 8, "ranks")) return rc;
        ESUM_HIP("copy", hipMemcpyAsync(a->ranks.p, ranks, (size_t)nr * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_esum_sel_init, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, (u64*)a->prefix.p, (int64_t*)a->rem.p,
                           (int32_t*)a->slotof.p, (u64*)a->slotpf.p, (int32_t*)a->nlead.p, (const int64_t*)a->ranks.p, nr, slots);
        ESUM_HIP("selection launch", hipGetLastError());
        ESUM_HIP("LDS size", hipFuncSetAttribute((const void*)k_esum_hist<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)es_hist_lds(ES_SLOTS, 1)));
        ESUM_HIP("LDS size", hipFuncSetAttribute((const void*)k_esum_hist<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)es_hist_lds(ES_SLOTS, 1)));
        ESUM_HIP("LDS size", hipFuncSetAttribute((const void*)k_esum_compact, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 ES_COMPACT_TABLE * 8 + ES_STAGE * 12));
        // workgroups of `per` elements (a multiple of ES_STAGE): at most 1024 of them
        auto cut = [](int64_t count, int64_t* per) {
            const int64_t wg = std::max<int64_t>(1, std::min<int64_t>((count + 4 * ES_STAGE - 1) / (4 * ES_STAGE), 1024));
            *per = ((count + wg - 1) / wg + ES_STAGE - 1) / ES_STAGE * ES_STAGE;
            return (count + *per - 1) / *per;
        };
        int ns = 1;
        int64_t listed = -1;             // >= 0: passes read the compacted list of that many elements
        a->sel_reads = a->list_reads = 0;
        a->listed = -1;
        u64 info[2] = {1, (u64)nel};
        for (int pass = 0; pass < SEL_PASSES; ++pass) {
            // compaction before pass 2: auto (1) where at most a quarter of the selection is left, forced (2) wherever the table fits
            if (pass == 2 && v.summary_compact > 0 && W * ns <= ES_COMPACT_TABLE && (v.summary_compact > 1 || info[1] * 4 <= (u64)nel)) {
                const int64_t cap = (int64_t)info[1];
                // no room for the list next to a long chain: the passes read the selection instead
                const bool room = a->lkey.bytes >= (size_t)cap * 8 && a->ldim.bytes >= (size_t)cap * 4;
                Buf nk, nd;
                bool ok = room;
                if (!room) {
                    ok = hipMalloc(&nk.p, (size_t)cap * 8) == hipSuccess && hipMalloc(&nd.p, (size_t)cap * 4) == hipSuccess;
                    if (ok) {
                        if (a->lkey.p) hipFree(a->lkey.p);
                        if (a->ldim.p) hipFree(a->ldim.p);
                        a->lkey.p = nk.p, a->lkey.bytes = (size_t)cap * 8;
                        a->ldim.p = nd.p, a->ldim.bytes = (size_t)cap * 4;
                    } else {
                        (void)hipGetLastError();
                        if (nk.p) hipFree(nk.p);
                        if (nd.p) hipFree(nd.p);
                    }
                }
                if (ok) {
                    int64_t per;
                    const int64_t wg = cut(nel, &per);
                    ESUM_HIP("memset", hipMemsetAsync(a->info.p, 0, 16, st));
                    hipLaunchKernelGGL(k_esum_compact, dim3((unsigned)wg), dim3(ES_HT), (size_t)W * ns * 8 + (size_t)ES_STAGE * 12, st, g, nel, per,
                                       (const u64*)a->slotpf.p, (const int32_t*)a->nlead.p, nr, ns, 16, (u64*)a->lkey.p, (uint32_t*)a->ldim.p,
                                       (u64*)a->info.p, (u64)cap);
                    ESUM_HIP("compaction launch", hipGetLastError());
                    listed = a->listed = cap;
                    ++a->sel_reads;
                }
            }
            const int DT = (int)std::min<int64_t>(W, ES_SLOTS / ns);
            const int64_t count = listed >= 0 ? listed : nel;
            int64_t per;
            const int64_t wg = cut(count, &per);
            const dim3 grid((unsigned)wg, (unsigned)((W + DT - 1) / DT));
            (listed >= 0 ? a->list_reads : a->sel_reads) += grid.y;
            ESUM_HIP("memset", hipMemsetAsync(a->hist.p, 0, (size_t)slots * 256 * 8, st));
            ESUM_HIP("memset", hipMemsetAsync(a->info.p, 0, 16, st));
            if (listed >= 0)
                hipLaunchKernelGGL(k_esum_hist<true>, grid, dim3(ES_HT), es_hist_lds(DT, ns), st, g, (const u64*)a->lkey.p, (const uint32_t*)a->ldim.p,
                                   count, per, (const u64*)a->slotpf.p, (const int32_t*)a->nlead.p, (u64*)a->hist.p, nr, ns, DT, pass);
            else
                hipLaunchKernelGGL(k_esum_hist<false>, grid, dim3(ES_HT), es_hist_lds(DT, ns), st, g, (const u64*)nullptr, (const uint32_t*)nullptr,
                                   count, per, (const u64*)a->slotpf.p, (const int32_t*)a->nlead.p, (u64*)a->hist.p, nr, ns, DT, pass);
            ESUM_HIP("histogram launch", hipGetLastError());
            hipLaunchKernelGGL(k_esum_scan, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, st, (u64*)a->prefix.p, (int64_t*)a->rem.p,
                               (int32_t*)a->slotof.p, (u64*)a->slotpf.p, (int32_t*)a->nlead.p, (const u64*)a->hist.p, (u64*)a->info.p,
                               (double*)a->order.p, nr, (int)W, pass);
            ESUM_HIP("scan launch", hipGetLastError());
            // the next pass's slots a dim (and, after pass 1, the length of the list) come back
            ESUM_HIP("copy", hipMemcpyAsync(info, a->info.p, 16, hipMemcpyDeviceToHost, st));
            ESUM_HIP("synchronize", hipStreamSynchronize(st));
            ns = (int)info[0];
            if (ns < 1 || ns > nr) return efail(c, -2, "emx_summary: the selection's state is inconsistent (%d slots for %d ranks)", ns, nr);
        }
        ESUM_HIP("copy", hipMemcpyAsync(order_out, a->order.p, (size_t)slots * 8, hipMemcpyDeviceToHost, st));
    }
    ESUM_HIP("synchronize", hipStreamSynchronize(st));
    return 0;
}

int emx_summary_batch(emx_batch* b, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop, int64_t stride, double* mean_out,
                      double* cov_out, int32_t nranks, const int64_t* ranks, double* order_out, double* map_coords_out,
                      double* map_log_prob_out, int64_t* nsamples_out) {
    return emx_summary_batch_plane(b, 0, member_lo, member_hi, start, stop, stride, mean_out, cov_out, nranks, ranks, order_out,
                                   map_coords_out, map_log_prob_out, nsamples_out);
}

// plane 4: the blob plane in the chain's place -- the same (rows, N, width) layout with width nblobs, so the kernels run unchanged
int emx_summary_batch_plane(emx_batch* b, int32_t plane, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop, int64_t stride,
                            double* mean_out, double* cov_out, int32_t nranks, const int64_t* ranks, double* order_out,
                            double* map_coords_out, double* map_log_prob_out, int64_t* nsamples_out) {
    EmxBatchView v;
    if (emx_internal_batch_view(b, &v)) return -1;
    if (plane != 0 && plane != 4) return sfail(b, -1, "emx_summary_batch_plane: plane 0 (coordinates) or 4 (blobs); got %d", plane);
    if (plane == 4) {
        if (v.nblobs < 1) return sfail(b, -1, "emx_summary_batch_plane: the handle's target has no blobs");
        v.chain = v.chain_blobs;
        v.D = v.nblobs;
    }
    if (!(0 <= member_lo && member_lo < member_hi && member_hi <= v.B))
        return sfail(b, -1, "emx_summary_batch: members [%d, %d) outside [0, %d) or empty", member_lo, member_hi, v.B);
    if (!v.chain || !v.chain_lp || v.stored <= 0) return sfail(b, -1, "emx_summary_batch: no stored chain (emx_batch_chain_config + a stored run)");
    if (stride < 1 || start < 0 || stop > v.stored) return sfail(b, -1, "emx_summary_batch: rows need 0 <= start, stop <= stored, stride >= 1");
    const int64_t nt = start < stop ? (stop - start + stride - 1) / stride : 0;
    const int64_t N = v.N, D = v.D, ND = N * D, M = member_hi - member_lo, n = nt * N;
    if (nsamples_out) *nsamples_out = n;
    if (nt < 1) return sfail(b, -1, "emx_summary_batch: the selection is empty");
    if (nranks < 0 || nranks > SEL_MAX_RANKS || (nranks > 0 && !ranks))
        return sfail(b, -1, "emx_summary_batch: 0 ... %d ranks", SEL_MAX_RANKS);
    for (int r = 0; r < nranks; ++r)
        if (ranks[r] < 0 || ranks[r] >= n) return sfail(b, -1, "emx_summary_batch: rank %lld outside [0, %lld)", (long long)ranks[r], (long long)n);
    const bool want_cov = cov_out != nullptr, want_mean = mean_out != nullptr || want_cov;
    const bool want_sel = order_out != nullptr && nranks > 0, want_map = map_coords_out != nullptr || map_log_prob_out != nullptr;
    const int nr = want_sel ? nranks : 0;

    // slices: R rows each, from nt alone (grid.y <= 65 535)
    int64_t R = 256;
    while ((nt + R - 1) / R > 65535) R *= 2;
    const int64_t S = (nt + R - 1) / R;
    const bool mfma = D >= 16;
    const int Dp = (int)((D + 15) / 16 * 16), DPB = Dp / 16, NP = DPB * (DPB + 1) / 2, P = (int)(D * (D + 1) / 2);
    const size_t gram_member = want_cov ? (size_t)S * (mfma ? (size_t)NP * 256 : (size_t)P) * 8 : 0;
    const size_t sel_member = (size_t)D * nr * (256 * 8 + 8 + 8 + 4);
    const size_t per_member = (want_mean ? (size_t)S * ND * 8 : 0) + gram_member + sel_member + (size_t)(D * D + nr * D + 2 * D + 1) * 8;
    int64_t mp = std::max<int64_t>(1, (int64_t)(((size_t)512 << 20) / per_member));
    mp = std::min<int64_t>(mp, std::min<int64_t>(M, 65535));
    if (v.summary_members > 0) mp = std::min<int64_t>(mp, v.summary_members);

    SUM_HIP("hipSetDevice", hipSetDevice(v.device));
    if (!*v.summary) *v.summary = new BatchSummary();
    BatchSummary* a = *v.summary;
    if (want_mean) {
        if (int rc = grow(b, a->mpart, (size_t)mp * S * ND * 8, "mean slab")) return rc;
        if (int rc = grow(b, a->mean, (size_t)mp * D * 8, "mean")) return rc;
        if (int rc = grow(b, a->meanc, (size_t)mp * D * 8, "mean")) return rc;
        if (int rc = grow(b, a->resid, (size_t)mp * D * 8, "residual sums")) return rc;
    }
    if (want_cov) {
        if (int rc = grow(b, a->gpart, (size_t)mp * gram_member, "Gram slab")) return rc;
        if (int rc = grow(b, a->cov, (size_t)mp * D * D * 8, "covariance")) return rc;
    }
    if (want_map) {
        if (int rc = grow(b, a->map_x, (size_t)mp * D * 8, "MAP coordinates")) return rc;
        if (int rc = grow(b, a->map_lp, (size_t)mp * 8, "MAP log-prob")) return rc;
    }
    if (want_sel) {
        const size_t slots = (size_t)mp * D * nr;
        if (int rc = grow(b, a->hist, slots * 256 * 8, "histograms")) return rc;
        if (int rc = grow(b, a->prefix, slots * 8, "prefixes")) return rc;
        if (int rc = grow(b, a->rem, slots * 8, "ranks left")) return rc;
        if (int rc = grow(b, a->leader, slots * 4, "leaders")) return rc;
        if (int rc = grow(b, a->order, slots * 8, "order statistics")) return rc;
        if (int rc = grow(b, a->ranks, (size_t)SEL_MAX_RANKS * 8, "ranks")) return rc;
        SUM_HIP("copy", hipMemcpyAsync(a->ranks.p, ranks, (size_t)nr * 8, hipMemcpyHostToDevice, v.stream));
    }
    const int DT = nr ? (int)std::min<int64_t>(D, std::max(1, SEL_MAX_RANKS / nr)) : 1;      // dims a histogram workgroup: DT nr <= 32 slots

    Sel g;
    g.chain = v.chain;
    g.chain_lp = v.chain_lp;
    g.cap = v.cap;
    g.N = N;
    g.ND = ND;
    g.t0 = start;
    g.stride = stride;
    g.nt = nt;
    g.R = R;
    g.D = (int32_t)D;
    g.S = (int32_t)S;
    auto blocks = [](int64_t count, int64_t per) { return dim3((unsigned)((count + per - 1) / per)); };
    for (int64_t m0 = member_lo; m0 < member_hi; m0 += mp) {
        const int64_t mc = std::min<int64_t>(mp, member_hi - m0), mo = m0 - member_lo;
        g.m0 = m0;
        const dim3 slices_j((unsigned)((ND + 63) / 64), (unsigned)S, (unsigned)mc);
        if (want_mean) {
            // pass 0: mean = the first mean mu0; pass 1: resid = the sum of (x - mu0) in the same order, meanc = mu0 + resid / n
            for (int pass = 0; pass < 2; ++pass) {
                const double* mu0 = pass ? (const double*)a->mean.p : nullptr;
                hipLaunchKernelGGL(k_bsum_mean_part, slices_j, dim3(256), 0, v.stream, g, mu0, (double*)a->mpart.p);
                SUM_HIP("mean launch", hipGetLastError());
                hipLaunchKernelGGL(k_bsum_mean_fin, blocks(mc * D, 256), dim3(256), 0, v.stream, g, (const double*)a->mpart.p, mu0,
                                   (double*)(pass ? a->meanc.p : a->mean.p), (double*)a->resid.p, mc);
                SUM_HIP("mean launch", hipGetLastError());
            }
            if (mean_out) SUM_HIP("copy", hipMemcpyAsync(mean_out + mo * D, a->meanc.p, (size_t)mc * D * 8, hipMemcpyDeviceToHost, v.stream));
        }
        if (want_cov) {
            if (mfma) {
                hipLaunchKernelGGL(k_bsum_gram_mfma, dim3((unsigned)((NP + GM_PAIRS_WG - 1) / GM_PAIRS_WG), (unsigned)S, (unsigned)mc), dim3(256), 0,
                                   v.stream, g, (const double*)a->mean.p, (double*)a->gpart.p, Dp, NP);
                SUM_HIP("Gram launch", hipGetLastError());
                hipLaunchKernelGGL(k_bsum_gram_fin_mfma, blocks(mc * NP * 256, 256), dim3(256), 0, v.stream, g, (const double*)a->gpart.p,
                                   (const double*)a->resid.p, (double*)a->cov.p, mc, Dp, NP);
            } else {
                hipLaunchKernelGGL(k_bsum_gram_small, dim3(1, (unsigned)S, (unsigned)mc), dim3(256), 0, v.stream, g, (const double*)a->mean.p,
                                   (double*)a->gpart.p);
                SUM_HIP("Gram launch", hipGetLastError());
                hipLaunchKernelGGL(k_bsum_gram_fin_small, blocks(mc * P, 256), dim3(256), 0, v.stream, g, (const double*)a->gpart.p,
                                   (const double*)a->resid.p, (double*)a->cov.p, mc);
            }
            SUM_HIP("Gram launch", hipGetLastError());
            SUM_HIP("copy", hipMemcpyAsync(cov_out + mo * D * D, a->cov.p, (size_t)mc * D * D * 8, hipMemcpyDeviceToHost, v.stream));
        }
        if (want_map) {
            hipLaunchKernelGGL(k_bsum_map, dim3((unsigned)mc), dim3(256), 0, v.stream, g, (double*)a->map_x.p, (double*)a->map_lp.p);
            SUM_HIP("MAP launch", hipGetLastError());
            if (map_coords_out)
                SUM_HIP("copy", hipMemcpyAsync(map_coords_out + mo * D, a->map_x.p, (size_t)mc * D * 8, hipMemcpyDeviceToHost, v.stream));
            if (map_log_prob_out)
                SUM_HIP("copy", hipMemcpyAsync(map_log_prob_out + mo, a->map_lp.p, (size_t)mc * 8, hipMemcpyDeviceToHost, v.stream));
        }
        if (want_sel) {
            const int64_t slots = mc * D * nr;
            hipLaunchKernelGGL(k_bsum_sel_init, blocks(slots, 256), dim3(256), 0, v.stream, (u64*)a->prefix.p, (int64_t*)a->rem.p,
                               (int32_t*)a->leader.p, (const int64_t*)a->ranks.p, nr, slots);
            SUM_HIP("selection launch", hipGetLastError());
            for (int pass = 0; pass < SEL_PASSES; ++pass) {
                SUM_HIP("memset", hipMemsetAsync(a->hist.p, 0, (size_t)slots * 256 * 8, v.stream));
                hipLaunchKernelGGL(k_bsum_hist, dim3((unsigned)((D + DT - 1) / DT), (unsigned)S, (unsigned)mc), dim3(256), 0, v.stream, g,
                                   (const u64*)a->prefix.p, (const int32_t*)a->leader.p, (u64*)a->hist.p, nr, DT, pass);
                SUM_HIP("histogram launch", hipGetLastError());
                hipLaunchKernelGGL(k_bsum_scan, blocks(mc * D, 64), dim3(64), 0, v.stream, (u64*)a->prefix.p, (int64_t*)a->rem.p, (int32_t*)a->leader.p,
                                   (const u64*)a->hist.p, (double*)a->order.p, nr, (int)D, mc * D, pass);
                SUM_HIP("scan launch", hipGetLastError());
            }
            SUM_HIP("copy", hipMemcpyAsync(order_out + mo * nr * D, a->order.p, (size_t)slots * 8, hipMemcpyDeviceToHost, v.stream));
        }
        // the pass's outputs leave before the next pass reuses the buffers
        SUM_HIP("synchronize", hipStreamSynchronize(v.stream));
    }
    return 0;
}

int emx_summary_info(emx_ctx* c, int64_t* selection_reads_out, int64_t* listed_out, int64_t* list_reads_out) {
    EmxChainView v;
    if (const int rc = emx_internal_chain_view(c, &v)) return rc;
    const EnsSummary* a = *v.summary;
    if (selection_reads_out) *selection_reads_out = a ? a->sel_reads : 0;
    if (listed_out) *listed_out = a ? a->listed : -1;
    if (list_reads_out) *list_reads_out = a ? a->list_reads : 0;
    return 0;
}

int emx_chain_minmax(emx_ctx* c, int32_t plane, int64_t start, int64_t stop, int64_t stride, double* lo_out, double* hi_out, int64_t* nonfinite_out) {
    const char* fn = "emx_chain_minmax";
    if (const int rc = emx_internal_settle(c)) return rc;
    EmxChainView v;
    if (const int rc = emx_internal_chain_view(c, &v)) return rc;
    ESel g;
    if (const int rc = eh_selection(c, fn, v, plane, start, stop, stride, &g)) return rc;
    if (!lo_out || !hi_out || !nonfinite_out) return efail(c, -1, "%s: the three outputs are needed", fn);
    const int64_t W = g.W;
    EHIST_HIP("hipSetDevice", hipSetDevice(v.device));
    if (!*v.summary) *v.summary = new EnsSummary();
    EnsSummary* a = *v.summary;
    const hipStream_t st = v.stream;
    const int64_t C = es_chunk(g.n, ES_MAX_CHUNKS), G = (g.n + C - 1) / C;
    const int CW = (int)std::min<int64_t>(W, 256);
    for (Buf* u : {&a->h_plo, &a->h_phi, &a->h_pnf})
        if (int rc = egrow(c, *u, (size_t)G * W * 8, "min / max partials", fn)) return rc;
    for (Buf* u : {&a->h_lo, &a->h_hi, &a->h_nf})
        if (int rc = egrow(c, *u, (size_t)W * 8, "min / max", fn)) return rc;
    hipLaunchKernelGGL(k_hist_minmax, dim3((unsigned)G, (unsigned)((W + CW - 1) / CW)), dim3(256), 0, st, g, C, CW, (double*)a->h_plo.p,
                       (double*)a->h_phi.p, (u64*)a->h_pnf.p);
    EHIST_HIP("min / max launch", hipGetLastError());
    hipLaunchKernelGGL(k_hist_minmax_fin, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, (const double*)a->h_plo.p, (const double*)a->h_phi.p,
                       (const u64*)a->h_pnf.p, G, (int)W, (double*)a->h_lo.p, (double*)a->h_hi.p, (u64*)a->h_nf.p);
    EHIST_HIP("min / max launch", hipGetLastError());
    EHIST_HIP("copy", hipMemcpyAsync(lo_out, a->h_lo.p, (size_t)W * 8, hipMemcpyDeviceToHost, st));
    EHIST_HIP("copy", hipMemcpyAsync(hi_out, a->h_hi.p, (size_t)W * 8, hipMemcpyDeviceToHost, st));
    EHIST_HIP("copy", hipMemcpyAsync(nonfinite_out, a->h_nf.p, (size_t)W * 8, hipMemcpyDeviceToHost, st));
    EHIST_HIP("synchronize", hipStreamSynchronize(st));
    return 0;
}

int emx_histograms(emx_ctx* c, int32_t plane, int64_t start, int64_t stop, int64_t stride, const int64_t* edge_off, const double* edges,
                   int64_t* counts_out, const int64_t* pedge_off, const double* pedges, int64_t npairs, const int32_t* pairs,
                   const int64_t* pair_off, int64_t* pair_counts_out, int64_t* nsamples_out) {
    const char* fn = "emx_histograms";
    if (const int rc = emx_internal_settle(c)) return rc;
    EmxChainView v;
    if (const int rc = emx_internal_chain_view(c, &v)) return rc;
    ESel g;
    if (const int rc = eh_selection(c, fn, v, plane, start, stop, stride, &g)) return rc;
    const int64_t W = g.W, N = g.N, nt = g.nt, P = npairs;
    if (nsamples_out) *nsamples_out = g.n;
    if (!counts_out) return efail(c, -1, "%s: counts_out is needed", fn);
    if (const int rc = eh_check_edges(c, fn, "marginal", edge_off, edges, W, EH_MAX_BINS)) return rc;
    if (P < 0 || P > 0x7fffffff) return efail(c, -1, "%s: %lld pairs", fn, (long long)P);
    if (P > 0) {
        if (!pairs || !pair_off || !pair_counts_out) return efail(c, -1, "%s: pairs, pair_off and pair_counts_out are needed with npairs > 0", fn);
        if (const int rc = eh_check_edges(c, fn, "pair", pedge_off, pedges, W, EH_MAX_PAIR_BINS)) return rc;
        if (pair_off[0] != 0) return efail(c, -1, "%s: the pair offsets start at 0", fn);
        for (int64_t p = 0; p < P; ++p) {
            const int64_t i = pairs[2 * p], j = pairs[2 * p + 1];
            if (i < 0 || i >= W || j < 0 || j >= W || i == j)
                return efail(c, -1, "%s: pair %lld is (%lld, %lld); two different columns of [0, %lld)", fn, (long long)p, (long long)i, (long long)j, (long long)W);
            const int64_t want = (pedge_off[i + 1] - pedge_off[i] - 1) * (pedge_off[j + 1] - pedge_off[j] - 1);
            if (pair_off[p + 1] - pair_off[p] != want)
                return efail(c, -1, "%s: pair %lld has room for %lld counters, its panel has %lld", fn, (long long)p, (long long)(pair_off[p + 1] - pair_off[p]), (long long)want);
        }
    }
    const int64_t nme = edge_off[W], npe = P ? pedge_off[W] : 0, ncnt = nme - W, npc = P ? pair_off[P] : 0;
    const bool same = P > 0 && !std::memcmp(edge_off, pedge_off, (size_t)(W + 1) * 8) && !std::memcmp(edges, pedges, (size_t)nme * 8);
    // column tiles: as many consecutive columns as EH_LDS_TABLES hold
    std::vector<EHTileSpan> tiles;
    size_t lds_max = 0;
    for (int64_t d0 = 0; d0 < W;) {
        int64_t d1 = d0;
        size_t bytes = 0;
        while (d1 < W && d1 - d0 < EH_MAX_TILE_COLS) {
            const int64_t nb = edge_off[d1 + 1] - edge_off[d1] - 1, pb = (P && !same) ? pedge_off[d1 + 1] - pedge_off[d1] - 1 : -1;
            const size_t add = (size_t)(nb + 1) * 8 + (size_t)(pb + 1) * 8 + (size_t)nb * 4;
            if (d1 > d0 && bytes + add > EH_LDS_TABLES) break;
            bytes += add;
            ++d1;
        }
        EHTileSpan t;
        t.d0 = (int)d0;
        t.dc = (int)(d1 - d0);
        t.lds = eh_code_lds(edge_off[d1] - edge_off[d0], (P && !same) ? pedge_off[d1] - pedge_off[d0] : 0, t.dc, P > 0);
        lds_max = std::max(lds_max, t.lds);
        tiles.push_back(t);
        d0 = d1;
    }
    // chunks of R selected rows: the code plane (W, Mp) of a chunk stays near 256 MB
    int64_t R = v.hist_chunk_rows > 0 ? v.hist_chunk_rows : (P ? std::max<int64_t>(1, ((int64_t)256 << 20) / (N * W)) : nt);
    R = std::min<int64_t>(R, nt);
    while (R * N > ((int64_t)1 << 40)) R = (R + 1) / 2;
    const int64_t Mp = (R * N + 15) / 16 * 16;

    EHIST_HIP("hipSetDevice", hipSetDevice(v.device));
    if (!*v.summary) *v.summary = new EnsSummary();
    EnsSummary* a = *v.summary;
    const hipStream_t st = v.stream;
    if (int rc = egrow(c, a->h_edges, (size_t)nme * 8, "edges", fn)) return rc;
    if (int rc = egrow(c, a->h_eoff, (size_t)(W + 1) * 8, "edge offsets", fn)) return rc;
    if (int rc = egrow(c, a->h_counts, (size_t)ncnt * 8, "counters", fn)) return rc;
    EHIST_HIP("copy", hipMemcpyAsync(a->h_edges.p, edges, (size_t)nme * 8, hipMemcpyHostToDevice, st));
    EHIST_HIP("copy", hipMemcpyAsync(a->h_eoff.p, edge_off, (size_t)(W + 1) * 8, hipMemcpyHostToDevice, st));
    EHIST_HIP("memset", hipMemsetAsync(a->h_counts.p, 0, (size_t)ncnt * 8, st));
    size_t pair_lds = 0;
    if (P) {
        if (int rc = egrow(c, a->h_pedges, (size_t)npe * 8, "pair edges", fn)) return rc;
        if (int rc = egrow(c, a->h_poff, (size_t)(W + 1) * 8, "pair edge offsets", fn)) return rc;
        if (int rc = egrow(c, a->h_pairs, (size_t)P * 8, "pairs", fn)) return rc;
        if (int rc = egrow(c, a->h_pairoff, (size_t)(P + 1) * 8, "pair offsets", fn)) return rc;
        if (int rc = egrow(c, a->h_pcounts, (size_t)npc * 8, "pair counters", fn)) return rc;
        if (int rc = egrow(c, a->h_codes, (size_t)W * Mp, "bin codes", fn)) return rc;
        EHIST_HIP("copy", hipMemcpyAsync(a->h_pedges.p, pedges, (size_t)npe * 8, hipMemcpyHostToDevice, st));
        EHIST_HIP("copy", hipMemcpyAsync(a->h_poff.p, pedge_off, (size_t)(W + 1) * 8, hipMemcpyHostToDevice, st));
        EHIST_HIP("copy", hipMemcpyAsync(a->h_pairs.p, pairs, (size_t)P * 8, hipMemcpyHostToDevice, st));
        EHIST_HIP("copy", hipMemcpyAsync(a->h_pairoff.p, pair_off, (size_t)(P + 1) * 8, hipMemcpyHostToDevice, st));
        EHIST_HIP("memset", hipMemsetAsync(a->h_pcounts.p, 0, (size_t)npc * 8, st));
        for (int64_t p = 0; p < P; ++p) pair_lds = std::max(pair_lds, (size_t)(pair_off[p + 1] - pair_off[p]) * 4);
        static size_t pair_granted[EH_MAX_DEVICES] = {};
        EHIST_HIP("LDS size", eh_grant_lds((const void*)k_hist_pair, pair_granted, v.device, pair_lds));
    }
    static size_t code_granted[EH_MAX_DEVICES] = {};
    EHIST_HIP("LDS size", eh_grant_lds((const void*)k_hist_code, code_granted, v.device, lds_max));

    for (int64_t r0 = 0; r0 < nt; r0 += R) {
        const int64_t M = std::min<int64_t>(R, nt - r0) * N;
        for (const EHTileSpan& t : tiles) {
            const int64_t TS = (int64_t)EH_K * (EH_T / t.dc);
            const int64_t wg = std::max<int64_t>(1, std::min<int64_t>((M + 4 * TS - 1) / (4 * TS), 1024));
            EHCode k;
            k.x = g.x + r0 * g.rowstep;
            k.N = N;
            k.rowstep = g.rowstep;
            k.M = M;
            k.per = ((M + wg - 1) / wg + TS - 1) / TS * TS;
            k.W = (int32_t)W;
            k.d0 = t.d0;
            k.dc = t.dc;
            k.same = same ? 1 : 0;
            k.edge_off = (const int64_t*)a->h_eoff.p;
            k.pedge_off = (const int64_t*)a->h_poff.p;
            k.edges = (const double*)a->h_edges.p;
            k.pedges = (const double*)a->h_pedges.p;
            k.counts = (u64*)a->h_counts.p;
            k.codes = P ? (uint8_t*)a->h_codes.p : nullptr;
            k.Mp = Mp;
            hipLaunchKernelGGL(k_hist_code, dim3((unsigned)((M + k.per - 1) / k.per)), dim3(EH_T), t.lds, st, k);
            EHIST_HIP("binning launch", hipGetLastError());
        }
        if (P) {
            // slices: enough workgroups for the device where the pairs are few; a slice stays below 2^31 samples and grid.y below 65 536
            int64_t slices = std::max<int64_t>(1, std::min<int64_t>((2048 + P - 1) / P, (M + 16383) / 16384));
            slices = std::max<int64_t>(slices, (M + ((int64_t)1 << 31) - 1) >> 31);
            EHPair k;
            k.codes = (const uint8_t*)a->h_codes.p;
            k.Mp = Mp;
            k.M = M;
            k.per = ((M + slices - 1) / slices + 15) / 16 * 16;
            k.pairs = (const int32_t*)a->h_pairs.p;
            k.pair_off = (const int64_t*)a->h_pairoff.p;
            k.pedge_off = (const int64_t*)a->h_poff.p;
            k.out = (u64*)a->h_pcounts.p;
            hipLaunchKernelGGL(k_hist_pair, dim3((unsigned)P, (unsigned)((M + k.per - 1) / k.per)), dim3(256), pair_lds, st, k);
            EHIST_HIP("pair launch", hipGetLastError());
        }
    }
    EHIST_HIP("copy", hipMemcpyAsync(counts_out, a->h_counts.p, (size_t)ncnt * 8, hipMemcpyDeviceToHost, st));
    if (P) EHIST_HIP("copy", hipMemcpyAsync(pair_counts_out, a->h_pcounts.p, (size_t)npc * 8, hipMemcpyDeviceToHost, st));
    EHIST_HIP("synchronize", hipStreamSynchronize(st));
    return 0;
}

int emx_host_order_stats(const double* x, int64_t n, int64_t stride, int32_t nranks, const int64_t* ranks, double* out) {
    if (!x || n < 1 || stride < 1 || nranks < 0 || nranks > SEL_MAX_RANKS || (nranks > 0 && (!ranks || !out))) return -1;
    for (int r = 0; r < nranks; ++r)
        if (ranks[r] < 0 || ranks[r] >= n) return -1;
    const int nr = nranks;
    u64 prefix[SEL_MAX_RANKS];
    int64_t rem[SEL_MAX_RANKS];
    int32_t leader[SEL_MAX_RANKS];
    for (int r = 0; r < nr; ++r) {
        prefix[r] = 0;
        rem[r] = ranks[r];
        leader[r] = 0;
    }
    std::vector<u64> hist((size_t)SEL_MAX_RANKS * 256);
    for (int pass = 0; pass < SEL_PASSES; ++pass) {
        const int shift = 56 - 8 * pass;
        std::fill(hist.begin(), hist.end(), 0);
        for (int64_t i = 0; i < n; ++i) {
            u64 bits;
            std::memcpy(&bits, x + i * stride, 8);
            const u64 key = sel_key(bits), hi = pass ? key >> (shift + 8) : 0;
            const unsigned digit = (unsigned)(key >> shift) & 255u;
            for (int r = 0; r < nr; ++r)
                if (leader[r] == r && (pass ? prefix[r] >> (shift + 8) : 0) == hi) ++hist[(size_t)r * 256 + digit];
        }
        for (int r = 0; r < nr; ++r) prefix[r] |= (u64)sel_scan_bins(&hist[(size_t)leader[r] * 256], &rem[r]) << shift;
        sel_leaders(prefix, leader, nr);
    }
    for (int r = 0; r < nr; ++r) {
        const u64 bits = sel_unkey(prefix[r]);
        std::memcpy(out + r, &bits, 8);
    }
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop

// ---- every member's histograms --------------------------------------------------------------------------------------------
namespace {

#define BHIST_HIP(what, expr)                                                                                          \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) return sfail(b, -2, "%s: %s: %s", fn, what, hipGetErrorString(e_));                      \
    } while (0)

int bgrow(emx_batch* b, const char* fn, Buf& u, size_t bytes, const char* what) {
    if (bytes <= u.bytes) return 0;
    if (u.p) hipFree(u.p);
    u.p = nullptr;
    u.bytes = 0;
    const hipError_t e = hipMalloc(&u.p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sfail(b, -2, "%s: %s allocation (%zu bytes): %s", fn, what, bytes, hipGetErrorString(e));
    }
    u.bytes = bytes;
    return 0;
}

// The selection of both entry points: the plane, the members and the rows start, start + stride, ... < stop, checked as
// emx_summary_batch_plane checks them.  *x: member_lo's first selected row; *W: the plane's width; *nt: selected rows.
int bh_selection(emx_batch* b, const char* fn, const EmxBatchView& v, int32_t plane, int32_t member_lo, int32_t member_hi, int64_t start,
                 int64_t stop, int64_t stride, const double** x, int64_t* W, int64_t* nt) {
    if (plane != 0 && plane != 4) return sfail(b, -1, "%s: plane 0 (coordinates) or 4 (blobs); got %d", fn, plane);
    const double* X = v.chain;
    *W = v.D;
    if (plane == 4) {
        if (v.nblobs < 1) return sfail(b, -1, "%s: the handle's target has no blobs", fn);
        X = v.chain_blobs;
        *W = v.nblobs;
    }
    if (!(0 <= member_lo && member_lo < member_hi && member_hi <= v.B))
        return sfail(b, -1, "%s: members [%d, %d) outside [0, %d) or empty", fn, member_lo, member_hi, v.B);
    if (!X || v.stored <= 0) return sfail(b, -1, "%s: no stored chain (emx_batch_chain_config + a stored run)", fn);
    if (stride < 1 || start < 0 || stop > v.stored) return sfail(b, -1, "%s: rows need 0 <= start, stop <= stored, stride >= 1", fn);
    *nt = start < stop ? (stop - start + stride - 1) / stride : 0;
    if (*nt < 1) return sfail(b, -1, "%s: the selection is empty", fn);
    *x = X + ((int64_t)member_lo * v.cap + start) * v.N * *W;
    return 0;
}

// eh_check_edges for members [0, M) of a batch: member m's edges at e + m step
int bh_check_edges(emx_batch* b, const char* fn, const char* what, const int64_t* off, const double* e, int64_t step, int64_t M, int64_t W,
                   int maxbins) {
    if (!off || !e) return sfail(b, -1, "%s: the %s edges and their offsets are needed", fn, what);
    if (off[0] != 0) return sfail(b, -1, "%s: the %s edge offsets start at 0", fn, what);
    for (int64_t d = 0; d < W; ++d) {
        const int64_t nb = off[d + 1] - off[d] - 1;
        if (nb < 1 || nb > maxbins) return sfail(b, -1, "%s: column %lld has %lld %s bins; 1 ... %d", fn, (long long)d, (long long)nb, what, maxbins);
    }
    if (step != 0 && step < off[W]) return sfail(b, -1, "%s: the %s edges of a member lie %lld doubles apart; 0 (shared) or at least %lld", fn, what, (long long)step, (long long)off[W]);
    for (int64_t m = 0; m < (step ? M : 1); ++m) {
        const double* em = e + m * step;
        for (int64_t d = 0; d < W; ++d)
            for (int64_t i = off[d]; i < off[d + 1]; ++i)
                if (em[i] != em[i] || (i > off[d] && !(em[i] > em[i - 1])))
                    return sfail(b, -1, "%s: the %s edges of column %lld of member %lld of the range are not strictly increasing", fn, what, (long long)d, (long long)m);
    }
    return 0;
}

// members [m0, m0 + mc) of a per-member host table (rows of `row` doubles, `step` apart; step 0: one shared row) -> dev, packed
int bh_upload(emx_batch* b, const char* fn, hipStream_t st, void* dev, const double* host, int64_t step, int64_t row, int64_t m0, int64_t mc,
              std::vector<double>& stage) {
    if (step == 0) return 0;             // the shared row went up once, before the chunks
    const double* src = host + m0 * step;
    if (step != row) {
        stage.resize((size_t)mc * row);
        for (int64_t m = 0; m < mc; ++m) std::memcpy(&stage[(size_t)m * row], src + m * step, (size_t)row * 8);
        src = stage.data();
    }
    BHIST_HIP("copy", hipMemcpyAsync(dev, src, (size_t)mc * row * 8, hipMemcpyHostToDevice, st));
    return 0;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int emx_chain_minmax_batch(emx_batch* b, int32_t plane, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop, int64_t stride,
                           double* lo_out, double* hi_out, int64_t* nonfinite_out) {
    const char* fn = "emx_chain_minmax_batch";
    EmxBatchView v;
    if (emx_internal_batch_view(b, &v)) return -1;
    const double* x = nullptr;
    int64_t W = 0, nt = 0;
    if (const int rc = bh_selection(b, fn, v, plane, member_lo, member_hi, start, stop, stride, &x, &W, &nt)) return rc;
    if (!lo_out || !hi_out || !nonfinite_out) return sfail(b, -1, "%s: the three outputs are needed", fn);
    const int64_t N = v.N, n = nt * N, M = member_hi - member_lo;
    BHIST_HIP("hipSetDevice", hipSetDevice(v.device));
    if (!*v.summary) *v.summary = new BatchSummary();
    BatchSummary* a = *v.summary;
    const hipStream_t st = v.stream;
    const int CW = (int)std::min<int64_t>(W, 256), SPB = 256 / CW;
    const int64_t mp = std::min<int64_t>(M, 65535);                    // members a launch: grid.z
    // slices: about 2 048 workgroups from the members of a launch, a slice no shorter than 16 rounds of the workgroup's lanes
    const int64_t ctiles = (W + CW - 1) / CW;
    int64_t S = std::max<int64_t>(1, std::min<int64_t>((2048 + mp * ctiles - 1) / (mp * ctiles), (n + 16 * SPB - 1) / (16 * SPB)));
    S = std::min<int64_t>(S, 65535);
    const int64_t per = (n + S - 1) / S;
    S = (n + per - 1) / per;
    for (Buf* u : {&a->h_plo, &a->h_phi, &a->h_pnf})
        if (int rc = bgrow(b, fn, *u, (size_t)mp * S * W * 8, "min / max partials")) return rc;
    for (Buf* u : {&a->h_lo, &a->h_hi, &a->h_nf})
        if (int rc = bgrow(b, fn, *u, (size_t)mp * W * 8, "min / max")) return rc;
    BHMinMax g;
    g.xstep = v.cap * N * W;
    g.N = N;
    g.rowstep = stride * N * W;
    g.n = n;
    g.per = per;
    g.W = (int32_t)W;
    g.S = (int32_t)S;
    for (int64_t m0 = 0; m0 < M; m0 += mp) {
        const int64_t mc = std::min<int64_t>(mp, M - m0);
        g.x = x + m0 * g.xstep;
        hipLaunchKernelGGL(k_bhist_minmax, dim3((unsigned)S, (unsigned)ctiles, (unsigned)mc), dim3(256), 0, st, g, CW, (double*)a->h_plo.p,
                           (double*)a->h_phi.p, (u64*)a->h_pnf.p);
        BHIST_HIP("min / max launch", hipGetLastError());
        hipLaunchKernelGGL(k_bhist_minmax_fin, dim3((unsigned)((mc * W + 255) / 256)), dim3(256), 0, st, (const double*)a->h_plo.p,
                           (const double*)a->h_phi.p, (const u64*)a->h_pnf.p, S, W, mc * W, (double*)a->h_lo.p, (double*)a->h_hi.p, (u64*)a->h_nf.p);
        BHIST_HIP("min / max launch", hipGetLastError());
        BHIST_HIP("copy", hipMemcpyAsync(lo_out + m0 * W, a->h_lo.p, (size_t)mc * W * 8, hipMemcpyDeviceToHost, st));
        BHIST_HIP("copy", hipMemcpyAsync(hi_out + m0 * W, a->h_hi.p, (size_t)mc * W * 8, hipMemcpyDeviceToHost, st));
        BHIST_HIP("copy", hipMemcpyAsync(nonfinite_out + m0 * W, a->h_nf.p, (size_t)mc * W * 8, hipMemcpyDeviceToHost, st));
        BHIST_HIP("synchronize", hipStreamSynchronize(st));          // the outputs leave before the next launch reuses the buffers
    }
    return 0;
}

int emx_histograms_batch(emx_batch* b, int32_t plane, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop, int64_t stride,
                         const int64_t* edge_off, const double* edges, int64_t edge_member_stride, int64_t* counts_out,
                         const int64_t* pedge_off, const double* pedges, int64_t pedge_member_stride, int64_t npairs, const int32_t* pairs,
                         const int64_t* pair_off, int64_t* pair_counts_out, int64_t* nsamples_out) {
    const char* fn = "emx_histograms_batch";
    EmxBatchView v;
    if (emx_internal_batch_view(b, &v)) return -1;
    const double* x = nullptr;
    int64_t W = 0, nt = 0;
    if (const int rc = bh_selection(b, fn, v, plane, member_lo, member_hi, start, stop, stride, &x, &W, &nt)) return rc;
    const int64_t N = v.N, M = member_hi - member_lo, P = npairs, es = edge_member_stride, ps = P ? pedge_member_stride : 0;
    if (nsamples_out) *nsamples_out = nt * N;
    if (!counts_out) return sfail(b, -1, "%s: counts_out is needed", fn);
    if (es < 0 || ps < 0) return sfail(b, -1, "%s: the member strides of the edges are 0 (shared) or positive", fn);
    if (const int rc = bh_check_edges(b, fn, "marginal", edge_off, edges, es, M, W, EH_MAX_BINS)) return rc;
    if (P < 0 || P > 0x7fffffff) return sfail(b, -1, "%s: %lld pairs", fn, (long long)P);
    if (P > 0) {
        if (!pairs || !pair_off || !pair_counts_out) return sfail(b, -1, "%s: pairs, pair_off and pair_counts_out are needed with npairs > 0", fn);
        if (const int rc = bh_check_edges(b, fn, "pair", pedge_off, pedges, ps, M, W, EH_MAX_PAIR_BINS)) return rc;
        if (pair_off[0] != 0) return sfail(b, -1, "%s: the pair offsets start at 0", fn);
        for (int64_t p = 0; p < P; ++p) {
            const int64_t i = pairs[2 * p], j = pairs[2 * p + 1];
            if (i < 0 || i >= W || j < 0 || j >= W || i == j)
                return sfail(b, -1, "%s: pair %lld is (%lld, %lld); two different columns of [0, %lld)", fn, (long long)p, (long long)i, (long long)j, (long long)W);
            const int64_t want = (pedge_off[i + 1] - pedge_off[i] - 1) * (pedge_off[j + 1] - pedge_off[j] - 1);
            if (pair_off[p + 1] - pair_off[p] != want)
                return sfail(b, -1, "%s: pair %lld has room for %lld counters, its panel has %lld", fn, (long long)p, (long long)(pair_off[p + 1] - pair_off[p]), (long long)want);
        }
    }
    const int64_t nme = edge_off[W], npe = P ? pedge_off[W] : 0, ncnt = nme - W, npc = P ? pair_off[P] : 0;
    // one search a value where every member's pair edges are its marginal edges
    bool same = P > 0 && !std::memcmp(edge_off, pedge_off, (size_t)(W + 1) * 8) && (es == 0) == (ps == 0);
    for (int64_t m = 0; same && m < (es ? M : 1); ++m) same = !std::memcmp(edges + m * es, pedges + m * ps, (size_t)nme * 8);
    // column tiles: as many consecutive columns as EH_LDS_TABLES hold
    std::vector<EHTileSpan> tiles;
    size_t lds_max = 0;
    for (int64_t d0 = 0; d0 < W;) {
        int64_t d1 = d0;
        size_t bytes = 0;
        while (d1 < W && d1 - d0 < EH_MAX_TILE_COLS) {
            const int64_t nb = edge_off[d1 + 1] - edge_off[d1] - 1, pb = (P && !same) ? pedge_off[d1 + 1] - pedge_off[d1] - 1 : -1;
            const size_t add = (size_t)(nb + 1) * 8 + (size_t)(pb + 1) * 8 + (size_t)nb * 4;
            if (d1 > d0 && bytes + add > EH_LDS_TABLES) break;
            bytes += add;
            ++d1;
        }
        EHTileSpan t;
        t.d0 = (int)d0;
        t.dc = (int)(d1 - d0);
        t.lds = eh_code_lds(edge_off[d1] - edge_off[d0], (P && !same) ? pedge_off[d1] - pedge_off[d0] : 0, t.dc, P > 0);
        lds_max = std::max(lds_max, t.lds);
        tiles.push_back(t);
        d0 = d1;
    }
    // Chunks.  Rows: R selected rows of a member at a time, all of them unless the code plane of ONE member exceeds the budget
    // (or "batch_hist_rows" says otherwise).  Members: mp at a time, so that the chunk's code plane, edges and counters stay near
    // 256 MB (or "batch_hist_members").
    const int64_t budget = (int64_t)256 << 20;
    int64_t R = v.hist_rows > 0 ? v.hist_rows : (P ? std::max<int64_t>(1, budget / (N * W)) : nt);
    R = std::min<int64_t>(R, nt);
    while (R * N > ((int64_t)1 << 40)) R = (R + 1) / 2;
    const int64_t Mp = (R * N + 15) / 16 * 16;
    const int64_t per_member = (P ? W * Mp : 0) + (nme + npe + ncnt + npc) * 8;
    int64_t mp = std::max<int64_t>(1, budget / per_member);
    if (v.hist_members > 0) mp = v.hist_members;
    mp = std::min<int64_t>(mp, std::min<int64_t>(M, 65535));

    BHIST_HIP("hipSetDevice", hipSetDevice(v.device));
    if (!*v.summary) *v.summary = new BatchSummary();
    BatchSummary* a = *v.summary;
    const hipStream_t st = v.stream;
    if (int rc = bgrow(b, fn, a->h_edges, (size_t)(es ? mp : 1) * nme * 8, "edges")) return rc;
    if (int rc = bgrow(b, fn, a->h_eoff, (size_t)(W + 1) * 8, "edge offsets")) return rc;
    if (int rc = bgrow(b, fn, a->h_counts, (size_t)mp * ncnt * 8, "counters")) return rc;
    BHIST_HIP("copy", hipMemcpyAsync(a->h_eoff.p, edge_off, (size_t)(W + 1) * 8, hipMemcpyHostToDevice, st));
    if (!es) BHIST_HIP("copy", hipMemcpyAsync(a->h_edges.p, edges, (size_t)nme * 8, hipMemcpyHostToDevice, st));
    size_t pair_lds = 0;
    if (P) {
        if (int rc = bgrow(b, fn, a->h_pedges, (size_t)(ps ? mp : 1) * npe * 8, "pair edges")) return rc;
        if (int rc = bgrow(b, fn, a->h_poff, (size_t)(W + 1) * 8, "pair edge offsets")) return rc;
        if (int rc = bgrow(b, fn, a->h_pairs, (size_t)P * 8, "pairs")) return rc;
        if (int rc = bgrow(b, fn, a->h_pairoff, (size_t)(P + 1) * 8, "pair offsets")) return rc;
        if (int rc = bgrow(b, fn, a->h_pcounts, (size_t)mp * npc * 8, "pair counters")) return rc;
        if (int rc = bgrow(b, fn, a->h_codes, (size_t)mp * W * Mp, "bin codes")) return rc;
        BHIST_HIP("copy", hipMemcpyAsync(a->h_poff.p, pedge_off, (size_t)(W + 1) * 8, hipMemcpyHostToDevice, st));
        BHIST_HIP("copy", hipMemcpyAsync(a->h_pairs.p, pairs, (size_t)P * 8, hipMemcpyHostToDevice, st));
        BHIST_HIP("copy", hipMemcpyAsync(a->h_pairoff.p, pair_off, (size_t)(P + 1) * 8, hipMemcpyHostToDevice, st));
        if (!ps) BHIST_HIP("copy", hipMemcpyAsync(a->h_pedges.p, pedges, (size_t)npe * 8, hipMemcpyHostToDevice, st));
        for (int64_t p = 0; p < P; ++p) pair_lds = std::max(pair_lds, (size_t)(pair_off[p + 1] - pair_off[p]) * 4);
        static size_t pair_granted[EH_MAX_DEVICES] = {};
        BHIST_HIP("LDS size", eh_grant_lds((const void*)k_bhist_pair, pair_granted, v.device, pair_lds));
    }
    static size_t code_granted[EH_MAX_DEVICES] = {};
    BHIST_HIP("LDS size", eh_grant_lds((const void*)k_bhist_code, code_granted, v.device, lds_max));

    const int64_t xstep = v.cap * N * W, rowstep = stride * N * W;
    std::vector<double> estage, pstage;
    a->h_launches = 0;
    for (int64_t m0 = 0; m0 < M; m0 += mp) {
        const int64_t mc = std::min<int64_t>(mp, M - m0);
        if (int rc = bh_upload(b, fn, st, a->h_edges.p, edges, es, nme, m0, mc, estage)) return rc;
        if (P)
            if (int rc = bh_upload(b, fn, st, a->h_pedges.p, pedges, ps, npe, m0, mc, pstage)) return rc;
        BHIST_HIP("memset", hipMemsetAsync(a->h_counts.p, 0, (size_t)mc * ncnt * 8, st));
        if (P) BHIST_HIP("memset", hipMemsetAsync(a->h_pcounts.p, 0, (size_t)mc * npc * 8, st));
        for (int64_t r0 = 0; r0 < nt; r0 += R) {
            const int64_t Ms = std::min<int64_t>(R, nt - r0) * N;             // samples of a member in this chunk of rows
            for (const EHTileSpan& t : tiles) {
                // slices: about 2 048 workgroups from the mc members, a workgroup at least two rounds of TS samples where there are
                // two, at most 2^30 samples (its LDS counters are uint32) and grid.x in bounds
                const int64_t TS = (int64_t)EH_K * (EH_T / t.dc), rounds = (Ms + TS - 1) / TS;
                int64_t wg = std::max<int64_t>(1, std::min<int64_t>((2048 + mc - 1) / mc, (rounds + 1) / 2));
                wg = std::max<int64_t>(wg, (Ms + ((int64_t)1 << 30) - 1) >> 30);
                BHCode k;
                k.x = x + m0 * xstep + r0 * rowstep;
                k.xstep = xstep;
                k.N = N;
                k.rowstep = rowstep;
                k.M = Ms;
                k.per = ((Ms + wg - 1) / wg + TS - 1) / TS * TS;
                k.W = (int32_t)W;
                k.d0 = t.d0;
                k.dc = t.dc;
                k.same = same ? 1 : 0;
                k.edge_off = (const int64_t*)a->h_eoff.p;
                k.pedge_off = (const int64_t*)a->h_poff.p;
                k.edges = (const double*)a->h_edges.p;
                k.pedges = (const double*)a->h_pedges.p;
                k.estep = es ? nme : 0;
                k.pstep = ps ? npe : 0;
                k.counts = (u64*)a->h_counts.p;
                k.cstep = ncnt;
                k.codes = P ? (uint8_t*)a->h_codes.p : nullptr;
                k.Mp = Mp;
                hipLaunchKernelGGL(k_bhist_code, dim3((unsigned)((Ms + k.per - 1) / k.per), (unsigned)mc), dim3(EH_T), t.lds, st, k);
                BHIST_HIP("binning launch", hipGetLastError());
                ++a->h_launches;
            }
            if (P) {
                // slices: enough workgroups for the device where panels x members are few; a slice stays below 2^31 samples and
                // grid.y below 65 536
                int64_t slices = std::max<int64_t>(1, std::min<int64_t>((2048 + P * mc - 1) / (P * mc), (Ms + 16383) / 16384));
                slices = std::max<int64_t>(slices, (Ms + ((int64_t)1 << 31) - 1) >> 31);
                BHPair k;
                k.codes = (const uint8_t*)a->h_codes.p;
                k.Mp = Mp;
                k.M = Ms;
                k.per = ((Ms + slices - 1) / slices + 15) / 16 * 16;
                k.W = (int32_t)W;
                const int64_t ny = (Ms + k.per - 1) / k.per;
                k.store = (ny == 1 && R >= nt) ? 1 : 0;
                k.pairs = (const int32_t*)a->h_pairs.p;
                k.pair_off = (const int64_t*)a->h_pairoff.p;
                k.pedge_off = (const int64_t*)a->h_poff.p;
                k.out = (u64*)a->h_pcounts.p;
                k.ostep = npc;
                hipLaunchKernelGGL(k_bhist_pair, dim3((unsigned)P, (unsigned)ny, (unsigned)mc), dim3(256), pair_lds, st, k);
                BHIST_HIP("pair launch", hipGetLastError());
                ++a->h_launches;
            }
        }
        BHIST_HIP("copy", hipMemcpyAsync(counts_out + m0 * ncnt, a->h_counts.p, (size_t)mc * ncnt * 8, hipMemcpyDeviceToHost, st));
        if (P) BHIST_HIP("copy", hipMemcpyAsync(pair_counts_out + m0 * npc, a->h_pcounts.p, (size_t)mc * npc * 8, hipMemcpyDeviceToHost, st));
        // the chunk's counts leave (and its staged edges are consumed) before the next chunk reuses the buffers
        BHIST_HIP("synchronize", hipStreamSynchronize(st));
    }
    return 0;
}

int emx_histograms_batch_info(emx_batch* b, int64_t* launches_out) {
    EmxBatchView v;
    if (emx_internal_batch_view(b, &v)) return -1;
    const BatchSummary* a = *v.summary;
    if (launches_out) *launches_out = a ? a->h_launches : 0;
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
