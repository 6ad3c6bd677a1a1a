// libemx, emx_rhat_batch / emx_rhat: the split-R-hat of Gelman and Rubin (BDA3 section 11.4, the Stan reference manual) computed
// next to the chain.  Only O(groups ndim) doubles cross to the host.
//
// Definition (emcee_amd.summary.split_rhat is the same on a host array):
//   Selection   the one get_chain(discard, thin) makes: stored rows t0 + t stride, t = 0 ... nt - 1.  h = nt / 2 (integer).  Every
//               series is split into its first h selected samples and its last h; the middle one is dropped when nt is odd.
//               nt < 4 is an error.
//   Series      one walker's values of one parameter.  A group holds C = 2 x (walkers pooled) half-series ("chains") of length h.
//   Outputs     per group and parameter, with mu_c the chain means and s_c^2 the chain variances (ddof = 1):
//                 within  = mean_c s_c^2
//                 between = var_c(mu_c, ddof = 1)
//                 rhat    = sqrt((h - 1) / h + between / within)
//               within and between come from here; rhat is formed on the host from the two by exactly that expression.  A
//               constant group gives 0 / 0 = NaN, a non-finite sample NaN; neither is an error.
//   Grouping    pool = 0: every member is a group, its N walkers the chains (C = 2 N).  pool = P > 0: members with equal
//               (m - first member) mod P are pooled into P groups (a batch of replicates: 1; a tempered handle: ntemps).
//   log_prob    the same statistic of the stored log-prob series as one more column: the kernels run on chain_lp, one column a walker.
//
// Layout: the N D doubles of a stored step are contiguous, so a lane takes a series column j = w D + d and a wave reads 64
// neighbouring doubles of a row.  The h selected rows of each half are cut into S slices of R rows, R and S fixed by nt alone, so a
// long chain of a small ensemble still fills the chip.  Members go in passes of at most "batch_rhat_members".  The kernels take
// (plane, cap, N, width, first member), not the handle: emx_rhat runs them on one context's chain as one member.  Per pass
//   k_rhat_part<0>   part[member][half][slice][j] = sum over the slice's rows of x - x0, x0 the chain's first sample; the 4 waves of
//                    a workgroup take consecutive quarters of the slice and are added in wave order
//   k_rhat_centre    mu0 = x0 + (sum over slices in order) / h: the centre, within u |mu| + h u spread of the chain's mean (and
//                    exactly the value of a constant chain)
//   k_rhat_part<1>   with d = x - mu0:  r = sum d  and  G = sum d^2 (an explicit fma; the file is built with -ffp-contract=off,
//                    nothing else is fused), per slice as above
//   k_rhat_chain     q = r / h, the chain mean being mu0 + q, and the corrected two-pass variance s^2 = (G - r^2 / h) / (h - 1):
//                    the shape of k_bsum_gram_fin_* -- the centre's rounding error, which is relative to |mean|, drops out
//   k_rhat_head      the group's centre c0 = mu0 of its first chain (first member, walker 0, first half), kept for later passes
//   k_rhat_walkers   per (member, column d): over the walkers in order, the two halves of each,  W = sum s^2,  E1 = sum e  and
//                    E2 = sum e^2 (fma) of the residual chain means e = (mu0 - c0) + q about the group's common centre, in at most
//                    1 024 runs of consecutive walkers, the length of a run fixed by N; a lane takes a column d, so a wave reads
//                    neighbouring doubles
//   k_rhat_member    the runs' sums: consecutive sixteenths of the runs in run order, then the sixteenths in order
//   k_rhat_group     after the last pass, per (group, column): the members' (W, E1, E2) in member order;  within = W / C,
//                    between = (E2 - E1^2 / C) / (C - 1), the corrected form again, so that nothing is relative to |mean|
// No floating-point atomics.  Every sum runs in an order fixed by (nt, N, D, pool): no bit depends on the member range (pool = 0),
// the pass size or the launch shape.  Scratch stays on the context / the batch handle between calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../include/emx.h"
#include "emx_internal.hpp"

namespace {

constexpr int64_t RH_SLICE_ROWS = 128;      // rows a slice (doubled while a half has more than 65 535 slices)

// One launch covers members m0 ... of the plane x (., cap, N W): blockIdx.z = 2 ml + half, blockIdx.y = slice.  Half 0 holds the
// selected rows [0, h), half 1 the rows [nt - h, nt); selected row t is stored row t0 + t stride.
struct RSel {
    const double* x;
    int64_t cap, N, NW, t0, stride, nt, h, R, m0;
    int32_t W, S;
};

__device__ __forceinline__ const double* rh_chain(const RSel& g, int64_t z, int64_t j) {
    const int64_t ml = z >> 1, first = (z & 1) ? g.nt - g.h : 0;
    return g.x + ((g.m0 + ml) * g.cap + g.t0 + first * g.stride) * g.NW + j;
}

// SECOND = 0: part (mp 2, S, NW) sums of x - x0.  SECOND = 1: part (mp 2, S, 2, NW) sums of d and of d^2, d = x - mu0[z][j]
template <int SECOND>
__global__ __launch_bounds__(256) void k_rhat_part(const RSel g, const double* __restrict__ mu0, double* __restrict__ part) {
    __shared__ double red[2][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane, s = blockIdx.y, z = blockIdx.z;
    const int64_t ra = s * g.R, rb = ra + g.R < g.h ? ra + g.R : g.h;
    const int64_t q = g.R / 4, ta = ra + wv * q, tb = ta + q < rb ? ta + q : rb;
    double r = 0.0, G = 0.0;
    if (j < g.NW) {
        const double* p = rh_chain(g, z, j);
        const int64_t step = g.stride * g.NW;
        const double c = SECOND ? mu0[z * g.NW + j] : p[0];
#pragma unroll 8
        for (int64_t t = ta; t < tb; ++t) {
            const double d = p[t * step] - c;
            r += d;
            if (SECOND) G = fma(d, d, G);
        }
    }
    red[0][wv][lane] = r;
    if (SECOND) red[1][wv][lane] = G;
    __syncthreads();
    if (wv == 0 && j < g.NW) {
        double* out = part + (z * g.S + s) * (SECOND ? 2 : 1) * g.NW + j;
        out[0] = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
        if (SECOND) out[g.NW] = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
    }
}

// one thread a chain (z, j) of the pass: mu0 (mp 2, NW)
__global__ __launch_bounds__(256) void k_rhat_centre(const RSel g, const double* __restrict__ part, double* __restrict__ mu0, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t z = i / g.NW, j = i - z * g.NW;
    double acc = 0.0;
    for (int64_t s = 0; s < g.S; ++s) acc += part[(z * g.S + s) * g.NW + j];
    mu0[i] = rh_chain(g, z, j)[0] + acc / (double)g.h;
}

// one thread a chain: q = r / h and the corrected two-pass variance, both (mp 2, NW)
__global__ __launch_bounds__(256) void k_rhat_chain(const RSel g, const double* __restrict__ part, double* __restrict__ q, double* __restrict__ var,
                                                    int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t z = i / g.NW, j = i - z * g.NW;
    double r = 0.0, G = 0.0;
    for (int64_t s = 0; s < g.S; ++s) {
        const double* p = part + (z * g.S + s) * 2 * g.NW + j;
        r += p[0];
        G += p[g.NW];
    }
    const double h = (double)g.h;
    q[i] = r / h;
    var[i] = (G - r * r / h) / (h - 1.0);
}

// the first `heads` members of the pass are the first of their groups: cen (groups, W) row mo + ml = mu0 of (ml, half 0, walker 0)
__global__ __launch_bounds__(256) void k_rhat_head(const double* __restrict__ mu0, double* __restrict__ cen, int64_t NW, int W, int64_t mo,
                                                   int64_t heads) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= heads * W) return;
    const int64_t ml = i / W, d = i - ml * W;
    cen[(mo + ml) * W + d] = mu0[ml * 2 * NW + d];
}

// A member's walkers are cut into at most RH_RUNS runs of `run` consecutive walkers, run = ceil(N / RH_RUNS).
// blockIdx.x = run i, blockIdx.y = ml; a thread takes columns d = threadIdx.x, + blockDim.x, ..., so that a wave reads
// neighbouring doubles: wpart (mp, runs, 3, W) = the run's sums of s^2, e and e^2 over its walkers in order, the two halves of each
__global__ __launch_bounds__(256) void k_rhat_walkers(const double* __restrict__ mu0, const double* __restrict__ q, const double* __restrict__ var,
                                                      const double* __restrict__ cen, double* __restrict__ wpart, int64_t N, int W, int64_t run,
                                                      int64_t mo, int64_t pool) {
    const int64_t i = blockIdx.x, runs = gridDim.x, ml = blockIdx.y, m = mo + ml, NW = N * W;
    const int64_t wa = i * run, wb = wa + run < N ? wa + run : N;
    for (int d = threadIdx.x; d < W; d += blockDim.x) {
        const double c0 = cen[(pool ? m % pool : m) * W + d];
        double Ws = 0.0, E1 = 0.0, E2 = 0.0;
        int64_t at = ml * 2 * NW + wa * W + d;      // half 0 of walker wa; half 1 is NW further
#pragma unroll 2
        for (int64_t w = wa; w < wb; ++w, at += W) {
            const double e0 = (mu0[at] - c0) + q[at], e1 = (mu0[at + NW] - c0) + q[at + NW];
            Ws += var[at];
            E1 += e0;
            E2 = fma(e0, e0, E2);
            Ws += var[at + NW];
            E1 += e1;
            E2 = fma(e1, e1, E2);
        }
        double* out = wpart + ((ml * runs + i) * 3) * W + d;
        out[0] = Ws;
        out[W] = E1;
        out[2 * W] = E2;
    }
}

// mem (members, 3, W) row mo + ml = the runs' sums: 16 threads an element (member, sum, column) take consecutive sixteenths of the
// runs in order and are added in that order; a workgroup holds 16 neighbouring elements
__global__ __launch_bounds__(256) void k_rhat_member(const double* __restrict__ wpart, double* __restrict__ mem, int64_t runs, int W, int64_t mo,
                                                     int64_t count) {
    __shared__ double red[16][16];
    const int col = threadIdx.x & 15, sec = threadIdx.x >> 4;
    const int64_t i = (int64_t)blockIdx.x * 16 + col, width = 3 * (int64_t)W;
    const int64_t ml = i / width, kd = i - ml * width;
    const int64_t per = (runs + 15) / 16, ra = sec * per, rb = ra + per < runs ? ra + per : runs;
    double tot = 0.0;
    if (i < count)
        for (int64_t r = ra; r < rb; ++r) tot += wpart[(ml * runs + r) * width + kd];
    red[sec][col] = tot;
    __syncthreads();
    if (sec == 0 && i < count) {
        double sum = 0.0;
        for (int s = 0; s < 16; ++s) sum += red[s][col];
        mem[(mo + ml) * width + kd] = sum;
    }
}

// one thread a (group, column): within / between (groups, ldo) at column col0 + d
__global__ __launch_bounds__(256) void k_rhat_group(const double* __restrict__ mem, double* __restrict__ within, double* __restrict__ between,
                                                    int64_t M, int64_t groups, int64_t N, int W, int ldo, int col0) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= groups * W) return;
    const int64_t gi = i / W, d = i - gi * W;
    double Ws = 0.0, E1 = 0.0, E2 = 0.0;
#pragma unroll 4
    for (int64_t m = gi; m < M; m += groups) {
        Ws += mem[(m * 3 + 0) * W + d];
        E1 += mem[(m * 3 + 1) * W + d];
        E2 += mem[(m * 3 + 2) * W + d];
    }
    const double C = (double)(2 * N * (M / groups));
    within[gi * ldo + col0 + d] = Ws / C;
    between[gi * ldo + col0 + d] = (E2 - E1 * E1 / C) / (C - 1.0);
}

}  // namespace

// ---- host -----------------------------------------------------------------------------------------------------------
// the scratch of a context or a batch handle: buffers that only grow, freed with their owner
struct RhatScratch {
    enum { PART, MU0, Q, VAR, CEN, MEM, WPART, WITHIN, BETWEEN, COUNT };
    void* p[COUNT] = {};
    size_t bytes[COUNT] = {};
    hipError_t get(int which, double** out, size_t doubles) {
        const size_t need = std::max<size_t>(doubles, 1) * 8;
        if (need > bytes[which]) {
            if (p[which]) (void)hipFree(p[which]);
            p[which] = nullptr;
            bytes[which] = 0;
            const hipError_t e = hipMalloc(&p[which], need);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return e;
            }
            bytes[which] = need;
        }
        *out = (double*)p[which];
        return hipSuccess;
    }
};

void emx_internal_rhat_release(RhatScratch* s) {
    if (!s) return;
    for (void* q : s->p)
        if (q) (void)hipFree(q);
    delete s;
}

namespace {

constexpr int64_t RH_RUNS = 1024;      // runs of walkers a member (k_rhat_walkers)

struct Plan {
    RhatScratch* sc;
    const double* x;      // the coordinates' plane (., cap, N, D)
    const double* lp;     // the log-prob plane (., cap, N)
    int64_t cap, N, D, lo, hi, pool, start, stride, nt, members_per_pass;
    bool log_prob;
    hipStream_t stream;
};

#define RH_HIP(what, expr)                                                                                             \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                        \
            snprintf(err, errlen, "%s: %s", what, hipGetErrorString(e_));                                              \
            return -2;                                                                                                 \
        }                                                                                                              \
    } while (0)

// one plane of width W into columns [col0, col0 + W) of the device outputs (groups, ldo)
int rh_plane(const Plan& pl, const double* x, int64_t W, double* within, double* between, int ldo, int col0, char* err, size_t errlen) {
    const int64_t M = pl.hi - pl.lo, groups = pl.pool ? pl.pool : M, NW = pl.N * W, h = pl.nt / 2;
    int64_t R = RH_SLICE_ROWS;
    while ((h + R - 1) / R > 65535) R *= 2;
    const int64_t S = (h + R - 1) / R;
    const size_t per_member = (size_t)2 * NW * (2 * S + 3) * 8;
    int64_t mp = std::max<int64_t>(1, (int64_t)(((size_t)512 << 20) / per_member));
    mp = std::min<int64_t>(mp, std::min<int64_t>(M, 32767));      // grid.z = 2 mp
    if (pl.members_per_pass > 0) mp = std::min<int64_t>(mp, pl.members_per_pass);

    const int64_t run = (pl.N + RH_RUNS - 1) / RH_RUNS, runs = (pl.N + run - 1) / run;
    RhatScratch& sc = *pl.sc;
    double *part, *mu0, *q, *var, *cen, *mem, *wpart;
    RH_HIP("slab allocation", sc.get(RhatScratch::PART, &part, (size_t)mp * 2 * S * 2 * NW));
    RH_HIP("chain centres allocation", sc.get(RhatScratch::MU0, &mu0, (size_t)mp * 2 * NW));
    RH_HIP("chain means allocation", sc.get(RhatScratch::Q, &q, (size_t)mp * 2 * NW));
    RH_HIP("chain variances allocation", sc.get(RhatScratch::VAR, &var, (size_t)mp * 2 * NW));
    RH_HIP("group centres allocation", sc.get(RhatScratch::CEN, &cen, (size_t)groups * W));
    RH_HIP("member sums allocation", sc.get(RhatScratch::MEM, &mem, (size_t)M * 3 * W));
    RH_HIP("walker sums allocation", sc.get(RhatScratch::WPART, &wpart, (size_t)mp * runs * 3 * W));

    RSel g;
    g.x = x;
    g.cap = pl.cap;
    g.N = pl.N;
    g.NW = NW;
    g.t0 = pl.start;
    g.stride = pl.stride;
    g.nt = pl.nt;
    g.h = h;
    g.R = R;
    g.W = (int32_t)W;
    g.S = (int32_t)S;
    auto blocks = [](int64_t count) { return dim3((unsigned)((count + 255) / 256)); };
    const hipStream_t st = pl.stream;
    for (int64_t m0 = pl.lo; m0 < pl.hi; m0 += mp) {
        const int64_t mc = std::min<int64_t>(mp, pl.hi - m0), mo = m0 - pl.lo, chains = mc * 2 * NW;
        g.m0 = m0;
        const dim3 slices((unsigned)((NW + 63) / 64), (unsigned)S, (unsigned)(2 * mc));
        hipLaunchKernelGGL(k_rhat_part<0>, slices, dim3(256), 0, st, g, (const double*)nullptr, part);
        RH_HIP("first pass launch", hipGetLastError());
        hipLaunchKernelGGL(k_rhat_centre, blocks(chains), dim3(256), 0, st, g, (const double*)part, mu0, chains);
        RH_HIP("centre launch", hipGetLastError());
        hipLaunchKernelGGL(k_rhat_part<1>, slices, dim3(256), 0, st, g, (const double*)mu0, part);
        RH_HIP("second pass launch", hipGetLastError());
        hipLaunchKernelGGL(k_rhat_chain, blocks(chains), dim3(256), 0, st, g, (const double*)part, q, var, chains);
        RH_HIP("chain launch", hipGetLastError());
        // the members that open a group: all of them, or the first `pool` of the range
        const int64_t heads = pl.pool ? std::max<int64_t>(0, std::min<int64_t>(mc, pl.pool - mo)) : mc;
        if (heads > 0) {
            hipLaunchKernelGGL(k_rhat_head, blocks(heads * W), dim3(256), 0, st, (const double*)mu0, cen, NW, (int)W, mo, heads);
            RH_HIP("head launch", hipGetLastError());
        }
        hipLaunchKernelGGL(k_rhat_walkers, dim3((unsigned)runs, (unsigned)mc), dim3((unsigned)std::min<int64_t>(256, (W + 63) / 64 * 64)), 0, st,
                           (const double*)mu0, (const double*)q, (const double*)var, (const double*)cen, wpart, pl.N, (int)W, run, mo, pl.pool);
        RH_HIP("walkers launch", hipGetLastError());
        hipLaunchKernelGGL(k_rhat_member, dim3((unsigned)((mc * 3 * W + 15) / 16)), dim3(256), 0, st, (const double*)wpart, mem, runs, (int)W, mo, mc * 3 * W);
        RH_HIP("member launch", hipGetLastError());
    }
    hipLaunchKernelGGL(k_rhat_group, blocks(groups * W), dim3(256), 0, st, (const double*)mem, within, between, M, groups, pl.N, (int)W, ldo, col0);
    RH_HIP("group launch", hipGetLastError());
    return 0;      // the stream orders the next plane's use of the scratch behind this one's
}

// 0; -1 / -2 with the reason in err
int rh_run(const Plan& pl, double* within_out, double* between_out, int64_t* nchains_out, int64_t* length_out, char* err, size_t errlen) {
    const int64_t M = pl.hi - pl.lo;
    if (pl.pool < 0 || (pl.pool > 0 && M % pl.pool != 0)) {
        snprintf(err, errlen, "pool = %lld: 0, or a divisor of the %lld members", (long long)pl.pool, (long long)M);
        return -1;
    }
    if (pl.nt < 4) {
        snprintf(err, errlen, "%lld selected rows; the split needs at least 4", (long long)pl.nt);
        return -1;
    }
    if (!within_out || !between_out) {
        snprintf(err, errlen, "within_out and between_out are needed");
        return -1;
    }
    if (pl.D > 65535) {
        snprintf(err, errlen, "at most 65535 columns; got %lld", (long long)pl.D);
        return -1;
    }
    const int64_t groups = pl.pool ? pl.pool : M;
    const int ldo = (int)(pl.D + (pl.log_prob ? 1 : 0));
    if (nchains_out) *nchains_out = 2 * pl.N * (M / groups);
    if (length_out) *length_out = pl.nt / 2;
    double *w, *b;
    RH_HIP("output allocation", pl.sc->get(RhatScratch::WITHIN, &w, (size_t)groups * ldo));
    RH_HIP("output allocation", pl.sc->get(RhatScratch::BETWEEN, &b, (size_t)groups * ldo));
    if (const int rc = rh_plane(pl, pl.x, pl.D, w, b, ldo, 0, err, errlen)) return rc;
    if (pl.log_prob)
        if (const int rc = rh_plane(pl, pl.lp, 1, w, b, ldo, (int)pl.D, err, errlen)) return rc;
    RH_HIP("copy", hipMemcpyAsync(within_out, w, (size_t)groups * ldo * 8, hipMemcpyDeviceToHost, pl.stream));
    RH_HIP("copy", hipMemcpyAsync(between_out, b, (size_t)groups * ldo * 8, hipMemcpyDeviceToHost, pl.stream));
    RH_HIP("synchronize", hipStreamSynchronize(pl.stream));
    return 0;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int emx_rhat_batch(emx_batch* b, int32_t member_lo, int32_t member_hi, int32_t pool, int64_t start, int64_t stop, int64_t stride,
                   int32_t log_prob, double* within_out, double* between_out, int64_t* nchains_out, int64_t* length_out) {
    EmxBatchView v;
    if (emx_internal_batch_view(b, &v)) return -1;
    char err[320], msg[384];
    auto fail = [&](int code) {
        snprintf(msg, sizeof msg, "emx_rhat_batch: %s", err);
        return emx_internal_batch_fail(b, code, msg);
    };
    if (!(0 <= member_lo && member_lo < member_hi && member_hi <= v.B)) {
        snprintf(err, sizeof err, "members [%d, %d) outside [0, %d) or empty", member_lo, member_hi, v.B);
        return fail(-1);
    }
    if (!v.chain || !v.chain_lp || v.stored <= 0) {
        snprintf(err, sizeof err, "no stored chain (emx_batch_chain_config + a stored run)");
        return fail(-1);
    }
    if (stride < 1 || start < 0 || stop > v.stored) {
        snprintf(err, sizeof err, "rows need 0 <= start, stop <= stored, stride >= 1");
        return fail(-1);
    }
    Plan pl;
    pl.x = v.chain;
    pl.lp = v.chain_lp;
    pl.cap = v.cap;
    pl.N = v.N;
    pl.D = v.D;
    pl.lo = member_lo;
    pl.hi = member_hi;
    pl.pool = pool;
    pl.start = start;
    pl.stride = stride;
    pl.nt = start < stop ? (stop - start + stride - 1) / stride : 0;
    pl.members_per_pass = v.rhat_members;
    pl.log_prob = log_prob != 0;
    pl.stream = v.stream;
    if (!*v.rhat) *v.rhat = new RhatScratch();
    pl.sc = *v.rhat;
    if (hipSetDevice(v.device) != hipSuccess) {
        snprintf(err, sizeof err, "hipSetDevice failed");
        return fail(-2);
    }
    const int rc = rh_run(pl, within_out, between_out, nchains_out, length_out, err, sizeof err);
    return rc ? fail(rc) : 0;
}

int emx_rhat(emx_ctx* c, int64_t start, int64_t stop, int64_t stride, int32_t log_prob, double* within_out, double* between_out,
             int64_t* nchains_out, int64_t* length_out) {
    if (const int rc = emx_internal_settle(c)) return rc;
    EmxChainView v;
    if (const int rc = emx_internal_chain_view(c, &v)) return rc;
    char err[320], msg[384];
    auto fail = [&](int code) {
        snprintf(msg, sizeof msg, "emx_rhat: %s", err);
        return emx_internal_fail(c, code, msg);
    };
    if (!v.chain || !v.chain_lp || v.stored <= 0) {
        snprintf(err, sizeof err, "no stored chain (emx_chain_config + stored steps)");
        return fail(-1);
    }
    if (stride < 1 || start < 0 || stop > v.stored) {
        snprintf(err, sizeof err, "rows need 0 <= start, stop <= stored, stride >= 1");
        return fail(-1);
    }
    Plan pl;
    pl.x = v.chain;
    pl.lp = v.chain_lp;
    pl.cap = v.cap;      // one member: never multiplied by a member index other than 0
    pl.N = v.N;
    pl.D = v.D;
    pl.lo = 0;
    pl.hi = 1;
    pl.pool = 0;
    pl.start = start;
    pl.stride = stride;
    pl.nt = start < stop ? (stop - start + stride - 1) / stride : 0;
    pl.members_per_pass = 0;
    pl.log_prob = log_prob != 0;
    pl.stream = v.stream;
    if (!*v.rhat) *v.rhat = new RhatScratch();
    pl.sc = *v.rhat;
    if (hipSetDevice(v.device) != hipSuccess) {
        snprintf(err, sizeof err, "hipSetDevice failed");
        return fail(-2);
    }
    const int rc = rh_run(pl, within_out, between_out, nchains_out, length_out, err, sizeof err);
    return rc ? fail(rc) : 0;
}

}  // extern "C"
#pragma GCC visibility pop
