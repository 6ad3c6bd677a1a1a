// libemx, emx_autocorr_batch: the integrated autocorrelation time of every member of an emx_batch, computed next to the
// member-major chain (B, cap, N, D) -- what emx_autocorr (emx_aux.hip) computes for one ensemble, the reference's
// integrated_time (autocorr.py:20-123) on backend.get_value("chain", discard, thin) (backend.py:42-58), for members
// [member_lo, member_hi) at once.  Only tau and the Sokal window of every (member, parameter) come back to the host.
//
// Series s = (member, walker, dim): within a member the N D series of one stored step are contiguous, members are cap N D
// doubles apart.  Members go in groups (their mean ACF within ~1 GB); per group
//   k_bacf_mean        mean of every series of the group over the selected samples, in two parts: m1 = mean(x), then
//                      m2 = mean(x - m1) in the same order -- m1's rounding error is relative to |m1| and would enter the
//                      lagged products linearly; what is left after m2 is relative to the spread
// then per chunk of consecutive series (a chunk may begin and end inside a member):
//   k_bacf_gather      buf[s][t] = (x - m1) - m2 for t < nt, 0 up to L (a tile transposed through LDS)
//   hipFFT D2Z         spectrum
//   k_bacf_power       |z|^2
//   hipFFT Z2D         autocovariance of every series
//   k_bacf_accumulate  macf[member][dim][t] += acf_w[t] / acf_w[0] over the chunk's walkers, in walker order
// then per group of members k_bacf_window: Sokal's window, one lane per (member, dim), in emx_autocorr's order.
// The hipFFT plans (keyed by L and the chunk's batch) and the scratch live on the handle, grown and never shrunk: a
// convergence loop that calls this on a growing chain creates plans only when L crosses a power of two.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/emx.h"
#include "emx_internal.hpp"

struct BatchAcf {
    struct Plan {
        int64_t L, batch;
        void *fwd, *inv;
    };
    std::vector<Plan> plans;                 // every one of length L (older lengths are destroyed when L changes)
    double *buf = nullptr, *mean = nullptr, *macf = nullptr, *tau = nullptr;
    double2* spec = nullptr;
    int32_t* win = nullptr;
    size_t buf_n = 0, spec_n = 0, mean_n = 0, macf_n = 0, tau_n = 0, win_n = 0;     // elements allocated
};

void emx_internal_batch_acf_release(BatchAcf* a) {
    if (!a) return;
    for (const BatchAcf::Plan& p : a->plans) {
        if (p.fwd) g_fft.Destroy(p.fwd);
        if (p.inv) g_fft.Destroy(p.inv);
    }
    for (void* p : {(void*)a->buf, (void*)a->spec, (void*)a->mean, (void*)a->macf, (void*)a->tau, (void*)a->win})
        if (p) hipFree(p);
    delete a;
}

namespace {

// ---- kernels --------------------------------------------------------------------------------------------------------
// series s of a launch is global series g = g0 + s: member m = g / ND, j = g % ND (walker j / D, dim j % D); its sample t
// is stored row t0 + t thin of the member, chain[(m cap + t0 + t thin) ND + j].
//
// mean[s]: lane = series (64 consecutive series a block, reading consecutive doubles but across a member boundary), the 4 waves
// sum consecutive quarters of the samples, combined in wave order.  The order depends on nt alone: no bit depends on the
// grouping or the chunking.  sub: nothing, or the first part of the mean, subtracted from every sample before it is added.
__global__ __launch_bounds__(256) void k_bacf_mean(const double* __restrict__ chain, const double* __restrict__ sub, double* __restrict__ mean,
                                                   int64_t g0, int64_t nser, int64_t ND, int64_t cap, int64_t t0, int64_t thin, int64_t nt) {
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * 64 + lane;
    const int64_t q = (nt + 3) / 4, ta = wv * q, tb = ta + q < nt ? ta + q : nt;
    double acc = 0.0;
    if (s < nser) {
        const int64_t g = g0 + s, m = g / ND, j = g - m * ND;
        const double* p = chain + (m * cap + t0) * ND + j;
        const int64_t step = thin * ND;
        if (sub) {
            const double m1 = sub[s];
#pragma unroll 8
            for (int64_t t = ta; t < tb; ++t) acc += p[t * step] - m1;
        } else {
#pragma unroll 8
            for (int64_t t = ta; t < tb; ++t) acc += p[t * step];
        }
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && s < nser) mean[s] = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) / (double)nt;
}

// buf[s][t] = (x[t][s] - mean[s]) - mean2[s] for t < nt, 0 up to L: a 64 x 64 tile (64 series x 64 samples) goes through LDS so that the
// chain reads (along s) and the buffer writes (along t) are both coalesced.  grid.y strides over L's tiles.
__global__ __launch_bounds__(256) void k_bacf_gather(const double* __restrict__ chain, const double* __restrict__ mean,
                                                     const double* __restrict__ mean2, double* __restrict__ buf, int64_t g0, int64_t nser, int64_t ND, int64_t cap,
                                                     int64_t t0, int64_t thin, int64_t nt, int64_t L) {
    __shared__ double tile[64][65];
    const int64_t sb = (int64_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;          // 64 x 4
    // the series this thread reads (fixed over the tiles): a tile may straddle a member boundary
    const int64_t sr = sb + tx;
    const bool live = sr < nser;
    const double* src = nullptr;
    double mu = 0.0, mu2 = 0.0;
    if (live) {
        const int64_t g = g0 + sr, m = g / ND, j = g - m * ND;
        src = chain + (m * cap + t0) * ND + j;
        mu = mean[sr];
        mu2 = mean2[sr];
    }
    const int64_t step = thin * ND;
    for (int64_t tb = (int64_t)blockIdx.y * 64; tb < L; tb += (int64_t)gridDim.y * 64) {
        for (int r = ty; r < 64; r += 4) {                           // r: sample inside the tile, tx: series
            const int64_t t = tb + r;
            tile[r][tx] = (live && t < nt) ? (src[t * step] - mu) - mu2 : 0.0;
        }
        __syncthreads();
        for (int r = ty; r < 64; r += 4) {                           // r: series inside the tile, tx: sample
            const int64_t s = sb + r, t = tb + tx;
            if (s < nser && t < L) buf[s * L + t] = tile[tx][r];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_bacf_power(double2* __restrict__ f, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double2 z = f[i];
    f[i] = double2{z.x * z.x + z.y * z.y, 0.0};
}

// macf[m - mg][d][t] = running value + sum over the chunk's walkers w of member m (in walker order) of acf_w,d[t] / acf_w,d[0]
// (autocorr.py:33-34, :93-96).  Walkers of (m, d) in the chunk: those with g0 <= m ND + w D + d < g1.  The running value is
// loaded and the walkers added one by one, so the sum does not depend on where chunks begin or end.  grid (t blocks, D, members
// the chunk touches from m_first).
__global__ __launch_bounds__(256) void k_bacf_accumulate(const double* __restrict__ buf, double* __restrict__ macf, int64_t g0, int64_t g1,
                                                         int64_t m_first, int64_t mg, int64_t N, int32_t D, int64_t nt, int64_t L) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int d = blockIdx.y;
    const int64_t m = m_first + blockIdx.z;
    if (t >= nt) return;
    const int64_t base = m * N * D + d;                              // global series of walker 0
    auto first_at = [&](int64_t g) -> int64_t {                      // smallest w >= 0 with base + w D >= g, at most N
        if (g <= base) return 0;
        const int64_t w = (g - base + D - 1) / D;
        return w < N ? w : N;
    };
    const int64_t w_lo = first_at(g0), w_hi = first_at(g1);
    if (w_lo >= w_hi) return;
    double* out = macf + ((m - mg) * D + d) * nt + t;
    double acc = *out;
    for (int64_t w = w_lo; w < w_hi; ++w) {
        const double* row = buf + (base + w * D - g0) * L;
        acc += row[t] / row[0];
    }
    *out = acc;
}

// Sokal window (autocorr.py:36-46, :98-101) of `nrow` (member, dim) rows of macf, one lane a row, in emx_autocorr's arithmetic:
// tau(m) = 2 cumsum(macf / N) - 1, below(m) = m < c tau(m); the window is the first lag not below.  auto_window's degenerate cases:
// no lag below -> nt - 1 (a constant series: NaN), every lag below -> 0.  The loop ends once both a lag not below and a lag
// below have been seen (the answer is then the first lag not below).
__global__ __launch_bounds__(256) void k_bacf_window(const double* __restrict__ macf, double* __restrict__ tau, int32_t* __restrict__ win,
                                                     int64_t nrow, int64_t N, int64_t nt, double c) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrow) return;
    const double* f = macf + i * nt;
    double cs = 0.0, tau0 = 0.0, tau_first = 0.0, tau_m = 0.0;
    int64_t first = -1;
    bool any_below = false;
    for (int64_t m = 0; m < nt; ++m) {
        cs += f[m] / (double)N;
        tau_m = 2.0 * cs - 1.0;
        if (m == 0) tau0 = tau_m;
        const bool below = (double)m < c * tau_m;
        any_below |= below;
        if (!below && first < 0) {
            first = m;
            tau_first = tau_m;
        }
        if (first >= 0 && any_below) break;
    }
    if (!any_below) {                // the loop ran to the end: tau_m is tau(nt - 1)
        first = nt - 1;
        tau_first = tau_m;
    } else if (first < 0) {          // every lag below
        first = 0;
        tau_first = tau0;
    }
    tau[i] = tau_first;
    win[i] = (int32_t)first;
}

// ---- host -----------------------------------------------------------------------------------------------------------
int bfail(emx_batch* b, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int bfail(emx_batch* b, int code, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return emx_internal_batch_fail(b, code, buf);
}

template <typename T>
int grow(emx_batch* b, T*& p, size_t& cap, size_t n, const char* what) {
    if (n <= cap) return 0;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    if (e != hipSuccess) return bfail(b, -2, "emx_autocorr_batch: %s allocation (%zu bytes): %s", what, n * sizeof(T), hipGetErrorString(e));
    cap = n;
    return 0;
}

// the forward / inverse plans of length L and batch `batch`: from the handle's cache, or created (plans of another length are
// destroyed first: the chain grew past a power of two)
int get_plan(emx_batch* b, BatchAcf* a, hipStream_t stream, int64_t L, int64_t batch, BatchAcf::Plan* out) {
    for (const BatchAcf::Plan& p : a->plans)
        if (p.L == L && p.batch == batch) {
            *out = p;
            return 0;
        }
    if (!a->plans.empty() && a->plans[0].L != L) {
        for (const BatchAcf::Plan& p : a->plans) {
            g_fft.Destroy(p.fwd);
            g_fft.Destroy(p.inv);
        }
        a->plans.clear();
    }
    BatchAcf::Plan p{L, batch, nullptr, nullptr};
    int len = (int)L;
    const int LC = (int)(L / 2 + 1);
    int e = g_fft.PlanMany(&p.fwd, 1, &len, nullptr, 1, (int)L, nullptr, 1, LC, FFT_D2Z, (int)batch);
    if (!e) e = g_fft.PlanMany(&p.inv, 1, &len, nullptr, 1, LC, nullptr, 1, (int)L, FFT_Z2D, (int)batch);
    if (!e) e = g_fft.SetStream(p.fwd, stream);
    if (!e) e = g_fft.SetStream(p.inv, stream);
    if (e) {
        if (p.fwd) g_fft.Destroy(p.fwd);
        if (p.inv) g_fft.Destroy(p.inv);
        return bfail(b, -6, "emx_autocorr_batch: hipFFT plan creation failed (code %d, length %lld, batch %lld)", e, (long long)L,
                     (long long)batch);
    }
    a->plans.push_back(p);
    *out = p;
    return 0;
}

#define ACF_HIP(what, expr)                                                                                             \
    do {                                                                                                                \
        const hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) return bfail(b, -2, "emx_autocorr_batch: %s: %s", what, hipGetErrorString(e_));           \
    } while (0)

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int emx_autocorr_batch(emx_batch* b, int32_t member_lo, int32_t member_hi, int64_t discard, int64_t thin, double cwin, double* tau_out,
                       int32_t* window_out, int64_t* nsamples_out) {
    EmxBatchView v;
    if (emx_internal_batch_view(b, &v)) return -1;
    if (!(0 <= member_lo && member_lo < member_hi && member_hi <= v.B))
        return bfail(b, -1, "emx_autocorr_batch: members [%d, %d) outside [0, %d) or empty", member_lo, member_hi, v.B);
    if (thin < 1 || discard < 0) return bfail(b, -1, "emx_autocorr_batch: thin >= 1 and discard >= 0");
    if (!tau_out) return bfail(b, -1, "emx_autocorr_batch: no output buffer");
    if (!v.chain || v.stored <= 0) return bfail(b, -1, "emx_autocorr_batch: no stored chain (emx_batch_chain_config + a stored run)");
    // Backend.get_value slice (backend.py:56): rows discard + thin - 1, + thin, ... < stored
    const int64_t t0 = discard + thin - 1;
    const int64_t nt = t0 < v.stored ? (v.stored - t0 + thin - 1) / thin : 0;
    if (nsamples_out) *nsamples_out = nt;
    if (nt < 1) return bfail(b, -1, "emx_autocorr_batch: the selection is empty");
    int64_t n = 1;
    while (n < nt) n <<= 1;                              // autocorr.py:13-17 next_pow_two
    const int64_t L = 2 * n, LC = n + 1;
    if (L > (1ll << 30)) return bfail(b, -1, "emx_autocorr_batch: %lld samples exceed the FFT length limit 2^30", (long long)nt);
    std::string err;
    if (fft_load(nullptr, err)) return bfail(b, -5, "emx_autocorr_batch: %s", err.c_str());
    ACF_HIP("hipSetDevice", hipSetDevice(v.device));
    if (!*v.acf) *v.acf = new BatchAcf();
    BatchAcf* a = *v.acf;

    const int64_t N = v.N, D = v.D, ND = N * D, M = member_hi - member_lo;
    // members a group: their macf (members, D, nt) and means (members, N D) within ~1 GB, at least one member; sized by n >= nt
    // so that the grouping (and with it every chunk's batch) stays put while the chain grows inside one power of two
    const int64_t gm = std::max<int64_t>(1, std::min<int64_t>(M, (1ll << 30) / (D * n * 8 + ND * 8)));
    // series a chunk: real buffer + spectrum within ~3 GB; hipFFT's int batch; <= 65 535 members touched (grid.z)
    const int64_t per_series = L * 8 + LC * 16;
    int64_t sc = std::max<int64_t>(1, std::min<int64_t>(gm * ND, (3ll << 30) / per_series));
    sc = std::min<int64_t>(sc, std::min<int64_t>(1ll << 30, 65534 * ND));
    if (v.acf_series > 0) sc = std::min<int64_t>(sc, v.acf_series);
    if (int rc = grow(b, a->buf, a->buf_n, (size_t)(sc * L), "buffer")) return rc;
    if (int rc = grow(b, a->spec, a->spec_n, (size_t)(sc * LC), "spectrum")) return rc;
    if (int rc = grow(b, a->mean, a->mean_n, (size_t)(2 * gm * ND), "mean")) return rc;
    if (int rc = grow(b, a->macf, a->macf_n, (size_t)(gm * D * nt), "mean-ACF")) return rc;
    if (int rc = grow(b, a->tau, a->tau_n, (size_t)(M * D), "tau")) return rc;
    if (int rc = grow(b, a->win, a->win_n, (size_t)(M * D), "window")) return rc;

    for (int64_t mg = member_lo; mg < member_hi; mg += gm) {
        const int64_t mcount = std::min<int64_t>(gm, member_hi - mg);
        ACF_HIP("memset", hipMemsetAsync(a->macf, 0, (size_t)(mcount * D * nt) * 8, v.stream));
        const int64_t gbeg = mg * ND, gend = (mg + mcount) * ND;
        double* mean2 = a->mean + gm * ND;      // the second part of the mean
        hipLaunchKernelGGL(k_bacf_mean, dim3((unsigned)((gend - gbeg + 63) / 64)), dim3(256), 0, v.stream, v.chain, (const double*)nullptr, a->mean,
                           gbeg, gend - gbeg, ND, v.cap, t0, thin, nt);
        hipLaunchKernelGGL(k_bacf_mean, dim3((unsigned)((gend - gbeg + 63) / 64)), dim3(256), 0, v.stream, v.chain, (const double*)a->mean, mean2,
                           gbeg, gend - gbeg, ND, v.cap, t0, thin, nt);
        ACF_HIP("mean launch", hipGetLastError());
        for (int64_t g0 = gbeg; g0 < gend; g0 += sc) {
            const int64_t nser = std::min<int64_t>(sc, gend - g0), g1 = g0 + nser;
            BatchAcf::Plan plan;
            if (int rc = get_plan(b, a, v.stream, L, nser, &plan)) return rc;
            hipLaunchKernelGGL(k_bacf_gather, dim3((unsigned)((nser + 63) / 64), (unsigned)std::min<int64_t>(65535, (L + 63) / 64)), dim3(256), 0,
                               v.stream, v.chain, (const double*)(a->mean + (g0 - gbeg)), (const double*)(mean2 + (g0 - gbeg)), a->buf, g0, nser, ND, v.cap, t0, thin, nt, L);
            ACF_HIP("gather launch", hipGetLastError());
            if (g_fft.ExecD2Z(plan.fwd, a->buf, a->spec)) return bfail(b, -6, "emx_autocorr_batch: hipFFT D2Z execution failed");
            const int64_t ne = nser * LC;
            hipLaunchKernelGGL(k_bacf_power, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, v.stream, a->spec, ne);
            ACF_HIP("power launch", hipGetLastError());
            if (g_fft.ExecZ2D(plan.inv, a->spec, a->buf)) return bfail(b, -6, "emx_autocorr_batch: hipFFT Z2D execution failed");
            const int64_t m_first = g0 / ND, m_last = (g1 - 1) / ND;
            hipLaunchKernelGGL(k_bacf_accumulate, dim3((unsigned)((nt + 255) / 256), (unsigned)D, (unsigned)(m_last - m_first + 1)), dim3(256), 0,
                               v.stream, a->buf, a->macf, g0, g1, m_first, mg, N, (int32_t)D, nt, L);
            ACF_HIP("accumulate launch", hipGetLastError());
        }
        const int64_t nrow = mcount * D, off = (mg - member_lo) * D;
        hipLaunchKernelGGL(k_bacf_window, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, v.stream, a->macf, a->tau + off, a->win + off,
                           nrow, N, nt, cwin);
        ACF_HIP("window launch", hipGetLastError());
    }
    ACF_HIP("copy", hipMemcpyAsync(tau_out, a->tau, (size_t)(M * D) * 8, hipMemcpyDeviceToHost, v.stream));
    if (window_out) ACF_HIP("copy", hipMemcpyAsync(window_out, a->win, (size_t)(M * D) * 4, hipMemcpyDeviceToHost, v.stream));
    ACF_HIP("synchronize", hipStreamSynchronize(v.stream));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
