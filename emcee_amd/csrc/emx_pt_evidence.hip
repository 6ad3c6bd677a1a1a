// libemx, emx_pt_evidence: the per-block sums behind PTSampler.get_evidence -- the stepping-stone evidence (Xie et al. 2011), the
// thermodynamic-integration evidence and the Monte-Carlo error of both -- reduced next to the stored log-likelihood plane.  Only
// O(objects rungs blocks) doubles cross to the host.
//
// Definition (emcee_amd.pt.stepping_stone_log_evidence is the same on a host array):
//   Selection   the one get_chain(discard, thin) makes: stored rows start + i stride, i = 0 ... nt - 1.
//   Blocks      K = nblocks, bl = nt / K (integer).  The LAST K bl selected rows are used (the remainder is dropped at the early,
//               burn-in end), cut into K consecutive blocks that are aligned in time across all rungs of an object.
//   Ladder      object g's ladder b[0] > ... > b[T-1] is the stored beta row of the first used step; it must be bit-equal on every
//               used step (ladder_changed[g] says whether it was not).
//   Pair j      (j = 0 ... T - 2) covers rungs j and j + 1.  d = fl(b[j] - b[j+1]).  The samples are the n = bl N values L of rung
//               j + 1, the hotter one, in block k;  a = fl(d L);  M[g,j,k] = max a;  S[g,j,k] = sum exp(a - M);  the block's
//               log-ratio is M + log(S / n).  L = -inf gives a = -inf and contributes 0; a block of nothing else has M = -inf and
//               S = 0 (log-ratio -inf, never NaN); any NaN sample makes the block's S NaN (M is the maximum of the others).
//   Merge       (host) M* = max_k M,  S* = sum_k S_k exp(M_k - M*) in block order,  log r[g,j] = M* + log(S* / (K n)): the forward
//               stepping-stone estimate of Z(b[j]) / Z(b[j+1]), whose weights are bounded by the hotter rung's own maximum.
//   Sums        A[g,t,k] = sum of L over block k of rung t;  mean_logl[g,t] = (the blocks' sums added in block order) / (K n).
//   Tail        b[T-1] mean_logl[g,T-1] when b[T-1] > 0 (thermodynamic integration's own extrapolation to beta = 0), else 0.
//   Results     logz_ss[g] = sum_j log r[g,j] + tail[g] (j ascending); block_logz_ss[g,k] the same from block k alone;
//               err_ss = std_k(block_logz_ss, ddof = 1) / sqrt(K); logz_ti, dlogz_ti, block_logz_ti and err_ti likewise from
//               thermodynamic_integration_log_evidence(b, means).
// The device produces A, M, S, the ladder and ladder_changed; everything from the merge on is the host's, in the order above.
//
// Layout: the plane is chain_L[(m cap + row) N + w], member m = g T + t; with stride 1 a block of a member is one run of bl N
// doubles.  A block's n samples, counted e = i N + w over its selected rows i, are cut into slices of PE_SLICE = 4 096 consecutive
// samples: the slice count ceil(n / 4096) is fixed by (bl, N) alone, so one object with a long chain still fills the chip.
//   k_pte_slice    one workgroup (4 waves) a (member, block, slice), which reads its samples from HBM once and keeps them in
//                  registers: thread h holds samples 2 (h + 256 i) and 2 (h + 256 i) + 1, i = 0 ... 7 -- one 16-byte load where the
//                  stride is 1 and the pair is 16-byte aligned, two 8-byte loads otherwise; the values and their order are the
//                  same either way.  The thread adds its L in that order and takes the maximum of its a; a butterfly over the
//                  wave's lanes (xor 32, 16, ... 1: every lane ends with the same bits) and the 4 waves in wave order through
//                  LDS give the slice's sum and its exact maximum M.  Then exp(a - M) of the held values is added in the same
//                  order: one exp a sample and no rescaling.  Rung 0 is never the hotter rung of a pair: its slices add L only.
//   k_pte_merge    one wave a (member, block): M = max of the slices' maxima; the lanes make the terms S_s exp(M_s - M) side by side
//                  (exp(0) = 1: a block of one slice keeps its bits) and one lane adds the slices' sums and the terms in slice
//                  order; for block 0 it also copies the member's beta of the first used row.
//   k_pte_ladder   the stored beta plane (plane 3 of emx_batch_chain_read) of the used rows against the first used row, bit for
//                  bit; a difference sets the object's flag (an integer atomic or).
// No floating-point atomics.  Every sum and every (M, S) merge runs in an order fixed by (nt, K, N, stride): no bit depends on the
// object range, on how many objects share a launch or on the launch shape.  Scratch stays on the batch handle between calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/emx.h"
#include "emx_internal.hpp"

namespace {

constexpr int PE_THREADS = 256, PE_PAIRS = 8;                  // pairs of samples a thread
constexpr int64_t PE_SLICE = 2 * PE_PAIRS * PE_THREADS;        // samples a slice
constexpr int64_t PE_LADDER_ROWS = 4096;                       // used rows a workgroup of k_pte_ladder

struct PSel {
    const double* L;         // (B, cap, N)
    const double* beta;      // (B, cap)
    int64_t cap, N, row0, stride, bl, n, S, m0;      // row0: the first used stored row; n = bl N; S slices a block; m0: first member
    int32_t T, K;
};

// the wave's lanes all end with the same sum / maximum
__device__ __forceinline__ double pe_wave_sum(double v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double pe_wave_max(double v) {
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// part (members of the launch, K, S, 3) = the slice's sum of L, maximum of a and sum of exp(a - maximum).
// blockIdx.x = k S + s, blockIdx.y = member - m0.  Six waves a SIMD asked for: left alone the compiler interleaves the 16 inlined exp and
// takes 136 registers, 3 waves a SIMD, which does not hide the loads; so bounded it takes 52, without scratch
__global__ __launch_bounds__(PE_THREADS) __attribute__((amdgpu_waves_per_eu(6))) void k_pte_slice(const PSel g, double* __restrict__ part) {
    __shared__ double red[3][PE_THREADS / 64];
    const int64_t k = blockIdx.x / g.S, s = blockIdx.x - k * g.S, ml = blockIdx.y, m = g.m0 + ml;
    const int t = (int)(m % g.T);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t e0 = s * PE_SLICE, left = g.n - e0;                       // samples of the block from this slice on: > 0
    const int64_t first = g.row0 + k * g.bl * g.stride;                     // the block's first stored row
    const double* base = g.L + (m * g.cap + first) * g.N;
    const bool run = g.stride == 1;
    const bool vec = run && ((((m * g.cap + first) * g.N) & 1) == 0);       // e0 is even: the pairs are 16-byte aligned
    const double ninf = -__builtin_inf();
    double d = 0.0;
    if (t > 0) {
        const int64_t at = g.row0;
        d = g.beta[(m - 1) * g.cap + at] - g.beta[m * g.cap + at];
    }
    double v[2 * PE_PAIRS];
    bool in[2 * PE_PAIRS];
#pragma unroll
    for (int i = 0; i < PE_PAIRS; ++i) {
        const int64_t q = 2 * ((int64_t)threadIdx.x + (int64_t)PE_THREADS * i);      // within the slice
        in[2 * i] = q < left;
        in[2 * i + 1] = q + 1 < left;
        v[2 * i] = v[2 * i + 1] = 0.0;
        if (vec && in[2 * i + 1]) {
            const double2 p = *reinterpret_cast<const double2*>(base + e0 + q);
            v[2 * i] = p.x;
            v[2 * i + 1] = p.y;
        } else if (run) {
            if (in[2 * i]) v[2 * i] = base[e0 + q];
            if (in[2 * i + 1]) v[2 * i + 1] = base[e0 + q + 1];
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (in[2 * i + h]) {
                    const int64_t e = e0 + q + h, r = e / g.N, w = e - r * g.N;
                    v[2 * i + h] = base[r * g.stride * g.N + w];
                }
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 2 * PE_PAIRS; ++i) sum += v[i];                     // a sample outside the block is 0 here
    sum = pe_wave_sum(sum);
    double mx = ninf;
    if (t > 0) {
#pragma unroll
        for (int i = 0; i < 2 * PE_PAIRS; ++i) {
            v[i] = in[i] ? d * v[i] : ninf;                                 // a; outside the block -inf: no weight
            mx = fmax(mx, v[i]);                                            // a NaN is passed over here and met in the sum below
        }
        mx = pe_wave_max(mx);
    }
    if (lane == 0) {
        red[0][wv] = sum;
        red[1][wv] = mx;
    }
    __syncthreads();
    const double M = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
    double se = 0.0;
    if (t > 0) {
#pragma unroll
        for (int i = 0; i < 2 * PE_PAIRS; ++i) se += v[i] == ninf ? 0.0 : exp(v[i] - M);
        se = pe_wave_sum(se);
        if (lane == 0) red[2][wv] = se;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* out = part + ((ml * g.K + k) * g.S + s) * 3;
        out[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        out[1] = M;
        out[2] = t > 0 ? ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3] : 0.0;
    }
}

// one wave a (member of the launch, block), blockIdx.x = ml K + k: sum_L (objects, T, K), amax / sexp (objects, T - 1, K), betas
// (objects, T), the object index counted from the call's first object (member mo of the call is the launch's first).  The lanes
// find the maximum (exact in any order) and make the slices' terms S_s exp(M_s - M) side by side, PE_MERGE slices at a time into
// LDS; lane 0 adds the sums and the terms from there in slice order
constexpr int PE_MERGE = 256;
__global__ __launch_bounds__(64) void k_pte_merge(const PSel g, const double* __restrict__ part, double* __restrict__ sum_L,
                                                  double* __restrict__ amax, double* __restrict__ sexp, double* __restrict__ betas, int64_t mo) {
    __shared__ double ta[PE_MERGE], ts[PE_MERGE];
    const int64_t i = blockIdx.x, ml = i / g.K, k = i - ml * g.K, mc = mo + ml, gl = mc / g.T, t = mc - gl * g.T;
    const int lane = threadIdx.x;
    const double* p = part + i * g.S * 3;
    const double ninf = -__builtin_inf();
    double M = ninf;
    for (int64_t s = lane; s < g.S; s += 64) M = fmax(M, p[3 * s + 1]);
    M = pe_wave_max(M);
    double A = 0.0, S = 0.0;
    for (int64_t s0 = 0; s0 < g.S; s0 += PE_MERGE) {
        const int cnt = (int)(g.S - s0 < PE_MERGE ? g.S - s0 : PE_MERGE);
        for (int q = lane; q < cnt; q += 64) {
            const double* e = p + 3 * (s0 + q);
            const double Ms = e[1], Ss = e[2];
            ta[q] = e[0];
            ts[q] = t == 0 ? 0.0 : Ms == ninf ? Ss : Ss * exp(Ms - M);      // a slice without weight holds 0, or NaN for a NaN sample
        }
        __syncthreads();
        if (lane == 0)
            for (int q = 0; q < cnt; ++q) {
                A += ta[q];
                S += ts[q];
            }
        __syncthreads();
    }
    if (lane != 0) return;
    sum_L[i + mo * g.K] = A;
    if (k == 0) betas[mc] = g.beta[(g.m0 + ml) * g.cap + g.row0];
    if (t > 0) {
        const int64_t o = (gl * (g.T - 1) + (t - 1)) * g.K + k;
        amax[o] = M;
        sexp[o] = S;
    }
}

// blockIdx.x = a run of PE_LADDER_ROWS used rows, blockIdx.y = member - m0; `used` rows from row0 on, every stride-th
__global__ __launch_bounds__(256) void k_pte_ladder(const PSel g, int64_t used, int32_t* __restrict__ changed, int64_t mo) {
    const int64_t ml = blockIdx.y, ra = (int64_t)blockIdx.x * PE_LADDER_ROWS, rb = ra + PE_LADDER_ROWS < used ? ra + PE_LADDER_ROWS : used;
    const double* p = g.beta + (g.m0 + ml) * g.cap + g.row0;
    const long long want = __double_as_longlong(p[0]);
    bool diff = false;
    for (int64_t r = ra + threadIdx.x; r < rb; r += 256) diff |= __double_as_longlong(p[r * g.stride]) != want;
    if (__ballot(diff) != 0ull && (threadIdx.x & 63) == 0) atomicOr(changed + (mo + ml) / g.T, 1);
}

}  // namespace

// ---- host -----------------------------------------------------------------------------------------------------------
// the scratch of a batch handle: two device buffers and a pinned host one that only grow, freed with the handle
struct PtEvidenceScratch {
    enum { PART, OUT, HOST, COUNT };
    void* p[COUNT] = {};
    size_t bytes[COUNT] = {};
    static void release(int which, void* q) { (void)(which == HOST ? hipHostFree(q) : hipFree(q)); }
    hipError_t get(int which, void** out, size_t need) {
        need = std::max<size_t>(need, 8);
        if (need > bytes[which]) {
            if (p[which]) release(which, p[which]);
            p[which] = nullptr;
            bytes[which] = 0;
            const hipError_t e = which == HOST ? hipHostMalloc(&p[which], need, hipHostMallocDefault) : hipMalloc(&p[which], need);
            if (e != hipSuccess) {
                p[which] = nullptr;
                return e;
            }
            bytes[which] = need;
        }
        *out = p[which];
        return hipSuccess;
    }
};

void emx_internal_pt_evidence_release(PtEvidenceScratch* s) {
    if (!s) return;
    for (int i = 0; i < PtEvidenceScratch::COUNT; ++i)
        if (s->p[i]) PtEvidenceScratch::release(i, s->p[i]);
    delete s;
}

namespace {

#define PE_HIP(what, expr)                                                                                             \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                        \
            (void)hipGetLastError();                                                                                   \
            snprintf(err, errlen, "%s: %s", what, hipGetErrorString(e_));                                              \
            return -2;                                                                                                 \
        }                                                                                                              \
    } while (0)

// the out buffer of a call: sum_L (nA), amax (nP), sexp (nP), betas (nB) doubles, then the objects' int32 flags: one copy to the host
struct PeLayout {
    size_t nA, nP, nB, objects;
    size_t doubles() const { return nA + 2 * nP + nB + (objects + 1) / 2; }
};

// members [mlo, mhi) of the handle; 0, or -2 with the reason in err
int pe_run(PSel g, PtEvidenceScratch& sc, int64_t mlo, int64_t mhi, int64_t used, double* sum_L, double* amax, double* sexp, double* betas,
           int32_t* changed, hipStream_t st, char* err, size_t errlen) {
    const int64_t members = mhi - mlo, T = g.T, K = g.K, objects = members / T;
    const int64_t per_pass = std::min<int64_t>(std::min<int64_t>(members, 65535), std::max<int64_t>(1, 0x7fffffffLL / K));      // grid.y; the merge's grid.x
    const PeLayout lay{(size_t)members * K, (size_t)objects * (T - 1) * K, (size_t)members, (size_t)objects};
    void *part, *out, *host;
    PE_HIP("slice sums allocation", sc.get(PtEvidenceScratch::PART, &part, (size_t)per_pass * K * g.S * 3 * 8));
    PE_HIP("output allocation", sc.get(PtEvidenceScratch::OUT, &out, lay.doubles() * 8));
    PE_HIP("staging allocation", sc.get(PtEvidenceScratch::HOST, &host, lay.doubles() * 8));
    double *dA = (double*)out, *dM = dA + lay.nA, *dS = dM + lay.nP, *dB = dS + lay.nP;
    int32_t* dC = (int32_t*)(dB + lay.nB);
    PE_HIP("flag reset", hipMemsetAsync(dC, 0, (size_t)objects * 4, st));
    for (int64_t m0 = mlo; m0 < mhi; m0 += per_pass) {
        const int64_t mc = std::min<int64_t>(per_pass, mhi - m0), mo = m0 - mlo;
        g.m0 = m0;
        hipLaunchKernelGGL(k_pte_slice, dim3((unsigned)(K * g.S), (unsigned)mc), dim3(PE_THREADS), 0, st, g, (double*)part);
        PE_HIP("slice launch", hipGetLastError());
        hipLaunchKernelGGL(k_pte_merge, dim3((unsigned)(mc * K)), dim3(64), 0, st, g, (const double*)part, dA, dM, dS, dB, mo);
        PE_HIP("merge launch", hipGetLastError());
        hipLaunchKernelGGL(k_pte_ladder, dim3((unsigned)((used + PE_LADDER_ROWS - 1) / PE_LADDER_ROWS), (unsigned)mc), dim3(256), 0, st, g, used, dC,
                           mo);
        PE_HIP("ladder launch", hipGetLastError());
    }
    PE_HIP("copy", hipMemcpyAsync(host, out, lay.doubles() * 8, hipMemcpyDeviceToHost, st));
    PE_HIP("synchronize", hipStreamSynchronize(st));
    const double* h = (const double*)host;
    std::memcpy(sum_L, h, lay.nA * 8);
    if (lay.nP) std::memcpy(amax, h + lay.nA, lay.nP * 8);
    if (lay.nP) std::memcpy(sexp, h + lay.nA + lay.nP, lay.nP * 8);
    std::memcpy(betas, h + lay.nA + 2 * lay.nP, lay.nB * 8);
    std::memcpy(changed, h + lay.nA + 2 * lay.nP + lay.nB, (size_t)objects * 4);
    return 0;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int emx_pt_evidence(emx_batch* b, int64_t g_lo, int64_t g_hi, int64_t start, int64_t stop, int64_t stride, int32_t nblocks, double* sum_L,
                    double* amax, double* sexp, double* betas, int32_t* ladder_changed, int64_t* block_rows) {
    EmxBatchView v;
    if (emx_internal_batch_view(b, &v)) return -1;
    char err[320], msg[384];
    auto fail = [&](int code) {
        snprintf(msg, sizeof msg, "emx_pt_evidence: %s", err);
        return emx_internal_batch_fail(b, code, msg);
    };
    if (!(v.pt_T > 0 && v.chain_L && v.chain_beta)) {
        snprintf(err, sizeof err, "no tempered chain");
        return fail(-1);
    }
    const int64_t T = v.pt_T, objects = v.B / T;
    if (!(0 <= g_lo && g_lo < g_hi && g_hi <= objects)) {
        snprintf(err, sizeof err, "objects [%lld, %lld) outside [0, %lld) or empty", (long long)g_lo, (long long)g_hi, (long long)objects);
        return fail(-1);
    }
    if (!(stride >= 1 && 0 <= start && start < stop && stop <= v.stored)) {
        snprintf(err, sizeof err, "rows [%lld, %lld) outside the %lld stored", (long long)start, (long long)stop, (long long)v.stored);
        return fail(-1);
    }
    const int64_t nt = (stop - start + stride - 1) / stride;
    if (!(1 <= nblocks && nblocks <= nt)) {
        snprintf(err, sizeof err, "nblocks = %d: between 1 and the %lld selected rows", nblocks, (long long)nt);
        return fail(-1);
    }
    if (!sum_L || !betas || !ladder_changed || (T > 1 && (!amax || !sexp))) {
        snprintf(err, sizeof err, "sum_L, amax, sexp, betas and ladder_changed are needed");
        return fail(-1);
    }
    PSel g;
    g.L = v.chain_L;
    g.beta = v.chain_beta;
    g.cap = v.cap;
    g.N = v.N;
    g.stride = stride;
    g.K = nblocks;
    g.T = (int32_t)T;
    g.bl = nt / nblocks;
    g.row0 = start + (nt - g.bl * nblocks) * stride;
    g.n = g.bl * g.N;
    g.S = (g.n + PE_SLICE - 1) / PE_SLICE;
    g.m0 = 0;
    if (g.S * nblocks > 0x7fffffffLL) {
        snprintf(err, sizeof err, "%lld slices a member: more than one launch holds", (long long)(g.S * nblocks));
        return fail(-1);
    }
    if (block_rows) *block_rows = g.bl;
    if (hipSetDevice(v.device) != hipSuccess) {
        snprintf(err, sizeof err, "hipSetDevice failed");
        return fail(-2);
    }
    if (!*v.pt_evidence) *v.pt_evidence = new PtEvidenceScratch();
    const int rc = pe_run(g, **v.pt_evidence, g_lo * T, g_hi * T, g.bl * nblocks, sum_L, amax, sexp, betas, ladder_changed, v.stream, err,
                          sizeof err);
    return rc ? fail(rc) : 0;
}

}  // extern "C"
#pragma GCC visibility pop
