// Batches of independent small ensembles whose log-probability is the caller's batched function (emx_set_batch_target_callback,
// emcee_amd.targets.BatchCallable / BatchKernel).  A proposal step of the batch is S_max phases (S_max: the most splits of
// any move of the schedule); per phase the host enqueues ONE k_batch_cb launch for every member and ONE call of the caller's
// function on the (B, R, D) proposal block, so the library's launches do not grow with B.
//
// k_batch_cb: workgroup b is member b, and a member is never split across workgroups.  It
//   1. commits the pending phase: the caller's log-probs of the block it was handed, the decision of small_update
//      (factor + lp_new - lp_old > logu, a non-finite proposal rejected), the accepted rows, flags, counts and, on a stored
//      step, the member's chain rows of the walkers of that split (each walker is updated by exactly one split of a step);
//   2. waits for its own stores (every wave's vmcnt(0)) and meets the workgroup barrier -- the proposals below read rows the
//      commit has just written, on the same CU: workgroup scope is all this hand-off needs;
//   3. proposes the next phase's split with k_small_run's device functions (small_plan_entry / native_gauss_slot,
//      small_propose) on the member's seed and step, or writes padding rows: copies of the member's current rows, valid
//      input for any likelihood, whose results are never read.
// Member b's bits are therefore those of the single-ensemble three-pass callback path (propose -> callback -> commit) with the
// same seed: the same plans, the same proposal arithmetic in the same row layout, the same decision.
#include <hip/hip_runtime.h>

#include "emx_batch_cb.hpp"
#include "emx_pt.hpp"

namespace emx {

namespace {

struct CbMember {          // what small_propose needs of a member
    uint32_t* st;
    __device__ __forceinline__ uint32_t* status() const { return st; }
};

// the box prior of row q (D values): 0 inside [lo, hi] (bounds included), -inf outside; the row's G lanes share the answer
template <int G>
__device__ __forceinline__ double box_prior(const double* q, const double* lo, const double* hi, int D, int gl) {
    int out = 0;
    for (int d = gl; d < D; d += G) {
        const double x = q[d];
        out |= (x >= lo[d] && x <= hi[d]) ? 0 : 1;
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) out |= __shfl_xor(out, m);
    return out ? -__builtin_inf() : 0.0;
}

// TEMPERED: the commit of parallel tempering (BatchCbArgs' tempering fields); the untempered instantiation is the kernel as it
// was, bit for bit and instruction for instruction.  BLOBS: the commit carries the caller's blobs with the row; with TEMPERED the
// tempered decision stands as it is and the blob commit comes behind it (a row outside the prior has NaN blobs, as its L is -inf)
template <int G, int V, int CH, bool TEMPERED, bool BLOBS = false>
__global__ __launch_bounds__(CB_MAX_THREADS) void k_batch_cb(const BatchCbArgs A) {
    constexpr int WPW = 64 / G;
    const int N = A.N, D = A.D, R = A.R, T = blockDim.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, nwave = T >> 6, sub = lane / G, gl = lane % G;
    const size_t b = blockIdx.x;
    double* X = A.X + b * (size_t)N * D;
    double* lp = A.lp + b * (size_t)N;
    uint8_t* acc = A.acc + b * (size_t)N;
    uint32_t* acc_count = A.acc_count + b * (size_t)N;
    const CbMember M{A.status + b * SMALL_STATUS_WORDS};

    // ---- 1. commit the pending phase (red_blue.py:96-104) ----
    if (TEMPERED && A.commit) {
        // the decision on the tempered lp = pt_tempered(beta, L, P); L and P follow the accepted rows.  On a stored step the
        // accept counts always move; the rows are written here unless the step ends with a swap pass (which writes them then).
        const int n = A.nrows[b];
        const bool stored = A.chain_row >= 0;
        const bool rows = stored && A.rows_in_commit;
        const double beta = A.beta[b];
        double* Lm = A.L + b * (size_t)N;
        double* Pm = A.P + b * (size_t)N;
        double* cr = rows ? A.chain + ((size_t)b * A.cap + A.chain_row) * (size_t)N * D : nullptr;
        double* cl = rows ? A.chain_lp + ((size_t)b * A.cap + A.chain_row) * (size_t)N : nullptr;
        double* cL = rows ? A.chain_L + ((size_t)b * A.cap + A.chain_row) * (size_t)N : nullptr;
        if (rows && tid == 0) A.chain_beta[(size_t)b * A.cap + A.chain_row] = beta;      // the member's beta row
        for (int base = wv * WPW; base < n; base += nwave * WPW) {
            const int t = base + sub;
            if (t < n) {                                                   // group-uniform
                const size_t r = b * R + t;
                const int i = A.wi[r];
                double pq = 0.0;
                if (A.lpr) pq = A.lpr[r];
                else if (A.box_lo) pq = box_prior<G>(A.q + r * D, A.box_lo, A.box_hi, D, gl);
                const double lraw = A.lpq[r];
                const bool pinf = pq == -__builtin_inf();
                const double lq = pinf ? -__builtin_inf() : lraw;             // the likelihood of a row outside the prior is ignored
                const double lpn = pt_tempered(beta, lq, pq), lpo = lp[i];
                if (gl == 0 && ((!pinf && lraw != lraw) || lpn != lpn)) raise_status(M.status(), ST_NAN_LOGP);
                const double lnpdiff = A.fac[r] + lpn - lpo;                         // (small_update's accept rule, on the tempered lp)
                const bool accept = lnpdiff > A.logu[r];
                Row<G, V, CH> x;
                if (accept || rows) load_row<G, V, CH>(x, accept ? A.q + r * D : X + (size_t)i * D, D, gl);
                if (accept) store_row<G, V, CH>(x, X + (size_t)i * D, D, gl);
                if (rows) store_row_stream<G, V, CH>(x, cr + (size_t)i * D, D, gl);
                if constexpr (BLOBS) {                                               // the blobs follow the accepted row; the plane's row only
                    const int K = A.nblobs;                                          // where this commit writes the stored rows
                    double* bw = A.blobs + (b * (size_t)N + i) * K;
                    double* bc = rows ? A.chain_blobs + (((size_t)b * A.cap + A.chain_row) * (size_t)N + i) * K : nullptr;
                    for (int k = gl; k < K; k += G) {
                        const double v = accept ? (pinf ? __builtin_nan("") : A.bq[r * K + k]) : bw[k];
                        if (accept) bw[k] = v;
                        if (rows) bc[k] = v;
                    }
                }
                if (gl == 0) {
                    const double lo = Lm[i];
                    if (accept) {
                        lp[i] = lpn;
                        Lm[i] = lq;
                        Pm[i] = pq;
                    }
                    acc[i] = accept ? 1 : 0;
                    if (stored) acc_count[i] += accept ? 1u : 0u;
                    if (rows) {
                        cl[i] = accept ? lpn : lpo;
                        cL[i] = accept ? lq : lo;
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (A.commit) {
        const int n = A.nrows[b];
        const bool stored = A.chain_row >= 0;
        double* cr = stored ? A.chain + ((size_t)b * A.cap + A.chain_row) * (size_t)N * D : nullptr;
        double* cl = stored ? A.chain_lp + ((size_t)b * A.cap + A.chain_row) * (size_t)N : nullptr;
        for (int base = wv * WPW; base < n; base += nwave * WPW) {
            const int t = base + sub;
            if (t < n) {                                                   // group-uniform
                const size_t r = b * R + t;
                const int i = A.wi[r];
                const double lpn = A.lpq[r], lpo = lp[i];
                if (gl == 0 && lpn != lpn) raise_status(M.status(), ST_NAN_LOGP);      // ensemble.py:550-551
                const double lnpdiff = A.fac[r] + lpn - lpo;                         // red_blue.py:99 (small_update's accept rule)
                const bool accept = lnpdiff > A.logu[r];                             // red_blue.py:100
                Row<G, V, CH> x;
                if (accept || stored) load_row<G, V, CH>(x, accept ? A.q + r * D : X + (size_t)i * D, D, gl);
                if (accept) store_row<G, V, CH>(x, X + (size_t)i * D, D, gl);
                if (stored) store_row_stream<G, V, CH>(x, cr + (size_t)i * D, D, gl);
                if constexpr (BLOBS) {                                               // move.py:29-45: the blobs follow the accepted row
                    const int K = A.nblobs;
                    double* bw = A.blobs + (b * (size_t)N + i) * K;
                    double* bc = stored ? A.chain_blobs + (((size_t)b * A.cap + A.chain_row) * (size_t)N + i) * K : nullptr;
                    for (int k = gl; k < K; k += G) {
                        const double v = accept ? A.bq[r * K + k] : bw[k];
                        if (accept) bw[k] = v;
                        if (stored) bc[k] = v;
                    }
                }
                if (gl == 0) {
                    if (accept) lp[i] = lpn;
                    acc[i] = accept ? 1 : 0;
                    if (stored) {                                                    // backend.py:229
                        cl[i] = accept ? lpn : lpo;
                        acc_count[i] += accept ? 1u : 0u;
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // ---- 2. the member's rows are committed before any wave of its workgroup proposes from them ----
    __syncthreads();
    if (!A.propose) return;

    // ---- 3. propose phase A.phase of step A.step (k_small_run's plan entry and proposal) ----
    const unsigned long long seed = A.seeds[b];
    const int m = A.nmoves == 1 ? 0 : native_move_choice(seed, A.step, A.cdf, A.nmoves);       // workgroup-uniform
    const int kind = A.kind[m];
    const int S = kind == MOVE_GAUSS ? 1 : A.nsplits[m];
    int ns = 0, pos0 = 0;
    if (A.phase < S) {
        const SplitSizes sz = split_sizes(N, S);
        for (int k = 0; k < A.phase; ++k) pos0 += sz.of(k);
        ns = sz.of(A.phase);
    }
    if (tid == 0) A.nrows[b] = ns;
    NativeArgs na;
    na.seed = seed;
    na.step = A.step;
    na.pk = make_perm_key((uint64_t)N, na.seed, na.step);
    GaussGen gg;
    gg.gseed = seed;
    gg.gstep = A.step;
    gg.gfac = A.gfac ? A.gfac[b * A.gfac_stride] : 1.0;
    gg.gsigma = A.gsigma[m];
    gg.gscale = A.gscale[m];
    const double gam = A.gammas[m];
    for (int base = wv * WPW; base < R; base += nwave * WPW) {             // wave-uniform
        const int t = base + sub;
        const bool live = t < ns;
        double* qrow = A.q + (b * R + (t < R ? t : 0)) * (size_t)D;
        if (ns > 0) {                                                      // workgroup-uniform
            const int pos = pos0 + (live ? t : 0);
            int i = 0, j0 = 0, j1 = 0, j2 = 0;
            double z = 0.0, lu = 0.0, fc = 0.0;
            Row<G, V, CH> q;
            double factor = 0.0;
            bool badq = false;
            if (kind == MOVE_GAUSS) {                                      // (the move ladder, SMALL_ANY_MOVE in emx_kernels.hpp, on kind alone)
                double u;
                native_gauss_slot(na, D, A.gmode[m], A.gcol, pos, i, j0, j1, j2, z, u);
                lu = plan_log_uniform(u);
                small_propose<G, V, CH, MOVE_GAUSS>(M, X, live, i, j0, j1, j2, z, fc, gam, D, gl, sub, q, factor, badq, &gg);
            } else if (kind == MOVE_STRETCH) {
                small_plan_entry<MOVE_STRETCH>(na, N, D, S, pos, A.a[m], A.sigma[m], A.g0[m], i, j0, j1, j2, z, lu, fc);
                small_propose<G, V, CH, MOVE_STRETCH>(M, X, live, i, j0, j1, j2, z, fc, gam, D, gl, sub, q, factor, badq);
            } else if (kind == MOVE_DE) {
                small_plan_entry<MOVE_DE>(na, N, D, S, pos, A.a[m], A.sigma[m], A.g0[m], i, j0, j1, j2, z, lu, fc);
                small_propose<G, V, CH, MOVE_DE>(M, X, live, i, j0, j1, j2, z, fc, gam, D, gl, sub, q, factor, badq);
            } else {
                small_plan_entry<MOVE_SNOOKER>(na, N, D, S, pos, A.a[m], A.sigma[m], A.g0[m], i, j0, j1, j2, z, lu, fc);
                small_propose<G, V, CH, MOVE_SNOOKER>(M, X, live, i, j0, j1, j2, z, fc, gam, D, gl, sub, q, factor, badq);
            }
            if (live) {
                store_row<G, V, CH>(q, qrow, D, gl);
                if (gl == 0) {
                    const size_t r = b * R + t;
                    A.fac[r] = badq ? -__builtin_inf() : factor;
                    A.logu[r] = lu;
                    A.wi[r] = i;
                }
                continue;
            }
        }
        if (t < R) {                                                       // padding: the member's own row t (R <= N)
            Row<G, V, CH> x;
            load_row<G, V, CH>(x, X + (size_t)t * D, D, gl);
            store_row<G, V, CH>(x, qrow, D, gl);
        }
    }
}

__global__ __launch_bounds__(64) void k_batch_lp_check(const double* lp, uint32_t* status, int N) {
    const size_t b = blockIdx.x;
    bool nan = false;
    for (int e = threadIdx.x; e < N; e += 64) nan |= lp[b * N + e] != lp[b * N + e];
    if (__ballot(nan) != 0ull && threadIdx.x == 0) raise_status(status + b * SMALL_STATUS_WORDS, ST_NAN_LOGP);
}

template <int G, int V, int CH>
hipError_t launch_cb(int grid, int threads, hipStream_t st, const BatchCbArgs& a) {
    auto kern = a.beta ? (a.nblobs > 0 ? k_batch_cb<G, V, CH, true, true> : k_batch_cb<G, V, CH, true>)
                       : a.nblobs > 0 ? k_batch_cb<G, V, CH, false, true> : k_batch_cb<G, V, CH, false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t batch_cb_dispatch(int G, int V, int CH, int grid, int threads, hipStream_t st, const BatchCbArgs& a) {
#define EMX_CASE(g, v, ch) \
    if (G == g && V == v && CH == ch) return launch_cb<g, v, ch>(grid, threads, st, a);
    EMX_CASE(4, 1, 1) EMX_CASE(8, 1, 1) EMX_CASE(8, 1, 2) EMX_CASE(8, 1, 4) EMX_CASE(16, 1, 4) EMX_CASE(32, 1, 4) EMX_CASE(64, 1, 4)
    EMX_CASE(4, 2, 1) EMX_CASE(8, 2, 1) EMX_CASE(8, 2, 2) EMX_CASE(8, 2, 4) EMX_CASE(16, 2, 4) EMX_CASE(32, 2, 4)
#undef EMX_CASE
    return hipErrorInvalidValue;
}

hipError_t batch_lp_check(const double* lp, uint32_t* status, int32_t B, int32_t N, hipStream_t st) {
    hipLaunchKernelGGL(k_batch_lp_check, dim3(B), dim3(64), 0, st, lp, status, N);
    return hipGetLastError();
}

}  // namespace emx
