// Parallel tempering on a batch handle (include/emx.h: emx_pt_*; emcee_amd.PTSampler).  Rung t of group g is member g T + t of the
// batch, sampling pt_tempered(beta_t, L, P) with k_batch_cb's tempered commit; this file holds what is new:
//
// k_pt_swap: one workgroup a group.  The pairs run in turn from the hottest, i = T - 1 ... 1 (ptemcee's order); inside a pair the
//   lanes run over the walkers k of rung i, each against walker pi_i(k) of rung i - 1 (pi_i a bijection: no two lanes touch the
//   same row).  Accepted when (beta_{i-1} - beta_i) (L_i[k] - L_{i-1}[pi_i(k)]) > log u_{i,k} (IEEE: NaN is rejected); then x, L
//   and P change places and lp is recomputed at both destinations.  Each pair ends by waiting for its stores and meeting the
//   workgroup barrier (k_batch_cb's hand-off from commit to propose), so that pair i - 1 sees what pair i left.  On a stored step
//   the pass then writes every rung's chain, lp, L and beta rows: the stored state is the state after the swap pass.
//   With adaptation on (PtSwapArgs::adapt), the pair loop also keeps each pair's accepts in LDS; after it one lane computes the
//   group's new ladder (pt_adapt_ladder, rung order) and writes beta[1 ... T - 2], then, after vmcnt(0) and the barrier, the
//   lanes recompute lp of every walker of the moved rungs, and after a second wait and barrier the stored rows are written.
//   With adaptation off the pass is the loop above alone.
//   Blobs (PtSwapArgs::nblobs > 0): a blob belongs to the point, so the lane that exchanges x exchanges the K doubles of the two rows
//   too (the pair's vmcnt(0) and barrier cover those stores), and a stored step writes every rung's rows of the blob plane.  The
//   ladder update does not touch them.  nblobs == 0 launches the blob-free instantiation: the pass above.
// k_pt_init: the tempered initial state (box prior, -inf likelihood outside the prior, tempered lp, NaN check; NaN blobs where the
//   prior is -inf).
// k_pt_mean_loglike: one workgroup a member, the mean of its L chain rows over the walkers (thermodynamic integration's input).
// k_pt_relp: lp from L, P and each member's beta (emx_pt_set_ladder).
// emx_host_pt_swap_draws / emx_host_pt_adapt_ladder: the host twins of the swap draws and of the ladder update.
#include <hip/hip_runtime.h>

#include "../../include/emx.h"
#include "emx_kernels.hpp"
#include "emx_pt.hpp"

namespace emx {

namespace {

constexpr int PT_THREADS = 256;

// BLOBS: the handle's target has blobs (PtSwapArgs::nblobs > 0); the blob-free instantiation is the pass as it was, instruction for instruction
template <bool BLOBS>
__global__ __launch_bounds__(PT_THREADS) void k_pt_swap(const PtSwapArgs A) {
    __shared__ unsigned int nacc;
    __shared__ unsigned int pacc[PT_ADAPT_MAX_T];     // adaptation: each pair's accepts of this pass, pair i at i - 1
    __shared__ double lad[PT_ADAPT_MAX_T];            // adaptation: the group's new ladder
    const int T = A.T, N = A.N, D = A.D, tid = threadIdx.x, nt = blockDim.x;
    const size_t g = blockIdx.x, m0 = g * (size_t)T;
    if (A.swap) {
        const unsigned long long seed = A.seeds[m0];
        for (int i = T - 1; i >= 1; --i) {
            if (tid == 0) nacc = 0u;
            __syncthreads();
            const size_t hot = m0 + i, cold = hot - 1;
            const double bh = A.beta[hot], bc = A.beta[cold];
            const double dbeta = bc - bh;
            const PermKey pk = pt_perm_key((uint64_t)N, seed, A.step, i);
            unsigned int mine = 0u;
            for (int k = tid; k < N; k += nt) {
                const int j = (int)perm_fwd((uint32_t)k, pk);
                const double lu = plan_log_uniform(pt_swap_uniform(seed, A.step, i, (uint32_t)k, (uint32_t)N));
                const size_t rh = hot * N + k, rc = cold * N + j;
                const double Lh = A.L[rh], Lc = A.L[rc];
                const double diff = Lh - Lc;
                if (dbeta * diff > lu) {
                    const double Ph = A.P[rh], Pc = A.P[rc];
                    double* xh = A.X + rh * D;
                    double* xc = A.X + rc * D;
                    for (int d = 0; d < D; ++d) {
                        const double v = xh[d];
                        xh[d] = xc[d];
                        xc[d] = v;
                    }
                    if constexpr (BLOBS) {                         // a blob belongs to the point: it changes places with x
                        double* bh2 = A.blobs + rh * A.nblobs;
                        double* bc2 = A.blobs + rc * A.nblobs;
                        for (int q = 0; q < A.nblobs; ++q) {
                            const double v = bh2[q];
                            bh2[q] = bc2[q];
                            bc2[q] = v;
                        }
                    }
                    A.L[rh] = Lc;
                    A.P[rh] = Pc;
                    A.lp[rh] = pt_tempered(bh, Lc, Pc);
                    A.L[rc] = Lh;
                    A.P[rc] = Ph;
                    A.lp[rc] = pt_tempered(bc, Lh, Ph);
                    ++mine;
                }
            }
            if (mine) atomicAdd(&nacc, mine);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this pair's rows are stored before the next pair reads them
            __syncthreads();
            if (tid == 0) {
                const size_t c = g * (size_t)(T - 1) + (i - 1);
                A.attempts[c] += (unsigned long long)N;
                A.accepts[c] += (unsigned long long)nacc;
                if (A.adapt) pacc[i - 1] = nacc;
            }
        }
        if (A.adapt && T > 2) {
            // the ladder update in rung order in one lane; then lp of every walker of the moved rungs from the new betas
            if (tid == 0) {
                for (int t = 0; t < T; ++t) lad[t] = A.beta[m0 + t];
                pt_adapt_ladder(lad, pacc, T, (long long)N, A.lag, A.time, A.adapt_t, lad);
                for (int t = 1; t < T - 1; ++t) A.beta[m0 + t] = lad[t];
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            for (int e = tid; e < (T - 2) * N; e += nt) {
                const size_t r = (m0 + 1) * N + e;
                A.lp[r] = pt_tempered(lad[1 + e / N], A.L[r], A.P[r]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the new lp is stored before the rows below read it
            __syncthreads();
        }
    }
    if (A.chain_row < 0) return;
    for (int t = tid; t < T; t += nt) A.chain_beta[(m0 + t) * (size_t)A.cap + A.chain_row] = A.beta[m0 + t];
    // the stored step's rows of every rung of the group: coordinates, tempered lp, L
    for (int t = 0; t < T; ++t) {
        const size_t m = m0 + t;
        const size_t crow = (size_t)m * A.cap + A.chain_row;
        const double* x = A.X + m * (size_t)N * D;
        double* cx = A.chain + crow * (size_t)N * D;
        for (int e = tid; e < N * D; e += nt) cx[e] = x[e];
        for (int e = tid; e < N; e += nt) {
            A.chain_lp[crow * N + e] = A.lp[m * N + e];
            A.chain_L[crow * N + e] = A.L[m * N + e];
        }
        if constexpr (BLOBS) {
            const size_t NK = (size_t)N * A.nblobs;
            const double* bw = A.blobs + m * NK;
            double* cb = A.chain_blobs + crow * NK;
            for (size_t e = tid; e < NK; e += nt) cb[e] = bw[e];
        }
    }
}

__global__ __launch_bounds__(PT_THREADS) void k_pt_relp(double* lp, const double* L, const double* P, const double* beta, int N) {
    const size_t m = blockIdx.x;
    const double bm = beta[m];
    for (int w = threadIdx.x; w < N; w += blockDim.x) lp[m * N + w] = pt_tempered(bm, L[m * N + w], P[m * N + w]);
}

__global__ __launch_bounds__(64) void k_pt_init(const double* X, double* lp, double* L, double* P, const double* beta,
                                                const double* box_lo, const double* box_hi, uint32_t* status, int N, int D,
                                                double* blobs, int K) {
    const size_t b = blockIdx.x;
    bool nan = false;
    for (int w = threadIdx.x; w < N; w += 64) {
        const size_t r = b * N + w;
        double p = P[r];
        if (box_lo) {
            bool in = true;
            for (int d = 0; d < D; ++d) {
                const double x = X[r * D + d];
                in = in && x >= box_lo[d] && x <= box_hi[d];
            }
            p = in ? 0.0 : -__builtin_inf();
            P[r] = p;
        }
        const double lraw = L[r];
        const bool pinf = p == -__builtin_inf();
        const double l = pinf ? -__builtin_inf() : lraw;
        const double v = pt_tempered(beta[b], l, p);
        L[r] = l;
        lp[r] = v;
        if (pinf)                                              // the row's blobs are ignored like its L
            for (int q = 0; q < K; ++q) blobs[r * K + q] = __builtin_nan("");
        nan |= (!pinf && lraw != lraw) || v != v;
    }
    if (__ballot(nan) != 0ull && threadIdx.x == 0) raise_status(status + b * SMALL_STATUS_WORDS, ST_NAN_LOGP);
}

__global__ __launch_bounds__(PT_THREADS) void k_pt_mean_loglike(const double* chain_L, long long cap, int N, long long start,
                                                                long long stop, long long stride, double* out) {
    __shared__ double part[PT_THREADS / 64];
    const size_t m = blockIdx.x;
    const long long nsel = (stop - start + stride - 1) / stride;
    const long long total = nsel * N;
    double s = 0.0;
    for (long long e = threadIdx.x; e < total; e += blockDim.x) {
        const long long row = start + (e / N) * stride, w = e % N;
        s += chain_L[((size_t)m * cap + row) * N + w];
    }
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += part[w];
        out[m] = total > 0 ? t / (double)total : __builtin_nan("");
    }
}

}  // namespace

hipError_t pt_swap_launch(int groups, hipStream_t st, const PtSwapArgs& a) {
    if (a.nblobs > 0)
        hipLaunchKernelGGL(k_pt_swap<true>, dim3(groups), dim3(PT_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(k_pt_swap<false>, dim3(groups), dim3(PT_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t pt_init_launch(const double* X, double* lp, double* L, double* P, const double* beta, const double* box_lo,
                          const double* box_hi, uint32_t* status, int32_t B, int32_t N, int32_t D, hipStream_t st, double* blobs,
                          int32_t nblobs) {
    hipLaunchKernelGGL(k_pt_init, dim3(B), dim3(64), 0, st, X, lp, L, P, beta, box_lo, box_hi, status, N, D, blobs, blobs ? nblobs : 0);
    return hipGetLastError();
}

hipError_t pt_relp_launch(double* lp, const double* L, const double* P, const double* beta, int32_t B, int32_t N, hipStream_t st) {
    hipLaunchKernelGGL(k_pt_relp, dim3(B), dim3(PT_THREADS), 0, st, lp, L, P, beta, N);
    return hipGetLastError();
}

hipError_t pt_mean_launch(const double* chain_L, long long cap, int32_t B, int32_t N, long long start, long long stop,
                          long long stride, double* out, hipStream_t st) {
    hipLaunchKernelGGL(k_pt_mean_loglike, dim3(B), dim3(PT_THREADS), 0, st, chain_L, cap, N, start, stop, stride, out);
    return hipGetLastError();
}

}  // namespace emx

#pragma GCC visibility push(default)
extern "C" {

int emx_host_pt_swap_draws(uint64_t seed, uint64_t step, int64_t nwalkers, int32_t ntemps, int32_t* perm_out, double* logu_out) {
    if (nwalkers < 1 || nwalkers > (int64_t)1 << 30 || ntemps < 1 || (ntemps > 1 && (!perm_out || !logu_out))) return -1;
    if ((int64_t)(ntemps - 1) * nwalkers > (int64_t)0xffffffff) return -1;
    for (int i = 1; i < ntemps; ++i) {
        const emx::PermKey pk = emx::pt_perm_key((uint64_t)nwalkers, seed, step, i);
        for (int64_t k = 0; k < nwalkers; ++k) {
            const size_t o = (size_t)(i - 1) * nwalkers + k;
            perm_out[o] = (int32_t)emx::perm_fwd((uint32_t)k, pk);
            logu_out[o] = emx::plan_log_tab(emx::pt_swap_uniform(seed, step, i, (uint32_t)k, (uint32_t)nwalkers), emx::h_plan_log_rows);
        }
    }
    return 0;
}

int emx_host_pt_adapt_ladder(const double* betas, const int64_t* accepts, int32_t ntemps, int64_t nwalkers, double lag,
                             double time, int64_t t, double* out) {
    if (ntemps < 1 || nwalkers < 1 || !betas || !out || (ntemps > 1 && !accepts) || t < 0) return -1;
    if (!(lag > 0.0) || !(time > 0.0) || lag == __builtin_inf() || time == __builtin_inf()) return -1;
    for (int i = 0; i < ntemps; ++i) out[i] = betas[i];
    emx::pt_adapt_ladder(betas, accepts, ntemps, (long long)nwalkers, lag, time, (long long)t, out);
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
