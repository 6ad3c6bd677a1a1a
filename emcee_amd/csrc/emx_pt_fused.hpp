// Fused tempered targets (include/emx.h: emx_pt_set_target_fused; emcee_amd.targets.PTFused / compile_fused_pt).  PUBLIC: the header
// a user's translation unit includes to compile their per-row log-likelihood (and, optionally, log-prior) into the tempered
// one-workgroup kernel k_pt_run below; the library includes it for the version constant, the argument struct and the LDS map.
//
//     #include <emx_pt_fused.hpp>                 // hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -I include -I emcee_amd/csrc
//     struct MyLike  { __device__ double operator()(const double* x, int ndim, int member, const void* user) const; };
//     struct MyPrior { __device__ double operator()(const double* x, int ndim, int member, const void* user) const; };
//     EMX_FUSED_PT_TARGET(my_model, MyLike, MyPrior, /*ndim=*/5)      // emits: extern "C" int my_model(emx_pt_fused_launch*)
//     EMX_FUSED_PT_TARGET(my_flat, MyLike, emx::NoFusedPrior, 5)      // no prior functor: the handle's box, or a flat prior
//
// Both functors have the contract of emx_fused_target.hpp's: called by ONE lane a row on `ndim` doubles in LDS, no LDS of their
// own, no barrier, no cross-lane operation.  member = object * ntemps + rung.  The likelihood is untempered; where the prior is
// -inf it is not called.  -inf is legal; a NaN likelihood where the prior is finite raises the reference's error naming (object, rung).
//
// Blobs -- derived quantities recorded with every sample (PTSampler.get_blobs) -- come from the likelihood's five-argument form,
// emx_fused_target.hpp's contract:
//
//     struct MyLike { __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const; };
//     EMX_FUSED_PT_TARGET_BLOBS(my_model, MyLike, MyPrior, /*ndim=*/5, /*nblobs=*/2)
//
// The call writes blobs[0 ... nblobs) (lane-private, zero on entry; 1 <= nblobs <= 32, any value is legal) and returns the untempered
// likelihood as before; the prior produces none.  A walker's blobs are replaced exactly when its proposal is accepted, an accepted
// swap exchanges them with x, L and P, and where the prior is -inf (an initial-state walker) they are NaN.  Everything else of the run
// is bit for bit that of the same functor without blobs.
//
// k_pt_run: workgroup g runs object g -- all its ntemps rungs -- for a whole launch.  No workgroup waits for another.  LDS map
// (pt_lds_layout; T rungs, N walkers, D dims, B plan steps, R staging rows a rung, DS = D | 1):
//   doubles  X (T, N, D) | lp, L, P (T, N) each | plan s0, logu, fac (B, T, N) each | beta (T) | swap log-uniforms (T - 1, N) |
//            staging rows (T, R, DS) | staging factors (T, R) | box lo, hi (D) each
//   64-bit   seeds (T) | swap accepts of the launch (T - 1)
//   32-bit   plan order, p0, p1, p2 (B, T, N) each | swap partners (T - 1, N) | moves (B, T) | accept counts (T, N) | pair accepts (T)
//   bytes    accept flags (T, N)
//   doubles  (only with K blobs, behind everything above so that K = 0 moves no offset) the walkers' blobs (T, N, K) | staging blobs (T, R, K)
// A half-step is two passes over the rows of all rungs (T R rows) with a barrier between them: pass 1 (G lanes a row) makes every
// proposal with small_propose into its staging row; pass 2 (one lane a row) is prior, likelihood, k_batch_cb<..., TEMPERED>'s
// decision and the commit.  The swap pass is k_pt_swap's on LDS, its draws made by every lane before the step's half-steps (they do
// not depend on the state), the pair chain itself nothing but LDS reads, writes and one barrier a pair.
//
// DATA form (emx_pt_fused_data.hpp: EMX_FUSED_PT_DATA_TARGET): LIKE is a model with base and term members whose likelihood sums over
// the object's data, and pass 2 -- and the initial state -- give every row a WAVE where the plain form gives it a lane: lane 0
// evaluates the prior, fused_data_value (emx_kernels.hpp) the likelihood with the 64 lanes striding over the data, lane 0 takes the
// decision and the wave commits the row.  Pass 1, the plans, the swap pass, the ladder update and the chain append are the text above.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "emx_fused_target.hpp"
#include "emx_pt.hpp"

// bumped with ANY change of PtRunArgs or of k_pt_run's LDS layout: a launcher and a library of different values refuse each other
#ifndef EMX_FUSED_PT_ABI
#define EMX_FUSED_PT_ABI 3u
#endif

namespace emx {

constexpr int PT_RUN_MAX_THREADS = 512;      // 8 waves a workgroup: up to 256 VGPRs a lane, so that four proposal forms and a user model fit without scratch

struct NoFusedPrior {};      // EMX_FUSED_PT_TARGET's prior argument: no prior functor (the handle's box, or a flat prior)

struct PtRunArgs {
    // member-strided state of the whole handle (member m = g T + t): X (B, N, D); lp, L, P, acc, acc_count (B, N); beta (B)
    double *X, *lp, *L, *P, *beta;
    uint8_t* acc;
    uint32_t* acc_count;
    uint32_t* status;
    const unsigned long long* seeds;
    unsigned long long *attempts, *accepts;      // (B / T, T - 1)
    // the chains, member-major with `cap` rows a member; row0: the first row this launch appends
    double *chain, *chain_lp, *chain_L, *chain_beta;
    long long cap, row0;
    const double *box_lo, *box_hi;               // nullptr: no box
    // the move schedule and the Gaussian moves' per-launch arrays, as SmallRunArgs
    double a[SMALL_MAX_MOVES], sigma[SMALL_MAX_MOVES], g0[SMALL_MAX_MOVES], gammas[SMALL_MAX_MOVES], cdf[SMALL_MAX_MOVES];
    int32_t kind[SMALL_MAX_MOVES], nsplits[SMALL_MAX_MOVES], gmode[SMALL_MAX_MOVES];
    double gsigma[SMALL_MAX_MOVES];
    const double* gscale[SMALL_MAX_MOVES];
    const double* step_fac;                      // (B, nsteps)
    const int32_t* step_col;                     // (nsteps)
    int32_t nmoves, smax;                        // smax: the most splits of any move (half-steps a step)
    unsigned long long step0;
    long long i0;
    int32_t T, N, D, nsteps, thin_by, store, plan_steps, eval0;
    int32_t stage_rows, max_rows;                // staging rows a rung; rows of the largest split (> stage_rows: a half-step runs in chunks)
    long long swap_every;
    int32_t adapt;
    double lag, time;
    long long adapt_t0;                          // the update counter t before this launch's first pass
    const void* user;
    const long long* ndata;                      // DATA form: the data count of every member (B); nullptr for a plain target
    // blobs (EMX_FUSED_PT_TARGET_BLOBS; nblobs 0: none): the walkers' current ones (B, N, nblobs) and the plane (B, cap, N, nblobs)
    double *blobs, *chain_blobs;
    int32_t nblobs;
};

// the LDS map of one object, in bytes from the start of dynamic LDS (host and device: one definition)
struct PtLds {
    size_t total;          // > SMALL_LDS_MAX on the host: refused; the offsets below are then meaningless
    uint32_t X, lp, L, P, s0, logu, fac, beta, swlu, stage, sfac, box, seeds, swacc, order, p0, p1, p2, swj, mvs, acnt, pacc, accs;
    uint32_t wbl, sbl;     // K > 0 only: the walkers' blobs and the staging blobs
};

__host__ __device__ inline PtLds pt_lds_layout(int64_t T, int64_t N, int64_t D, int64_t B, int64_t R, int64_t K = 0) {
    PtLds o;
    const size_t TN = (size_t)(T * N), plan = (size_t)B * TN, pairs = (size_t)(T > 1 ? (T - 1) * N : 0), DS = (size_t)(D | 1);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += bytes;
        return (uint32_t)here;
    };
    o.X = take(TN * (size_t)D * 8);
    o.lp = take(TN * 8);
    o.L = take(TN * 8);
    o.P = take(TN * 8);
    o.s0 = take(plan * 8);
    o.logu = take(plan * 8);
    o.fac = take(plan * 8);
    o.beta = take((size_t)T * 8);
    o.swlu = take(pairs * 8);
    o.stage = take((size_t)(T * R) * DS * 8);
    o.sfac = take((size_t)(T * R) * 8);
    o.box = take(2 * (size_t)D * 8);
    o.seeds = take((size_t)T * 8);
    o.swacc = take((size_t)T * 8);
    o.order = take(plan * 4);
    o.p0 = take(plan * 4);
    o.p1 = take(plan * 4);
    o.p2 = take(plan * 4);
    o.swj = take(pairs * 4);
    o.mvs = take((size_t)(B * T) * 4);
    o.acnt = take(TN * 4);
    o.pacc = take((size_t)T * 4);
    o.accs = take(TN);
    o.wbl = o.sbl = 0;
    if (K > 0) {           // behind every region a blob-free object has: K = 0 moves no offset and takes no byte
        at = (at + 7) & ~(size_t)7;
        o.wbl = take(TN * (size_t)K * 8);
        o.sbl = take((size_t)(T * R) * (size_t)K * 8);
    }
    o.total = (at + 15) & ~(size_t)15;
    return o;
}

struct PtMember {          // what small_propose needs of a rung
    uint32_t* st;
    __device__ __forceinline__ uint32_t* status() const { return st; }
};

// prior, likelihood and tempered log-probability of one row: k_batch_cb<..., TEMPERED>'s and k_pt_init's rule.  -> the NaN status
// (The prior -- functor, else box, else flat -- is written out here and in pt_row_eval_data; the rest of the rule here and in
// pt_row_finish.  Each pair must agree.)
// NBLOBS > 0: the likelihood's five-argument form writes the row's blobs (zeroed here first; NaN where the prior is -inf)
template <typename LIKE, typename PRIOR, int NBLOBS = 0>
__device__ __forceinline__ bool pt_row_eval(const double* x, int D, int member, const void* user, double beta, const double* lo,
                                            const double* hi, bool box, double& pq, double& lq, double& lpn, double* blobs = nullptr) {
    if constexpr (!std::is_same<PRIOR, NoFusedPrior>::value) {
        pq = PRIOR{}(x, D, member, user);
    } else {
        bool in = true;
        if (box)
            for (int d = 0; d < D; ++d) in = in && x[d] >= lo[d] && x[d] <= hi[d];
        pq = in ? 0.0 : -__builtin_inf();
    }
    const bool pinf = pq == -__builtin_inf();
    double lraw = -__builtin_inf();
    if constexpr (NBLOBS > 0) {
#pragma unroll
        for (int k = 0; k < NBLOBS; ++k) blobs[k] = pinf ? __builtin_nan("") : 0.0;
        if (!pinf) lraw = LIKE{}(x, D, member, user, blobs);
    } else {
        if (!pinf) lraw = LIKE{}(x, D, member, user);      // the likelihood of a row outside the prior is ignored: not called
    }
    lq = pinf ? -__builtin_inf() : lraw;
    lpn = pt_tempered(beta, lq, pq);
    return (!pinf && lraw != lraw) || lpn != lpn;
}

// the DATA form's prior and untempered likelihood of one row, by a WHOLE wave (every lane active; `bad`, the same in every lane: the
// row reaches neither prior nor model): lane 0 evaluates the prior -- pt_row_eval's -- and every lane gets it; where it is finite the
// likelihood is fused_data_value's (emx_fused_target_data.hpp, "THE VALUE").  -> pinf (the same in every lane): the row is outside
// the prior, or bad
template <typename MODEL, typename PRIOR>
__device__ __forceinline__ bool pt_row_eval_data(const double* x, int D, int member, const void* user, long long ndata, const double* lo,
                                                 const double* hi, bool box, bool bad, int lane, double& pq, double& lraw) {
    double p = -__builtin_inf();
    if (lane == 0 && !bad) {
        if constexpr (!std::is_same<PRIOR, NoFusedPrior>::value) {
            p = PRIOR{}(x, D, member, user);
        } else {
            bool in = true;
            if (box)
                for (int d = 0; d < D; ++d) in = in && x[d] >= lo[d] && x[d] <= hi[d];
            p = in ? 0.0 : -__builtin_inf();
        }
    }
    pq = wave_first(p);
    const bool pinf = bad || pq == -__builtin_inf();
    lraw = fused_data_value<MODEL>(x, D, member, user, ndata, pinf, lane);      // (the model of a row outside the prior is not called)
    return pinf;
}

// the rest of pt_row_eval's rule from those two values (lane 0).  -> the NaN status
__device__ __forceinline__ bool pt_row_finish(bool pinf, double pq, double lraw, double beta, double& lq, double& lpn) {
    lq = pinf ? -__builtin_inf() : lraw;
    lpn = pt_tempered(beta, lq, pq);
    return (!pinf && lraw != lraw) || lpn != lpn;
}

template <int G, int V, int CH, int MOVESEL, typename LIKE, typename PRIOR, bool DATA = false, int NBLOBS = 0>
static __global__ __launch_bounds__(PT_RUN_MAX_THREADS) void k_pt_run(const PtRunArgs A) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int WPW = 64 / G;
    const int T = A.T, N = A.N, D = A.D, NT = blockDim.x, tid = threadIdx.x, B = A.plan_steps, R = A.stage_rows;
    const int lane = tid & 63, wv = tid >> 6, nwave = NT >> 6, sub = lane / G, gl = lane % G;
    const int TN = T * N, TR = T * R, DS = D | 1, ND = N * D;
    const size_t m0 = (size_t)blockIdx.x * (size_t)T;
    static_assert(!(DATA && NBLOBS > 0), "the DATA form carries no blobs");
    const PtLds O = pt_lds_layout(T, N, D, B, R, NBLOBS);
    char* lds = reinterpret_cast<char*>(smem);
    double* Xs = reinterpret_cast<double*>(lds + O.X);
    double* lps = reinterpret_cast<double*>(lds + O.lp);
    double* Ls = reinterpret_cast<double*>(lds + O.L);
    double* Ps = reinterpret_cast<double*>(lds + O.P);
    double* s0s = reinterpret_cast<double*>(lds + O.s0);
    double* logus = reinterpret_cast<double*>(lds + O.logu);
    double* facs = reinterpret_cast<double*>(lds + O.fac);
    double* betaS = reinterpret_cast<double*>(lds + O.beta);
    double* swlu = reinterpret_cast<double*>(lds + O.swlu);
    double* stage = reinterpret_cast<double*>(lds + O.stage);
    double* sfac = reinterpret_cast<double*>(lds + O.sfac);
    double* loS = reinterpret_cast<double*>(lds + O.box);
    double* hiS = loS + D;
    unsigned long long* seedS = reinterpret_cast<unsigned long long*>(lds + O.seeds);
    unsigned long long* swacc = reinterpret_cast<unsigned long long*>(lds + O.swacc);
    int* orders = reinterpret_cast<int*>(lds + O.order);
    int* p0s = reinterpret_cast<int*>(lds + O.p0);
    int* p1s = reinterpret_cast<int*>(lds + O.p1);
    int* p2s = reinterpret_cast<int*>(lds + O.p2);
    int* swj = reinterpret_cast<int*>(lds + O.swj);
    int* mvs = reinterpret_cast<int*>(lds + O.mvs);
    uint32_t* acnt = reinterpret_cast<uint32_t*>(lds + O.acnt);
    unsigned int* pacc = reinterpret_cast<unsigned int*>(lds + O.pacc);
    uint8_t* accs = reinterpret_cast<uint8_t*>(lds + O.accs);
    [[maybe_unused]] double* wbl = reinterpret_cast<double*>(lds + O.wbl);      // NBLOBS > 0: the walkers' blobs (T, N, NBLOBS)
    [[maybe_unused]] double* sbl = reinterpret_cast<double*>(lds + O.sbl);      // ... and the staging rows' (T, R, NBLOBS)
    const bool box = A.box_lo != nullptr;

    // ---- the object's rungs are consecutive members: one contiguous block of every member-strided array ----
    for (int e = tid; e < TN * D; e += NT) Xs[e] = A.X[m0 * (size_t)ND + e];
    for (int e = tid; e < TN; e += NT) {
        lps[e] = A.lp[m0 * (size_t)N + e];
        Ls[e] = A.L[m0 * (size_t)N + e];
        Ps[e] = A.P[m0 * (size_t)N + e];
        acnt[e] = 0u;
        accs[e] = A.acc[m0 * (size_t)N + e];
    }
    for (int t = tid; t < T; t += NT) {
        betaS[t] = A.beta[m0 + t];
        seedS[t] = A.seeds[m0 + t];
        swacc[t] = 0ull;
        pacc[t] = 0u;
    }
    if (box)
        for (int d = tid; d < D; d += NT) {
            loS[d] = A.box_lo[d];
            hiS[d] = A.box_hi[d];
        }
    if constexpr (NBLOBS > 0)
        for (int e = tid; e < TN * NBLOBS; e += NT) wbl[e] = A.blobs[m0 * (size_t)N * NBLOBS + e];
    __syncthreads();
    if (A.eval0) {
        // the initial state (k_pt_init's rule), every walker's own row through the functors
        if constexpr (DATA) {
            for (int r = __builtin_amdgcn_readfirstlane(wv); r < TN; r += nwave) {      // wave-uniform: a wave a walker's own row
                const int t = r / N;
                double pq, lraw;
                const bool pinf = pt_row_eval_data<LIKE, PRIOR>(Xs + (size_t)r * D, D, (int)(m0 + t), A.user, A.ndata[m0 + t], loS, hiS, box,
                                                                false, lane, pq, lraw);
                if (lane == 0) {
                    double lq, lpn;
                    if (pt_row_finish(pinf, pq, lraw, betaS[t], lq, lpn)) raise_status(A.status + (m0 + t) * SMALL_STATUS_WORDS, ST_NAN_LOGP);
                    Ps[r] = pq;
                    Ls[r] = lq;
                    lps[r] = lpn;
                }
            }
        } else
        for (int r = tid; r < TN; r += NT) {
            const int t = r / N;
            double pq, lq, lpn;
            bool nan;
            if constexpr (NBLOBS > 0)       // the walker's own blobs, NaN where P is -inf
                nan = pt_row_eval<LIKE, PRIOR, NBLOBS>(Xs + (size_t)r * D, D, (int)(m0 + t), A.user, betaS[t], loS, hiS, box, pq, lq, lpn,
                                                       wbl + (size_t)r * NBLOBS);
            else
                nan = pt_row_eval<LIKE, PRIOR>(Xs + (size_t)r * D, D, (int)(m0 + t), A.user, betaS[t], loS, hiS, box, pq, lq, lpn);
            if (nan) raise_status(A.status + (m0 + t) * SMALL_STATUS_WORDS, ST_NAN_LOGP);
            Ps[r] = pq;
            Ls[r] = lq;
            lps[r] = lpn;
        }
        __syncthreads();
    }
    const unsigned long long seed0 = seedS[0];     // the object's swap draws are keyed by its rung-0 seed
    int row = 0;                                   // stored rows appended by this launch
    long long npass = 0;                           // swap passes made by this launch
    for (int sb = 0; sb < A.nsteps; sb += B) {
        const int nb = min(B, A.nsteps - sb);
        __syncthreads();                           // the previous batch's plans are no longer read
        // ---- every rung's plans of nb steps in one pass (k_small_run's plan pass, entry for entry, under the rung's own seed) ----
        for (int e = tid; e < nb * TN; e += NT) {
            const int b = e / TN, rem = e - b * TN, t = rem / N, pos = rem - t * N;
            NativeArgs na;
            na.seed = seedS[t];
            na.step = A.step0 + (unsigned long long)(sb + b);
            const int m = A.nmoves == 1 ? 0 : native_move_choice(na.seed, na.step, A.cdf, A.nmoves);
            const int kind = MOVESEL == SMALL_ANY_MOVE ? A.kind[m] : MOVESEL;
            if (pos == 0) mvs[b * T + t] = m;
            na.pk = make_perm_key((uint64_t)N, na.seed, na.step);
            int i = 0, a0 = 0, a1 = 0, a2 = 0;
            double z = 0.0, lu = 0.0, fc = 0.0;
            const int S = A.nsplits[m];
            // (the move ladder, SMALL_ANY_MOVE in emx_kernels.hpp, for this kernel's two selectors: every copy agrees arm for arm)
            if (MOVESEL == SMALL_ANY_MOVE && kind == MOVE_GAUSS) {
                double u;
                native_gauss_slot(na, D, A.gmode[m], A.step_col ? A.step_col[sb + b] : 0, pos, i, a0, a1, a2, z, u);
                lu = plan_log_uniform(u);
            } else if (MOVESEL == MOVE_STRETCH || (MOVESEL == SMALL_ANY_MOVE && kind == MOVE_STRETCH))
                small_plan_entry<MOVE_STRETCH>(na, N, D, S, pos, A.a[m], A.sigma[m], A.g0[m], i, a0, a1, a2, z, lu, fc);
            else if (MOVESEL == SMALL_ANY_MOVE && kind == MOVE_DE)
                small_plan_entry<MOVE_DE>(na, N, D, S, pos, A.a[m], A.sigma[m], A.g0[m], i, a0, a1, a2, z, lu, fc);
            else
                small_plan_entry<MOVE_SNOOKER>(na, N, D, S, pos, A.a[m], A.sigma[m], A.g0[m], i, a0, a1, a2, z, lu, fc);
            orders[e] = i;
            p0s[e] = a0;
            p1s[e] = a1;
            p2s[e] = a2;
            s0s[e] = z;
            logus[e] = lu;
            facs[e] = fc;
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            const int s = sb + b;
            const unsigned long long step = A.step0 + (unsigned long long)s;
            const bool pass = A.swap_every > 0 && (step + 1ull) % (unsigned long long)A.swap_every == 0ull;      // workgroup-uniform
            if (pass && T > 1) {
                // the pass's draws: pairing and log-uniform of every (pair, walker), side by side, before the state they meet exists
                for (int e = tid; e < (T - 1) * N; e += NT) {
                    const int i = 1 + e / N, k = e - (i - 1) * N;
                    const PermKey pk = pt_perm_key((uint64_t)N, seed0, step, i);
                    swj[e] = (int)perm_fwd((uint32_t)k, pk);
                    swlu[e] = plan_log_uniform(pt_swap_uniform(seed0, step, i, (uint32_t)k, (uint32_t)N));
                }
                for (int t = tid; t < T; t += NT) pacc[t] = 0u;
            }
            // ---- the half-steps: phase k is split k of every rung whose move has one (a rung's move is its own draw) ----
            // (a split's rows read their own walkers and the complement only, so a split larger than the staging area runs in
            // chunks of R slots to the same bits)
            for (int k = 0; k < A.smax; ++k)
            for (int c0 = 0; c0 < A.max_rows; c0 += R) {
                // pass 1: the proposals of all rungs into their staging rows (rung t, slot -> row t R + slot), G lanes a row
                for (int rb = wv * WPW; rb < TR; rb += nwave * WPW) {              // wave-uniform
                    const int r = rb + sub;
                    if (r >= TR) continue;                                          // row-uniform from here on
                    // THE SLOT RULE (rung, slot, move, split sizes, plan entry): the same text stands in both forms of pass 2 below and
                    // must agree with them to the bit, or a proposal is decided against another walker's plan entry.  Only the last
                    // skip differs: this pass keeps a dead row (slot >= ns) in flight, both forms of pass 2 skip it.
                    const int t = r / R, slot = c0 + (r - t * R);
                    const int m = mvs[b * T + t];
                    const int kind = MOVESEL == SMALL_ANY_MOVE ? A.kind[m] : MOVESEL;
                    const int S = kind == MOVE_GAUSS ? 1 : A.nsplits[m];
                    if (k >= S) continue;
                    const SplitSizes sz = split_sizes(N, S);
                    const int ns = sz.of(k), pos0 = k * sz.q + min(k, sz.r);
                    if (c0 >= ns) continue;
                    const bool live = slot < ns;
                    const int pos = (b * T + t) * N + pos0 + (live ? slot : 0);
                    const double* Xt = Xs + (size_t)t * ND;
                    const PtMember M{A.status + (m0 + t) * SMALL_STATUS_WORDS};
                    const double gam = A.gammas[m];
                    Row<G, V, CH> q;
                    double factor = 0.0;
                    bool badq = false;
                    const int i = orders[pos], j0 = p0s[pos], j1 = p1s[pos], j2 = p2s[pos];
                    // (the move ladder, SMALL_ANY_MOVE in emx_kernels.hpp, for this kernel's two selectors: every copy agrees arm for arm)
                    if (MOVESEL == SMALL_ANY_MOVE && kind == MOVE_GAUSS) {
                        GaussGen gg;
                        gg.gseed = seedS[t];
                        gg.gstep = step;
                        gg.gfac = A.step_fac ? A.step_fac[(m0 + t) * (size_t)A.nsteps + s] : 1.0;
                        gg.gsigma = A.gsigma[m];
                        gg.gscale = A.gscale[m];
                        small_propose<G, V, CH, MOVE_GAUSS>(M, Xt, live, i, j0, j1, j2, s0s[pos], facs[pos], gam, D, gl, sub, q, factor, badq, &gg);
                    } else if (MOVESEL == MOVE_STRETCH || (MOVESEL == SMALL_ANY_MOVE && kind == MOVE_STRETCH))
                        small_propose<G, V, CH, MOVE_STRETCH>(M, Xt, live, i, j0, j1, j2, s0s[pos], facs[pos], gam, D, gl, sub, q, factor, badq);
                    else if (MOVESEL == SMALL_ANY_MOVE && kind == MOVE_DE)
                        small_propose<G, V, CH, MOVE_DE>(M, Xt, live, i, j0, j1, j2, s0s[pos], facs[pos], gam, D, gl, sub, q, factor, badq);
                    else
                        small_propose<G, V, CH, MOVE_SNOOKER>(M, Xt, live, i, j0, j1, j2, s0s[pos], facs[pos], gam, D, gl, sub, q, factor, badq);
                    if (live) {
#pragma unroll
                        for (int c = 0; c < CH; ++c)
#pragma unroll
                            for (int v = 0; v < V; ++v) {
                                const int d = (c * G + gl) * V + v;
                                if (d < D) stage[(size_t)r * DS + d] = q.x[c][v];
                            }
                        if (gl == 0) sfac[r] = badq ? -__builtin_inf() : factor;
                    }
                }
                __syncthreads();
                if constexpr (DATA) {
                    // pass 2, a wave a row -- the prior by lane 0, the model over the object's data by the wave, the tempered
                    // decision by lane 0, the commit by every lane; the values stored are the one-lane form's
                    for (int r = __builtin_amdgcn_readfirstlane(wv); r < TR; r += nwave) {      // wave-uniform, as every skip below
                        // (pass 1's slot rule, a dead row skipped)
                        const int t = r / R, slot = c0 + (r - t * R);
                        const int m = mvs[b * T + t];
                        const int kind = MOVESEL == SMALL_ANY_MOVE ? A.kind[m] : MOVESEL;
                        const int S = kind == MOVE_GAUSS ? 1 : A.nsplits[m];
                        if (k >= S) continue;
                        const SplitSizes sz = split_sizes(N, S);
                        const int ns = sz.of(k), pos0 = k * sz.q + min(k, sz.r);
                        if (slot >= ns) continue;
                        const int pos = (b * T + t) * N + pos0 + slot;
                        const int w = t * N + orders[pos];
                        const double* qrow = stage + (size_t)r * DS;
                        const double fac = sfac[r];                                 // the same value in every lane
                        const bool bad = fac == -__builtin_inf();                   // (-inf: as below)
                        double pq, lraw, lq = 0.0, lpn = 0.0;
                        const bool pinf = pt_row_eval_data<LIKE, PRIOR>(qrow, D, (int)(m0 + t), A.user, A.ndata[m0 + t], loS, hiS, box, bad,
                                                                        lane, pq, lraw);
                        int acc = 0;
                        if (lane == 0 && !bad) {
                            if (pt_row_finish(pinf, pq, lraw, betaS[t], lq, lpn)) raise_status(A.status + (m0 + t) * SMALL_STATUS_WORDS, ST_NAN_LOGP);
                            const double lnpdiff = fac + lpn - lps[w];             // (small_update's accept rule, emx_kernels.hpp, on the tempered lp)
                            acc = lnpdiff > logus[pos] ? 1 : 0;
                        }
                        const bool accept = __builtin_amdgcn_readfirstlane(acc) != 0;
                        if (accept) {
                            wave_commit_row(Xs + (size_t)w * D, qrow, D, lane);
                            if (lane == 0) {
                                lps[w] = lpn;
                                Ls[w] = lq;
                                Ps[w] = pq;
                            }
                        }
                        if (lane == 0) accs[w] = accept ? 1 : 0;
                    }
                } else
                // pass 2: one lane a row -- prior, likelihood, the tempered decision, the commit
                for (int r = tid; r < TR; r += NT) {
                    // (pass 1's slot rule, a dead row skipped)
                    const int t = r / R, slot = c0 + (r - t * R);
                    const int m = mvs[b * T + t];
                    const int kind = MOVESEL == SMALL_ANY_MOVE ? A.kind[m] : MOVESEL;
                    const int S = kind == MOVE_GAUSS ? 1 : A.nsplits[m];
                    if (k >= S) continue;
                    const SplitSizes sz = split_sizes(N, S);
                    const int ns = sz.of(k), pos0 = k * sz.q + min(k, sz.r);
                    if (slot >= ns) continue;
                    const int pos = (b * T + t) * N + pos0 + slot;
                    const int w = t * N + orders[pos];
                    const double* qrow = stage + (size_t)r * DS;
                    const double fac = sfac[r];
                    bool accept = false;
                    if (fac != -__builtin_inf()) {                                 // (-inf: a non-finite proposal, rejected without reaching a functor)
                        double pq, lq, lpn;
                        bool nan;
                        if constexpr (NBLOBS > 0)       // the lane writes its row's staging blobs
                            nan = pt_row_eval<LIKE, PRIOR, NBLOBS>(qrow, D, (int)(m0 + t), A.user, betaS[t], loS, hiS, box, pq, lq, lpn,
                                                                   sbl + (size_t)r * NBLOBS);
                        else
                            nan = pt_row_eval<LIKE, PRIOR>(qrow, D, (int)(m0 + t), A.user, betaS[t], loS, hiS, box, pq, lq, lpn);
                        if (nan) raise_status(A.status + (m0 + t) * SMALL_STATUS_WORDS, ST_NAN_LOGP);
                        const double lnpdiff = fac + lpn - lps[w];                 // (small_update's accept rule, emx_kernels.hpp, on the tempered lp)
                        accept = lnpdiff > logus[pos];
                        if (accept) {
                            for (int d = 0; d < D; ++d) Xs[(size_t)w * D + d] = qrow[d];
                            if constexpr (NBLOBS > 0) {
#pragma unroll
                                for (int q = 0; q < NBLOBS; ++q) wbl[(size_t)w * NBLOBS + q] = sbl[(size_t)r * NBLOBS + q];
                            }
                            lps[w] = lpn;
                            Ls[w] = lq;
                            Ps[w] = pq;
                        }
                    }
                    accs[w] = accept ? 1 : 0;
                }
                __syncthreads();
            }
            // ---- the swap pass (k_pt_swap's, on LDS): pairs from the hottest, each seeing what the one before left ----
            if (pass) {
                if (T > 1) {
                    for (int i = T - 1; i >= 1; --i) {
                        const double bh = betaS[i], bc = betaS[i - 1];
                        const double dbeta = bc - bh;
                        unsigned int mine = 0u;
                        for (int k = tid; k < N; k += NT) {
                            const int e = (i - 1) * N + k;
                            const int rh = i * N + k, rc = (i - 1) * N + swj[e];
                            const double Lh = Ls[rh], Lc = Ls[rc];
                            const double diff = Lh - Lc;
                            if (dbeta * diff > swlu[e]) {
                                const double Ph = Ps[rh], Pc = Ps[rc];
                                double* xh = Xs + (size_t)rh * D;
                                double* xc = Xs + (size_t)rc * D;
                                for (int d = 0; d < D; ++d) {
                                    const double v = xh[d];
                                    xh[d] = xc[d];
                                    xc[d] = v;
                                }
                                if constexpr (NBLOBS > 0) {       // a blob belongs to the point: it changes places with x
#pragma unroll
                                    for (int q = 0; q < NBLOBS; ++q) {
                                        const double v = wbl[(size_t)rh * NBLOBS + q];
                                        wbl[(size_t)rh * NBLOBS + q] = wbl[(size_t)rc * NBLOBS + q];
                                        wbl[(size_t)rc * NBLOBS + q] = v;
                                    }
                                }
                                Ls[rh] = Lc;
                                Ps[rh] = Pc;
                                lps[rh] = pt_tempered(bh, Lc, Pc);
                                Ls[rc] = Lh;
                                Ps[rc] = Ph;
                                lps[rc] = pt_tempered(bc, Lh, Ph);
                                ++mine;
                            }
                        }
                        if (mine) atomicAdd(&pacc[i - 1], mine);
                        __syncthreads();
                    }
                    for (int t = tid; t < T - 1; t += NT) swacc[t] += (unsigned long long)pacc[t];
                    if (A.adapt && T > 2) {
                        // the ladder update in rung order in one lane; then lp of every walker of the moved rungs from the new betas
                        if (tid == 0) pt_adapt_ladder(betaS, pacc, T, (long long)N, A.lag, A.time, A.adapt_t0 + npass, betaS);
                        __syncthreads();
                        for (int e = tid; e < (T - 2) * N; e += NT) {
                            const int r = N + e;
                            lps[r] = pt_tempered(betaS[1 + e / N], Ls[r], Ps[r]);
                        }
                    }
                    __syncthreads();
                }
                ++npass;
            }
            // ---- a stored step: the state after the swap pass; the accept counts move on stored steps ----
            if (A.store && ((A.i0 + s + 1) % A.thin_by == 0)) {
                const size_t crow = (size_t)(A.row0 + row);
                for (int e = tid; e < TN * D; e += NT) {
                    const int t = e / ND;
                    A.chain[((m0 + t) * (size_t)A.cap + crow) * (size_t)ND + (e - t * ND)] = Xs[e];
                }
                for (int e = tid; e < TN; e += NT) {
                    const int t = e / N;
                    const size_t o = ((m0 + t) * (size_t)A.cap + crow) * (size_t)N + (e - t * N);
                    A.chain_lp[o] = lps[e];
                    A.chain_L[o] = Ls[e];
                    acnt[e] += accs[e];
                }
                if constexpr (NBLOBS > 0)
                    for (int e = tid; e < TN * NBLOBS; e += NT) {
                        const int t = e / (N * NBLOBS);
                        A.chain_blobs[((m0 + t) * (size_t)A.cap + crow) * (size_t)(N * NBLOBS) + (e - t * N * NBLOBS)] = wbl[e];
                    }
                for (int t = tid; t < T; t += NT) A.chain_beta[(m0 + t) * (size_t)A.cap + crow] = betaS[t];
                ++row;
                __syncthreads();                     // the next half-step overwrites what was just copied
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < TN * D; e += NT) A.X[m0 * (size_t)ND + e] = Xs[e];
    for (int e = tid; e < TN; e += NT) {
        A.lp[m0 * (size_t)N + e] = lps[e];
        A.L[m0 * (size_t)N + e] = Ls[e];
        A.P[m0 * (size_t)N + e] = Ps[e];
        A.acc[m0 * (size_t)N + e] = accs[e];
        A.acc_count[m0 * (size_t)N + e] += acnt[e];
    }
    for (int t = tid; t < T; t += NT) A.beta[m0 + t] = betaS[t];
    if constexpr (NBLOBS > 0)
        for (int e = tid; e < TN * NBLOBS; e += NT) A.blobs[m0 * (size_t)N * NBLOBS + e] = wbl[e];
    if (T > 1 && npass > 0)
        for (int t = tid; t < T - 1; t += NT) {
            const size_t c = (size_t)blockIdx.x * (size_t)(T - 1) + t;
            A.attempts[c] += (unsigned long long)npass * (unsigned long long)N;
            A.accepts[c] += swacc[t];
        }
}

template <typename LIKE, typename PRIOR, int NDIM, int MOVESEL, bool DATA = false, int NBLOBS = 0>
hipError_t launch_pt_move(int grid, int threads, size_t lds, hipStream_t st, const PtRunArgs& a) {
    static size_t lds_granted[MAX_DEVICES] = {};
    return fused_launch_kernel(k_pt_run<fused_g(NDIM), fused_v(NDIM), fused_ch(NDIM), MOVESEL, LIKE, PRIOR, DATA, NBLOBS>, lds_granted, grid,
                               threads, lds, st, a);
}

// the launcher behind EMX_FUSED_PT_TARGET: fused_launch_checks (emx_fused_target.hpp), then one launch of every object
// (include/emx.h: emx_pt_fused_launch).  The probe (grid == 0) also reports whether a prior functor is compiled in.  A descriptor
// whose blob count is not the NBLOBS compiled in is answered 4, as fused_batch_launch answers it.
template <typename LIKE, typename PRIOR, int NDIM, int MOVES, int NBLOBS = 0>
int fused_pt_launch(emx_pt_fused_launch* L) {
    static_assert(NDIM >= 1 && NDIM <= 256, "a fused tempered target has 1 <= ndim <= 256");
    static_assert(NBLOBS >= 0 && NBLOBS <= 32, "a fused tempered target has 0 <= nblobs <= 32");
    static_assert((MOVES & (EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY)) != 0, "no move selector compiled in");
    bool stretch = false;
    const int rc = fused_launch_checks(L, EMX_FUSED_PT_ABI, sizeof(PtRunArgs), NDIM, MOVES, PT_RUN_MAX_THREADS, &stretch, [](emx_pt_fused_launch* d) {
        d->has_prior = std::is_same<PRIOR, NoFusedPrior>::value ? 0 : 1;      // the probe reports it
        return d->nblobs != NBLOBS ? 4 : FUSED_GO_ON;
    });
    if (rc != FUSED_GO_ON) return rc;
    PtRunArgs a = *static_cast<const PtRunArgs*>(L->args);
    if (a.D != NDIM) return 2;
    if (a.nblobs != NBLOBS || (NBLOBS > 0 && !a.blobs)) return 4;
    a.user = L->user;
    return fused_launch_by_moves<MOVES>(stretch, [&](auto sel) {
        return launch_pt_move<LIKE, PRIOR, NDIM, decltype(sel)::value, false, NBLOBS>(L->grid, L->threads, (size_t)L->lds_bytes, (hipStream_t)L->hip_stream, a);
    });
}

}  // namespace emx

#define EMX_FUSED_PT_TARGET_MOVES(name, LikeFunctor, PriorFunctor, ndim, moves)                       \
    extern "C" __attribute__((visibility("default"))) int name(emx_pt_fused_launch* launch) {         \
        return emx::fused_pt_launch<LikeFunctor, PriorFunctor, (ndim), (moves)>(launch);              \
    }
#define EMX_FUSED_PT_TARGET(name, LikeFunctor, PriorFunctor, ndim) \
    EMX_FUSED_PT_TARGET_MOVES(name, LikeFunctor, PriorFunctor, ndim, EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY)
// the likelihood's five-argument form (..., double* blobs) with `nblobs` doubles a sample; both move selectors
#define EMX_FUSED_PT_TARGET_BLOBS(name, LikeFunctor, PriorFunctor, ndim, nblobs)                                                           \
    extern "C" __attribute__((visibility("default"))) int name(emx_pt_fused_launch* launch) {                                              \
        static_assert((nblobs) >= 1, "EMX_FUSED_PT_TARGET_BLOBS: 1 <= nblobs <= 32 (none: EMX_FUSED_PT_TARGET)");                          \
        return emx::fused_pt_launch<LikeFunctor, PriorFunctor, (ndim), EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY, (nblobs)>(launch);   \
    }
