// Fused user targets of the single sampler whose log-probability SUMS OVER DATA (include/emx.h: emx_set_target_fused_data;
// emcee_amd.targets.DeviceFused(..., ndata=) / compile_fused_ensemble(..., data=True)).  PUBLIC: the header a user's translation unit
// includes to compile a likelihood of the form  log p(theta) = base(theta) + sum_k term(theta; datum_k)  into the half-step of a
// large ensemble with a WAVE a row in the data sum, where emx_fused_ensemble.hpp's functor would loop over the data in one lane.
//
//     #include <emx_fused_ensemble_data.hpp>      // hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -I include -I emcee_amd/csrc
//     struct MyModel {                            // stateless; `user`: the device pointer given to DeviceFused
//         // once a row, by one lane: prior, normalisation, all that does not run over the data
//         __device__ double base(const double* x, int ndim, const void* user) const;
//         // datum k of [0, ndata): pure, no LDS of its own, no barrier, no cross-lane operation
//         __device__ double term(const double* x, int ndim, long long k, const void* user) const;
//     };
//     EMX_FUSED_ENSEMBLE_DATA_TARGET(my_model, MyModel, /*ndim=*/5)   // emits: extern "C" int my_model(const emx_fused_ensemble_data_launch*)
//
// `x` points at `ndim` doubles in LDS (the staged row).  `ndata` is a run-time value given when the target is bound
// (0 <= ndata < 2^31), not a template argument: one launcher serves every data set.
//
// THE VALUE.  The log-probability of a row is DEFINED as  base + S  where
//   * lane partial p_l, l = 0 ... 63, starts at +0.0 and adds term(x, ndim, k, user) for k = l, l + 64, l + 128, ... in ascending k
//     (p_l = p_l + term: a separate add, the translation unit is compiled with -ffp-contract=off);
//   * S is the balanced pairwise tree over p_0 ... p_63 -- adjacent pairs, level by level: (p_0 + p_1), (p_2 + p_3), ..., then
//     pairs of those, six levels -- which is what group_sum<64> of emx_kernels.hpp computes.
// It depends on nothing else: not the tile, not the grid, not the rows a workgroup takes, not the move.
// emcee_amd.targets.fused_data_sum(terms) sums a float64 array in exactly this order on the host.
//   * base -inf or NaN: no term is evaluated for that row and the value is base (NaN raises the reference's error, -inf rejects);
//   * a NaN  base + S  raises the reference's error too;
//   * a row with a non-finite coordinate is rejected without reaching the functor;
//   * ndata == 0 gives base + 0.0.
//
// k_halfstep_user_data is k_halfstep_user (emx_fused_ensemble.hpp) with another phase 2: phases 1 (the proposal, G lanes a row,
// staged in LDS) and 3 (commit, chain append) are that kernel's text.  In phase 2 each wave takes rows of the tile in turn: lane 0
// calls base, all 64 lanes stride over the data, the reduction runs with the whole wave active outside any lane-divergent region
// (DPP and permlane reads of inactive lanes are undefined), and lane 0 takes the decision by k_halfstep_user's rule.
// (The two phases and the rule stay this kernel's own text: made of functions shared with k_halfstep_user the kernel computed the
// same bits and was 1.1 to 1.4 % slower at 4 096 walkers x 16, twice -- profiles/ensemble_fused_shared_text.md.  A change of the
// rule there is a change here; tests/test_gpu_ensemble_fused_data.py compares the chains bit for bit.)
// TILE stays the compile-time upper bound of the rows a workgroup takes (the register arrays of phase 1); the rows it actually
// takes are a run-time argument, 4 ... TILE, so that a mid-size ensemble spreads over the chip (fused_ens_data_rows_rule;
// profiles/ensemble_fused_data.md); passes of phase 1 / 3 without a live row are skipped by a workgroup-uniform branch.
// Out of scope: blobs, the one-workgroup small form, several GPUs.  (A batch's data targets: emx_fused_target_data.hpp; PTSampler's:
// emx_pt_fused_data.hpp.)
#pragma once
#include "emx_fused_ensemble.hpp"

// bumped with ANY change of HalfStepArgs, of emx_fused_ensemble_data_launch or of k_halfstep_user_data's launch rules.  A value of its
// own: a data launcher handed the data-free descriptor, and a data-free launcher handed this one, answer 1
#ifndef EMX_FUSED_ENSEMBLE_DATA_ABI
#define EMX_FUSED_ENSEMBLE_DATA_ABI 0x454e4401u
#endif

namespace emx {

// workgroups a CU the default rows-a-workgroup rule asks for before it stops halving the tile.  Measured (profiles/ensemble_fused_data.md,
// the sweep): up to 4 096 walkers 4 rows are the fastest at every count of data, by up to 12x over the whole tile at 16 384 data; at
// 65 536 walkers (128 slots a CU) 4 rows are the fastest at 16 384 data, by 7 %, and behind the fastest (8 rows) by 11 % at 64 data
// and 4 % at 1 024.  32 and not 16, which would take 8 rows there: the step at 16 384 data costs 25 times the step at 64.
constexpr int FUSED_ENS_DATA_WG_PER_CU = 32;

// Rows a workgroup takes by default: the tile of the data-free kernel, halved until the split makes FUSED_ENS_DATA_WG_PER_CU
// workgroups a CU, never below a row a wave.  (Results do not depend on it.)
inline int fused_ens_data_rows_rule(int D, long long nslots, int num_cu) {
    int rows = fused_ens_tile_rule(D);
    while (rows > FUSED_ENS_DATA_MIN_ROWS && (nslots + rows - 1) / rows < (long long)num_cu * FUSED_ENS_DATA_WG_PER_CU) rows /= 2;
    return rows;
}

template <int G, int V, int CH, int MOVE, typename USER, int TILE>
static __global__ __launch_bounds__(FUSED_ENS_THREADS) void k_halfstep_user_data(const HalfStepArgs A, const void* user, const long long ndata,
                                                                                 const int rows) {
    static_assert(G >= 4 && G <= 64 && (64 % G) == 0, "G lanes per walker");
    constexpr int T = FUSED_ENS_THREADS;
    constexpr int WPW = 64 / G;                 // rows a wave and pass
    constexpr int GPB = (T / 64) * WPW;         // rows a workgroup and pass
    static_assert(TILE >= GPB && TILE % GPB == 0 && TILE <= T, "the tile is whole passes of the workgroup");
    constexpr int NPASS = TILE / GPB;
    constexpr int NR = rows_per_pass<MOVE>();
    constexpr bool EVAL = MOVE == MOVE_EVAL;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int D = A.D, DS = D | 1;              // the row stride of k_halfstep_user
    double* const stage = smem;                 // `rows` (<= TILE) rows, a factor a row, a flag a row: fused_ens_lds_of(D, rows)
    double* const sfac = stage + (size_t)rows * DS;
    int* const sflag = reinterpret_cast<int*>(sfac + rows);
    const int tid = threadIdx.x, lane = tid & 63, wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sub = lane / G, gl = lane % G;

    for (int t0 = A.t_lo + (int)blockIdx.x * rows; t0 < A.t_hi; t0 += (int)gridDim.x * rows) {      // workgroup-uniform
        const int nrow = min(rows, A.t_hi - t0);
        // -------- 1. proposals, G lanes a row (k_halfstep_user's; a pass without a live row is skipped) --------
        int wi[NPASS], ja[NPASS], jb[NR >= 3 ? NPASS : 1], jc[NR >= 4 ? NPASS : 1];
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            if (p * GPB >= nrow) continue;      // workgroup-uniform
            const int r = p * GPB + wib * WPW + sub;
            const int pos = A.pos0 + t0 + (r < nrow ? r : 0);
            wi[p] = A.order[pos];
            ja[p] = NR >= 2 ? A.p0[pos] : -1;
            if constexpr (NR >= 3) jb[p] = A.p1[pos];
            if constexpr (NR >= 4) jc[p] = A.p2[pos];
        }
        Row<G, V, CH> xi[NPASS];
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            if (p * GPB >= nrow) continue;      // workgroup-uniform
            const int r = p * GPB + wib * WPW + sub;
            const bool live = r < nrow;
            const int pos = A.pos0 + t0 + (live ? r : 0);
            const int i = wi[p];
            Row<G, V, CH> xa, xb, xc, q;
            load_row<G, V, CH>(xi[p], A.X + (size_t)i * D, D, gl);
            if constexpr (MOVE == MOVE_GAUSS) {
                if (A.disp) load_row<G, V, CH>(xa, A.disp + (size_t)i * D, D, gl);
                else gauss_disp_row<G, V, CH>(xa, A, i, ja[p], D, gl);
            } else if constexpr (NR >= 2) {
                load_row<G, V, CH>(xa, A.X + (size_t)ja[p] * D, D, gl);
            }
            if constexpr (NR >= 3) load_row<G, V, CH>(xb, A.X + (size_t)jb[p] * D, D, gl);
            if constexpr (NR >= 4) load_row<G, V, CH>(xc, A.X + (size_t)jc[p] * D, D, gl);
            double s0 = 0.0, factor = 0.0;
            if constexpr (!EVAL) {
                s0 = (MOVE == MOVE_SNOOKER) ? 0.0 : A.s0[pos];
                factor = A.fac[pos];
            }
            make_proposal<G, V, CH, MOVE>(xi[p], NR >= 2 ? xa : xi[p], NR >= 3 ? xb : xi[p], NR >= 4 ? xc : xi[p], s0, A.gammas, D, gl, q,
                                          factor, ja[p]);
            // a non-finite proposal: the sticky error (ensemble.py:476-479), rejected, never handed to the functor
            bool bl = false;
#pragma unroll
            for (int c = 0; c < CH; ++c)
#pragma unroll
                for (int v = 0; v < V; ++v) bl |= !(fabs(q.x[c][v]) <= 1.79769313486231570815e308);
            const bool badq = group_any<G>(bl, sub);
            if (live) {
                if (!EVAL && badq && gl == 0) raise_status(A.status, ST_BAD_COORD);
#pragma unroll
                for (int c = 0; c < CH; ++c)
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const int d = (c * G + gl) * V + v;
                        if (d < D) stage[(size_t)r * DS + d] = q.x[c][v];
                    }
                if (gl == 0) {
                    sfac[r] = factor;
                    sflag[r] = badq ? 1 : 0;
                }
            }
        }
        __syncthreads();
        // -------- 2. a wave a row: base by lane 0, the data over 64 lanes, the tree, the decision by lane 0 --------
        for (int r = wib; r < nrow; r += T / 64) {       // wave-uniform: every lane of the wave is active throughout
            const bool bad = sflag[r] != 0;              // the same value in every lane
            const double* const x = stage + (size_t)r * DS;
            int my_i = 0;
            double my_lpo = 0.0, my_logu = 0.0, b = -__builtin_inf();
            if (lane == 0) {
                const int pos = A.pos0 + t0 + r;
                my_i = A.order[pos];
                if constexpr (!EVAL) {
                    my_lpo = A.lp[my_i];
                    my_logu = A.logu[pos];
                }
                if (!bad) b = USER{}.base(x, D, user);
            }
            const double base = wave_first(b);            // emx_kernels.hpp
            const bool go = !bad && base == base && base != -__builtin_inf();      // the same value in every lane
            double part = 0.0;
            if (go)
                for (long long k = lane; k < ndata; k += 64) part = part + USER{}.term(x, D, k, user);
            const double S = group_sum<64>(part);        // the whole wave, reconverged: outside the strided loop and every lane branch
            if (lane == 0) {
                if constexpr (EVAL) {
                    double lpn = -__builtin_inf();       // a non-finite row: rejected by whoever compares against it
                    if (!bad) {
                        lpn = go ? base + S : base;
                        if (lpn != lpn) raise_status(A.status, ST_NAN_LOGP);
                    }
                    A.lp[my_i] = lpn;
                } else {
                    bool accept = false;
                    double lpn = my_lpo;
                    if (!bad) {
                        lpn = go ? base + S : base;
                        if (lpn != lpn) raise_status(A.status, ST_NAN_LOGP);                 // ensemble.py:550-551
                        const double lnpdiff = sfac[r] + lpn - my_lpo;                       // red_blue.py:99
                        accept = lnpdiff > my_logu;                                          // red_blue.py:100
                    }
                    if (accept) A.lp[my_i] = lpn;                                            // move.py:34
                    A.acc[my_i] = accept ? 1 : 0;
                    if (A.chain_lp) {
                        A.chain_lp[my_i] = accept ? lpn : my_lpo;
                        if (accept) A.acc_count[my_i] += 1u;
                    }
                    sflag[r] = accept ? 2 : 0;
                }
            }
        }
        __syncthreads();
        // -------- 3. commit, G lanes a row (k_halfstep_user's) --------
        if constexpr (!EVAL) {
#pragma unroll
            for (int p = 0; p < NPASS; ++p) {
                const int r = p * GPB + wib * WPW + sub;
                if (r >= nrow) continue;
                const bool accept = sflag[r] == 2;
                if (!accept && !A.chain) continue;
                Row<G, V, CH> rr = xi[p];
                if (accept) {
#pragma unroll
                    for (int c = 0; c < CH; ++c)
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            const int d = (c * G + gl) * V + v;
                            rr.x[c][v] = d < D ? stage[(size_t)r * DS + d] : 0.0;
                        }
                    store_row<G, V, CH>(rr, A.X + (size_t)wi[p] * D, D, gl);
                }
                if (A.chain) store_row_stream<G, V, CH>(rr, A.chain + (size_t)wi[p] * D, D, gl);
            }
            __syncthreads();                        // the staged rows are consumed before the next tile overwrites them
        }
    }
}

// the launcher behind EMX_FUSED_ENSEMBLE_DATA_TARGET (include/emx.h: emx_fused_ensemble_data_launch): fused_ens_launch_checks'
// answers (emx_fused_ensemble.hpp), then one launch with the descriptor's rows a workgroup: 0, or 100 + a hipError_t.
template <typename USER, int NDIM>
int fused_ensemble_data_launch(const emx_fused_ensemble_data_launch* L) {
    constexpr int G = fused_ens_g(NDIM), V = fused_ens_v(NDIM), CH = fused_ens_ch(NDIM), TILE = fused_ens_tile_rule(NDIM);
    static_assert(G * V * CH >= NDIM, "the row layout covers the row");
    static_assert(fused_ens_lds_of(NDIM, TILE) <= 48 * 1024, "the staging area stays below the LDS a kernel gets without asking");
    int grid;
    if (const int rc = fused_ens_launch_checks<NDIM, 0>(L, EMX_FUSED_ENSEMBLE_DATA_ABI, &grid); rc || !grid) return rc;
    const HalfStepArgs& a = *static_cast<const HalfStepArgs*>(L->args);
    const hipError_t e = fused_ens_with_move(L->move, [&](auto move) {
        hipLaunchKernelGGL((k_halfstep_user_data<G, V, CH, decltype(move)::value, USER, TILE>), dim3(grid), dim3(FUSED_ENS_THREADS),
                           fused_ens_lds_of(NDIM, L->rows), (hipStream_t)L->hip_stream, a, L->user, (long long)L->ndata, L->rows);
        return hipGetLastError();
    });
    return e == hipSuccess ? 0 : 100 + (int)e;
}

}  // namespace emx

#define EMX_FUSED_ENSEMBLE_DATA_TARGET(name, Model, ndim)                                                        \
    extern "C" __attribute__((visibility("default"))) int name(const emx_fused_ensemble_data_launch* launch) {  \
        return emx::fused_ensemble_data_launch<Model, (ndim)>(launch);                                           \
    }
