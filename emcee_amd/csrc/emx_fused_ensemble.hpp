// Fused user targets of the single sampler (include/emx.h: emx_set_target_fused; emcee_amd.targets.DeviceFused /
// compile_fused_ensemble).  PUBLIC: this is the header a user's translation unit includes to compile their own per-row
// log-probability into the half-step of a large ensemble, and the library includes it for the version constants and the launch rules.
//
//     #include <emx_fused_ensemble.hpp>           // hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -I include -I emcee_amd/csrc
//     struct MyModel {                            // stateless; `user`: the device pointer given to DeviceFused; `member` is always 0
//         __device__ double operator()(const double* x, int ndim, int member, const void* user) const;
//     };
//     EMX_FUSED_ENSEMBLE_TARGET(my_model, MyModel, /*ndim=*/5)    // emits: extern "C" int my_model(const emx_fused_ensemble_launch*)
//
// The functor contract is the batch one (emx_fused_target.hpp), so one model source serves both: `x` points at `ndim` doubles in
// LDS, the call is made once per live row by ONE lane and depends on nothing but its arguments and memory reachable from `user`
// (no LDS of its own, no barrier, no cross-lane operation).  -inf is legal, NaN raises the reference's error; a row with a
// non-finite coordinate is rejected without being handed over.
//
// k_halfstep_user is ONE launch per half-step where a DeviceKernel target takes three (propose -> the caller's kernel -> commit,
// the proposal block going through HBM twice): a workgroup takes tiles of TILE slots of the split,
//   1. G lanes a row make the proposal -- k_halfstep's arithmetic in pick_shape's row layout (load_row / make_proposal /
//      gauss_disp_row: the same bits, group reductions included) -- and stage it in LDS, rows D | 1 doubles apart;
//   2. one lane a row calls the functor on its staged row and takes the decision (k_wide_commit's rule): lp, acc, acc_count,
//      chain_lp, the NaN status bit;
//   3. G lanes a row commit the accepted rows from LDS to X and append the chain row of a stored step (streaming stores).
// The MOVE_EVAL instantiation is phases 1 and 2 over rows of X (initial log-probs; the log-prob pass of WalkMove / KDEMove).
//
// Blobs (derived quantities kept next to the chain).  The batch contract's five-argument form serves here too:
//     struct MyModel { __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const; };
//     EMX_FUSED_ENSEMBLE_TARGET_BLOBS(my_model, MyModel, /*ndim=*/5, /*nblobs=*/2)     // int my_model(const emx_fused_ensemble_blobs_launch*)
// The call writes blobs[0 ... nblobs) (lane-private, zero on entry; 1 <= nblobs <= 32; any value is legal, NaN included).
// The same kernel with NB > 0 is the same half-step: the decision lane commits the blobs to the walkers' current ones where it
// commits lp and appends the blob plane's row where it appends chain_lp -- a rejected row keeps its previous blobs -- so the blobs
// cost no launch and no second pass over the proposal block.  Both launchers instantiate the one text, k_halfstep_user<..., NB>.
//
// Small ensembles (opt-in; include/emx.h: emx_set_target_fused_small).  An ensemble that fits one workgroup's LDS runs whole
// run_mcmc calls inside k_small_run (emx_kernels.hpp) when the translation unit ALSO emits
//     EMX_FUSED_ENSEMBLE_SMALL_TARGET(my_model_small, MyModel, /*ndim=*/5)              // int my_model_small(const emx_fused_launch*)
//     EMX_FUSED_ENSEMBLE_SMALL_TARGET_BLOBS(my_model_small, MyModel, /*ndim=*/5, /*nblobs=*/2)
// next to the half-step launcher above (which keeps the initial log-probs, every evaluation of rows and the ensembles that do not
// fit).  The launcher carries k_small_run<..., BATCH = false, USER> for the single-StretchMove and the any-schedule selectors, each
// with Philox plans and with the plans of the host's MT19937 twin: four kernels, which is why the macro is a second one -- a
// translation unit without it compiles to what it always did.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#if __has_include(<emx.h>)
#include <emx.h>
#else
#include "../../include/emx.h"
#endif
#include "emx_kernels.hpp"
#include "emx_small_host.hpp"

// bumped with ANY change of HalfStepArgs or of k_halfstep_user's launch rules: a launcher and a library of different values refuse
// each other
#ifndef EMX_FUSED_ENSEMBLE_ABI
#define EMX_FUSED_ENSEMBLE_ABI 0x454e5301u
#endif
// the same for emx_fused_ensemble_blobs_launch and k_halfstep_user with NB > 0: a value of its own, so that a blob launcher handed the
// blob-free descriptor, and a blob-free launcher handed the blob descriptor, answer 1
#ifndef EMX_FUSED_ENSEMBLE_BLOBS_ABI
#define EMX_FUSED_ENSEMBLE_BLOBS_ABI 0x454e4201u
#endif
// the small launcher's descriptor is emx_fused_launch with this constant, bumped -- like EMX_FUSED_ABI of emx_fused_target.hpp -- with
// ANY change of SmallRunArgs or of k_small_run's LDS layout.  A value of its own, so that a batch launcher (EMX_FUSED_BATCH_TARGET: the
// BATCH kernel, which reads per-member arrays a single ensemble has none of) and a small launcher answer 1 to each other's descriptor
#ifndef EMX_FUSED_ENSEMBLE_SMALL_ABI
#define EMX_FUSED_ENSEMBLE_SMALL_ABI 0x45535302u
#endif

namespace emx {

constexpr int FUSED_ENS_MAX_NDIM = 256;
constexpr int FUSED_ENS_THREADS = 256;      // four waves: (256 / G) rows a pass
constexpr int FUSED_ENS_MAX_BLOBS = 32;     // float64 blobs a sample (emcee_amd._lib.MAX_BLOBS)
constexpr int FUSED_ENS_MAX_DEVICES = 64;   // devices one process may drive (the one-workgroup kernel's LDS limit is raised per device)

// pick_shape(D, D) (emx_small_host.hpp) -- the layout of the element-wise k_halfstep -- as a constant expression
constexpr int fused_ens_v(int D) { return D % 2 == 0 ? 2 : 1; }
constexpr int fused_ens_g(int D) { return shape_g((D + fused_ens_v(D) - 1) / fused_ens_v(D)); }
constexpr int fused_ens_ch(int D) { return shape_ch((D + fused_ens_v(D) - 1) / fused_ens_v(D)); }

// Slots a workgroup stages at once (profiles/ensemble_fused.md): as many as keep the staging area near 33 KB, so that four
// workgroups share a CU's 160 KB; never fewer than one pass of the workgroup's groups.
constexpr int fused_ens_tile_rule(int D) { return D <= 64 ? 64 : D <= 128 ? 32 : 16; }
// dynamic LDS of a workgroup: the staged rows, a factor a row, a flag a row (1: non-finite proposal, 2: accepted)
constexpr size_t fused_ens_lds_of(int D, int tile) { return ((size_t)tile * ((size_t)(D | 1) * 8 + 8 + 4) + 15) / 16 * 16; }
constexpr size_t fused_ens_lds_bytes(int D) { return fused_ens_lds_of(D, fused_ens_tile_rule(D)); }
// The launch rules of a target with NB blobs a sample.  The decision lane keeps its NB doubles in registers (a private array), not
// in LDS -- at ndim 64 the staging area's 34 048 B and 64 x 32 doubles more would pass 48 KB -- so tile and LDS do not depend on NB
// (profiles/ensemble_fused_blobs.md has the registers this costs); the functions exist so that rule and check have one place.
constexpr int fused_ens_blobs_tile_rule(int D, int /*NB*/) { return fused_ens_tile_rule(D); }
constexpr size_t fused_ens_blobs_lds_bytes(int D, int NB) { return fused_ens_lds_of(D, fused_ens_blobs_tile_rule(D, NB)); }
// the fewest slots a workgroup of a data target (emx_fused_ensemble_data.hpp) takes: a row a wave
constexpr int FUSED_ENS_DATA_MIN_ROWS = FUSED_ENS_THREADS / 64;

// The half-step of both launchers, ONE text: NB = 0 is the blob-free target (EMX_FUSED_ENSEMBLE_TARGET; cur and plane_row null and
// unused -- the instantiation compiles to the instructions the blob-free copy of this text compiled to before the two were folded,
// profiles/ensemble_fused_shared_text.md), NB > 0 the functor's five-argument form (EMX_FUSED_ENSEMBLE_TARGET_BLOBS).  The decision
// lane holds its NB blobs in registers (a private array: the staging area, and with it every launch rule, is that of NB = 0),
// commits them to `cur` (N, NB; the walkers' current blobs) where it commits lp, and appends `plane_row` (N, NB; the blob plane's
// row of a stored step, or null) where it appends chain_lp.  All blob code sits under if constexpr (NB > 0).
template <int G, int V, int CH, int MOVE, typename USER, int TILE, int NB>
static __global__ __launch_bounds__(FUSED_ENS_THREADS) void k_halfstep_user(const HalfStepArgs A, const void* user, double* __restrict__ cur,
                                                                            double* __restrict__ plane_row) {
    static_assert(NB >= 0 && NB <= FUSED_ENS_MAX_BLOBS, "0 <= nblobs <= 32");
    static_assert(G >= 4 && G <= 64 && (64 % G) == 0, "G lanes per walker");
    constexpr int T = FUSED_ENS_THREADS;
    constexpr int WPW = 64 / G;                 // rows a wave and pass
    constexpr int GPB = (T / 64) * WPW;         // rows a workgroup and pass
    static_assert(TILE >= GPB && TILE % GPB == 0 && TILE <= T, "the tile is whole passes of the workgroup, a lane a row in the decision");
    constexpr int NPASS = TILE / GPB;
    constexpr int NR = rows_per_pass<MOVE>();
    constexpr bool EVAL = MOVE == MOVE_EVAL;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int D = A.D, DS = D | 1;              // odd row stride: the decision lanes' reads of column d hit distinct banks
    double* const stage = smem;
    double* const sfac = stage + (size_t)TILE * DS;
    int* const sflag = reinterpret_cast<int*>(sfac + TILE);
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    const int sub = lane / G, gl = lane % G;

    for (int t0 = A.t_lo + (int)blockIdx.x * TILE; t0 < A.t_hi; t0 += (int)gridDim.x * TILE) {      // workgroup-uniform
        const int nrow = min(TILE, A.t_hi - t0);
        // the decision lane's scalars: independent of the proposals, in flight while they are made
        int my_i = 0;
        double my_lpo = 0.0, my_logu = 0.0;
        if (tid < nrow) {
            const int pos = A.pos0 + t0 + tid;
            my_i = A.order[pos];
            if constexpr (!EVAL) {
                my_lpo = A.lp[my_i];
                my_logu = A.logu[pos];
            }
        }
        // -------- 1. proposals, G lanes a row --------
        int wi[NPASS], ja[NPASS], jb[NR >= 3 ? NPASS : 1], jc[NR >= 4 ? NPASS : 1];
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
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
                if (!EVAL && badq && gl == 0) raise_status(A.status, ST_BAD_COORD);      // (an evaluated block's was raised by the kernel that proposed it)
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
        // -------- 2. the functor and the decision, one lane a row (red_blue.py:96-101, as k_wide_commit) --------
        if (tid < nrow) {
            const bool bad = sflag[tid] != 0;
            if constexpr (EVAL) {
                double lpn = -__builtin_inf();      // a non-finite row: rejected by whoever compares against it
                if (!bad) {
                    if constexpr (NB > 0) {
                        double b[NB] = {};
                        lpn = USER{}(stage + (size_t)tid * DS, D, 0, user, b);
#pragma unroll
                        for (int k = 0; k < NB; ++k) cur[(size_t)my_i * NB + k] = b[k];      // with lp, below
                    } else {
                        lpn = USER{}(stage + (size_t)tid * DS, D, 0, user);
                    }
                    if (lpn != lpn) raise_status(A.status, ST_NAN_LOGP);
                }
                A.lp[my_i] = lpn;
            } else {
                bool accept = false;
                double lpn = my_lpo;
                [[maybe_unused]] double b[NB > 0 ? NB : 1];
                if (!bad) {
                    if constexpr (NB > 0) {
#pragma unroll
                        for (int k = 0; k < NB; ++k) b[k] = 0.0;
                        lpn = USER{}(stage + (size_t)tid * DS, D, 0, user, b);
                    } else {
                        lpn = USER{}(stage + (size_t)tid * DS, D, 0, user);
                    }
                    if (lpn != lpn) raise_status(A.status, ST_NAN_LOGP);                 // ensemble.py:550-551
                    const double lnpdiff = sfac[tid] + lpn - my_lpo;                     // red_blue.py:99
                    accept = lnpdiff > my_logu;                                          // red_blue.py:100
                }
                if (accept) A.lp[my_i] = lpn;                                            // move.py:34
                A.acc[my_i] = accept ? 1 : 0;
                if (A.chain_lp) {
                    A.chain_lp[my_i] = accept ? lpn : my_lpo;
                    if (accept) A.acc_count[my_i] += 1u;
                }
                if constexpr (NB > 0) {
                    // the blobs go where lp goes: a rejected row (a non-finite proposal and a -inf factor among them) keeps the
                    // walker's previous ones, and a stored step appends whichever the walker now has
                    double* const mine = cur + (size_t)my_i * NB;
                    if (accept) {
#pragma unroll
                        for (int k = 0; k < NB; ++k) mine[k] = b[k];
                    }
                    if (plane_row) {
                        if (!accept) {
#pragma unroll
                            for (int k = 0; k < NB; ++k) b[k] = mine[k];
                        }
#pragma unroll
                        for (int k = 0; k < NB; ++k) __builtin_nontemporal_store(b[k], plane_row + (size_t)my_i * NB + k);
                    }
                }
                sflag[tid] = accept ? 2 : 0;
            }
        }
        __syncthreads();
        // -------- 3. commit, G lanes a row: accepted rows from LDS (move.py:33), the chain row of a stored step --------
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

// ---- the launchers ----

// the run-time move as a compile-time one: f(std::integral_constant<int, MOVE_...>{}) -> hipError_t
template <typename F>
hipError_t fused_ens_with_move(const int move, F&& f) {
    switch (move) {
        case MOVE_STRETCH: return f(std::integral_constant<int, MOVE_STRETCH>{});
        case MOVE_DE: return f(std::integral_constant<int, MOVE_DE>{});
        case MOVE_SNOOKER: return f(std::integral_constant<int, MOVE_SNOOKER>{});
        case MOVE_GAUSS: return f(std::integral_constant<int, MOVE_GAUSS>{});
        case MOVE_EVAL: return f(std::integral_constant<int, MOVE_EVAL>{});
    }
    return hipErrorInvalidValue;
}

// What the three half-step launchers check before they launch, in the order in which they answer: a descriptor that is wrong in
// two ways gets the answer of the first.  DESC: emx_fused_ensemble_launch, _blobs_launch (NB: its blob count) or _data_launch;
// `abi`: its constant.  -> 0 and *grid workgroups to launch (0: none -- the probe of emx_set_target_fused*, an empty split), or
// non-zero and nothing launched: 1 another version of the header (or another launcher type's descriptor), 2 another ndim, 3 a
// move or launch shape that was not compiled in (rows a workgroup outside 4 ... the tile, data outside [0, 2^31)), 4 another number
// of blobs or no walkers' blob array, 5 a HalfStepArgs that carries an exchange, a graph descriptor or a device-side slot count.
template <int NDIM, int NB, typename DESC>
int fused_ens_launch_checks(const DESC* L, const uint32_t abi, int* const grid) {
    static_assert(NDIM >= 1 && NDIM <= FUSED_ENS_MAX_NDIM, "a fused user target has 1 <= ndim <= 256");
    constexpr bool BLOBS = std::is_same<DESC, emx_fused_ensemble_blobs_launch>::value, DATA = std::is_same<DESC, emx_fused_ensemble_data_launch>::value;
    *grid = 0;
    if (!L || L->abi != abi || L->args_bytes != (uint32_t)sizeof(HalfStepArgs)) return 1;
    if (L->ndim != NDIM) return 2;
    if (L->move != MOVE_STRETCH && L->move != MOVE_DE && L->move != MOVE_SNOOKER && L->move != MOVE_GAUSS && L->move != MOVE_EVAL) return 3;
    if constexpr (BLOBS)
        if (L->nblobs != NB) return 4;
    if (L->grid == 0) return 0;                       // the probe
    int rows = fused_ens_tile_rule(NDIM);             // slots a workgroup: the tile, or what a data launch asks for
    if constexpr (DATA) {
        if (L->rows < FUSED_ENS_DATA_MIN_ROWS || L->rows > rows || L->ndata < 0 || L->ndata >= (1ll << 31)) return 3;
        rows = L->rows;
    }
    if (!L->args || L->grid < 0 || L->threads != FUSED_ENS_THREADS || L->lds_bytes < fused_ens_lds_of(NDIM, rows)) return 3;
    if constexpr (BLOBS)
        if (!L->blobs_cur) return 4;
    const HalfStepArgs& a = *static_cast<const HalfStepArgs*>(L->args);
    if (a.D != NDIM) return 2;
    if (a.sendbuf || a.desc || a.t_hi_dev || a.peers || a.npeer || a.declp || a.push_peers || a.npush) return 5;
    if (a.t_hi <= a.t_lo) return 0;
    // `grid` of the descriptor is the most workgroups the library allows; `rows` slots a workgroup until then
    const long long tiles = ((long long)a.t_hi - a.t_lo + rows - 1) / rows;
    *grid = (int)(tiles < L->grid ? tiles : L->grid);
    return 0;
}

// the launcher behind EMX_FUSED_ENSEMBLE_TARGET (NB = 0; cur, plane_row null) and EMX_FUSED_ENSEMBLE_TARGET_BLOBS (cur, plane_row:
// the descriptor's blob pointers): fused_ens_launch_checks' answers, then one launch: 0, or 100 + a hipError_t
template <typename USER, int NDIM, int NB, typename DESC>
int fused_ens_lane_launch(const DESC* L, const uint32_t abi, double* cur, double* plane_row) {
    constexpr int G = fused_ens_g(NDIM), V = fused_ens_v(NDIM), CH = fused_ens_ch(NDIM), TILE = fused_ens_blobs_tile_rule(NDIM, NB);
    static_assert(G * V * CH >= NDIM, "the row layout covers the row");
    constexpr size_t lds = fused_ens_blobs_lds_bytes(NDIM, NB);
    static_assert(lds <= 48 * 1024, "the staging area stays below the LDS a kernel gets without asking, whatever the blob count");
    int grid;
    if (const int rc = fused_ens_launch_checks<NDIM, NB>(L, abi, &grid); rc || !grid) return rc;
    const hipStream_t st = (hipStream_t)L->hip_stream;
    const HalfStepArgs& a = *static_cast<const HalfStepArgs*>(L->args);
    const hipError_t e = fused_ens_with_move(L->move, [&](auto move) {
        constexpr int MOVE = decltype(move)::value;
        hipLaunchKernelGGL((k_halfstep_user<G, V, CH, MOVE, USER, TILE, NB>), dim3(grid), dim3(FUSED_ENS_THREADS), lds, st, a, L->user, cur,
                           MOVE == MOVE_EVAL ? nullptr : plane_row);      // (an evaluation of rows appends no row of the blob plane)
        return hipGetLastError();
    });
    return e == hipSuccess ? 0 : 100 + (int)e;
}

template <typename USER, int NDIM>
int fused_ensemble_launch(const emx_fused_ensemble_launch* L) {
    return fused_ens_lane_launch<USER, NDIM, 0>(L, EMX_FUSED_ENSEMBLE_ABI, nullptr, nullptr);
}

template <typename USER, int NDIM, int NB>
int fused_ensemble_blobs_launch(const emx_fused_ensemble_blobs_launch* L) {
    static_assert(NB >= 1 && NB <= FUSED_ENS_MAX_BLOBS, "EMX_FUSED_ENSEMBLE_TARGET_BLOBS: 1 <= nblobs <= 32 (none: EMX_FUSED_ENSEMBLE_TARGET)");
    return fused_ens_lane_launch<USER, NDIM, NB>(L, EMX_FUSED_ENSEMBLE_BLOBS_ABI, L ? L->blobs_cur : nullptr, L ? L->blobs_row : nullptr);
}

// ---- small ensembles: the one-workgroup kernel around the same functor ----
template <typename USER, int NDIM, int MOVESEL, bool PLANNED, int NB>
hipError_t launch_fused_ens_small(int threads, size_t lds, hipStream_t st, const SmallRunArgs& a) {
    constexpr int G = fused_ens_g(NDIM), V = fused_ens_v(NDIM), CH = fused_ens_ch(NDIM);
    static_assert(G * V * CH >= NDIM, "the row layout covers the row");
    auto kern = k_small_run<G, V, CH, MOVESEL, PLANNED, 0, false, USER, NB>;
    static size_t lds_granted[FUSED_ENS_MAX_DEVICES] = {};      // as launch_small_move: function attributes are per device
    int dev = 0;
    if (lds > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < FUSED_ENS_MAX_DEVICES && lds > lds_granted[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        lds_granted[dev] = lds;
    }
    hipLaunchKernelGGL(kern, dim3(1), dim3(threads), lds, st, a);
    return hipGetLastError();
}

// the launcher behind EMX_FUSED_ENSEMBLE_SMALL_TARGET[_BLOBS] (include/emx.h: emx_set_target_fused_small).  The descriptor is
// emx_fused_launch: abi EMX_FUSED_ENSEMBLE_SMALL_ABI, args a SmallRunArgs, grid 1 (0: the probe), reserved 1 when the plans are the
// host's (exact MT19937 mode: args carries `plans`), else 0.  0, or non-zero and nothing launched: 1 another version of the headers
// (or another launcher type's descriptor), 2 another ndim, 3 a move selector or a launch shape that was not compiled in -- a
// workgroup, an LDS size or a staging area that does not hold the ensemble among them --, 4 another number of blobs, 100 + a hipError_t.
template <typename USER, int NDIM, int NB>
int fused_ensemble_small_launch(const emx_fused_launch* L) {
    static_assert(NDIM >= 1 && NDIM <= FUSED_ENS_MAX_NDIM, "a fused user target has 1 <= ndim <= 256");
    static_assert(NB >= 0 && NB <= FUSED_ENS_MAX_BLOBS, "a fused user target has 0 <= nblobs <= 32");
    if (!L || L->abi != EMX_FUSED_ENSEMBLE_SMALL_ABI || L->args_bytes != (uint32_t)sizeof(SmallRunArgs)) return 1;
    if (L->ndim != NDIM) return 2;
    const bool stretch = L->movesel == MOVE_STRETCH;
    if ((!stretch && L->movesel != SMALL_ANY_MOVE) || (L->reserved != 0 && L->reserved != 1)) return 3;
    if (L->nblobs != NB) return 4;
    if (L->grid == 0) return 0;                       // the probe of emx_set_target_fused_small
    if (!L->args || L->grid != 1 || L->threads < 64 || L->threads > 1024 || L->threads % 64 != 0) return 3;
    SmallRunArgs a = *static_cast<const SmallRunArgs*>(L->args);
    if (a.D != NDIM) return 2;
    if (a.nblobs != NB || (NB > 0 && !a.blobs)) return 4;
    const bool planned = L->reserved == 1;
    if (planned != (a.plans != nullptr) || (planned && a.nmoves > 1 && !a.step_moves)) return 3;
    // what the kernel keeps in LDS fits what the launch asks for: the ensemble, `batch` steps' plans, a staging row for every slot of
    // the largest split, the blobs
    if (a.N < 2 || a.N > 4096 || a.batch < 1 || a.nmoves < 1 || a.nmoves > SMALL_MAX_MOVES || a.stage_rows < 1) return 3;
    for (int m = 0; m < a.nmoves; ++m) {
        if (a.nsplits[m] < 1 || (a.N + a.nsplits[m] - 1) / a.nsplits[m] > a.stage_rows) return 3;
        if ((a.kind[m] == MOVE_GAUSS && planned) || (stretch && a.kind[m] != MOVE_STRETCH)) return 3;      // (exact mode: the normals are the host's)
    }
    const size_t need = small_lds_bytes(a.N, NDIM, 0, 0, a.batch) + small_fused_stage_bytes(a.stage_rows, NDIM) + small_blob_bytes(a.N, NB);
    if (need > (size_t)L->lds_bytes || (size_t)L->lds_bytes > SMALL_LDS_MAX) return 3;
    a.user = L->user;
    const hipStream_t st = (hipStream_t)L->hip_stream;
    const size_t lds = (size_t)L->lds_bytes;
    hipError_t e;
    if (stretch)
        e = planned ? launch_fused_ens_small<USER, NDIM, MOVE_STRETCH, true, NB>(L->threads, lds, st, a)
                    : launch_fused_ens_small<USER, NDIM, MOVE_STRETCH, false, NB>(L->threads, lds, st, a);
    else
        e = planned ? launch_fused_ens_small<USER, NDIM, SMALL_ANY_MOVE, true, NB>(L->threads, lds, st, a)
                    : launch_fused_ens_small<USER, NDIM, SMALL_ANY_MOVE, false, NB>(L->threads, lds, st, a);
    return e == hipSuccess ? 0 : 100 + (int)e;
}

}  // namespace emx

#define EMX_FUSED_ENSEMBLE_TARGET(name, Functor, ndim)                                                      \
    extern "C" __attribute__((visibility("default"))) int name(const emx_fused_ensemble_launch* launch) {  \
        return emx::fused_ensemble_launch<Functor, (ndim)>(launch);                                         \
    }

// the five-argument functor (..., double* blobs) with `nblobs` doubles a sample
#define EMX_FUSED_ENSEMBLE_TARGET_BLOBS(name, Functor, ndim, nblobs)                                              \
    extern "C" __attribute__((visibility("default"))) int name(const emx_fused_ensemble_blobs_launch* launch) {  \
        return emx::fused_ensemble_blobs_launch<Functor, (ndim), (nblobs)>(launch);                               \
    }

// opt-in, next to one of the two above: the one-workgroup kernel of an ensemble that fits one workgroup's LDS
#define EMX_FUSED_ENSEMBLE_SMALL_TARGET(name, Functor, ndim)                                      \
    extern "C" __attribute__((visibility("default"))) int name(const emx_fused_launch* launch) { \
        return emx::fused_ensemble_small_launch<Functor, (ndim), 0>(launch);                      \
    }
#define EMX_FUSED_ENSEMBLE_SMALL_TARGET_BLOBS(name, Functor, ndim, nblobs)                                                          \
    extern "C" __attribute__((visibility("default"))) int name(const emx_fused_launch* launch) {                                   \
        static_assert((nblobs) >= 1, "EMX_FUSED_ENSEMBLE_SMALL_TARGET_BLOBS: 1 <= nblobs <= 32 (none: EMX_FUSED_ENSEMBLE_SMALL_TARGET)"); \
        return emx::fused_ensemble_small_launch<Functor, (ndim), (nblobs)>(launch);                                                 \
    }
