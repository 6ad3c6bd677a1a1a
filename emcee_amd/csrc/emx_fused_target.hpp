// Fused user targets of a batch of small ensembles (include/emx.h: emx_set_batch_target_fused; emcee_amd.targets.BatchFused /
// compile_fused).  PUBLIC: this is the header a user's translation unit includes to compile their own per-row log-probability
// into the one-workgroup kernel k_small_run (emx_kernels.hpp), and the library includes it for the version constants.
//
//     #include <emx_fused_target.hpp>             // hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -I include -I emcee_amd/csrc
//     struct MyModel {                            // stateless; `user`: the device pointer given to BatchFused, `member`: the index in the batch
//         __device__ double operator()(const double* x, int ndim, int member, const void* user) const;
//     };
//     EMX_FUSED_BATCH_TARGET(my_model, MyModel, /*ndim=*/5)       // emits: extern "C" int my_model(const emx_fused_launch*)
//
// `x` points at `ndim` doubles in LDS.  The call is made once per live row by ONE lane and must depend on nothing but its arguments
// and memory reachable from `user`: no LDS of its own, no barrier, no cross-lane operation (its neighbours hold other rows, or are
// idle).  -inf is legal, NaN raises the reference's error naming the member; a row with a non-finite coordinate is rejected
// without being handed over.  `ndim` is fixed at compile time so that the translation unit carries ONE row layout's kernels:
// by default the single-StretchMove selector and the any-schedule one (every schedule a batch accepts runs under one of them);
// EMX_FUSED_BATCH_TARGET_MOVES takes a mask that narrows that to one.
//
// Blobs -- derived quantities recorded with every sample (EnsembleBatch.get_blobs) -- come from the five-argument form:
//
//     struct MyModel {
//         __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const;
//     };
//     EMX_FUSED_BATCH_TARGET_BLOBS(my_model, MyModel, /*ndim=*/5, /*nblobs=*/2)
//
// The call writes blobs[0 ... nblobs) (lane-private, zero on entry; 1 <= nblobs <= 32, any value is legal, NaN included) and
// returns the log-probability as before.  The kernel keeps every walker's blobs in LDS, replaces them exactly when it accepts
// the row, and stores them next to the chain.  Coordinates, log-probs and accept counts are those of the same function without blobs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#if __has_include(<emx.h>)
#include <emx.h>
#else
#include "../../include/emx.h"
#endif
#include "emx_small_launch.hpp"

// bumped with ANY change of SmallRunArgs or of k_small_run's LDS layout: a launcher and a library of different values refuse each other
#ifndef EMX_FUSED_ABI
#define EMX_FUSED_ABI 3u
#endif

#define EMX_FUSED_MOVES_STRETCH 1      // the schedule is one StretchMove
#define EMX_FUSED_MOVES_ANY 2          // any schedule (stretch, DE, snooker, Gaussian moves; a single StretchMove too)

namespace emx {

// pick_shape (emx_small_host.hpp) of an element-wise target, as a constant expression
constexpr int fused_v(int D) { return D % 2 == 0 ? 2 : 1; }
constexpr int fused_g(int D) { return shape_g((D + fused_v(D) - 1) / fused_v(D)); }
constexpr int fused_ch(int D) { return shape_ch((D + fused_v(D) - 1) / fused_v(D)); }

// DATA: the wave-a-row form of a model with base and term (emx_fused_target_data.hpp)
template <typename USER, int NDIM, int MOVESEL, int NBLOBS = 0, bool DATA = false>
hipError_t launch_fused_move(int grid, int threads, size_t lds, hipStream_t st, const SmallRunArgs& a) {
    constexpr int G = fused_g(NDIM), V = fused_v(NDIM), CH = fused_ch(NDIM);
    auto kern = k_small_run<G, V, CH, MOVESEL, false, 0, true, USER, NBLOBS, DATA>;
    static size_t lds_granted[MAX_DEVICES] = {};      // as launch_small_move: function attributes are per device
    int dev = 0;
    if (lds > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MAX_DEVICES && lds > lds_granted[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        lds_granted[dev] = lds;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, a);
    return hipGetLastError();
}

// the launcher behind EMX_FUSED_BATCH_TARGET: the checks, then one launch of the batch (include/emx.h: emx_fused_launch)
template <typename USER, int NDIM, int MOVES, int NBLOBS = 0>
int fused_batch_launch(const emx_fused_launch* L) {
    static_assert(NDIM >= 1 && NDIM <= 256, "a fused user target has 1 <= ndim <= 256");
    static_assert(NBLOBS >= 0 && NBLOBS <= 32, "a fused user target has 0 <= nblobs <= 32");
    static_assert((MOVES & (EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY)) != 0, "no move selector compiled in");
    if (!L || L->abi != EMX_FUSED_ABI || L->args_bytes != (uint32_t)sizeof(SmallRunArgs)) return 1;
    if (L->ndim != NDIM) return 2;
    const bool stretch = L->movesel == MOVE_STRETCH;
    if (!stretch && L->movesel != SMALL_ANY_MOVE) return 3;
    if (!stretch && !(MOVES & EMX_FUSED_MOVES_ANY)) return 3;
    // the blob count against the one compiled in.  (A blob-free launcher reads the field only of a descriptor that carries `args`,
    // as the library's always does: a bare probe of the four fields above is answered from them alone.)
    if ((NBLOBS > 0 || L->args) && L->nblobs != NBLOBS) return 4;
    if (L->grid == 0) return 0;                       // the probe of emx_set_batch_target_fused
    if (!L->args || L->grid < 0 || L->threads < 64 || L->threads > 1024 || L->threads % 64 != 0) return 3;
    SmallRunArgs a = *static_cast<const SmallRunArgs*>(L->args);
    if (a.D != NDIM) return 2;
    if (a.nblobs != NBLOBS || (NBLOBS > 0 && !a.blobs)) return 4;
    a.user = L->user;
    hipError_t e = hipErrorInvalidValue;
    if constexpr ((MOVES & EMX_FUSED_MOVES_STRETCH) != 0) {
        if (stretch) e = launch_fused_move<USER, NDIM, MOVE_STRETCH, NBLOBS>(L->grid, L->threads, (size_t)L->lds_bytes, (hipStream_t)L->hip_stream, a);
    }
    if constexpr ((MOVES & EMX_FUSED_MOVES_ANY) != 0) {
        if (!stretch || !(MOVES & EMX_FUSED_MOVES_STRETCH))      // the any-schedule kernel runs a single StretchMove to the same bits
            e = launch_fused_move<USER, NDIM, SMALL_ANY_MOVE, NBLOBS>(L->grid, L->threads, (size_t)L->lds_bytes, (hipStream_t)L->hip_stream, a);
    }
    return e == hipSuccess ? 0 : 100 + (int)e;
}

}  // namespace emx

#define EMX_FUSED_BATCH_TARGET_MOVES(name, Functor, ndim, moves)                                   \
    extern "C" __attribute__((visibility("default"))) int name(const emx_fused_launch* launch) {  \
        return emx::fused_batch_launch<Functor, (ndim), (moves)>(launch);                          \
    }
#define EMX_FUSED_BATCH_TARGET(name, Functor, ndim) \
    EMX_FUSED_BATCH_TARGET_MOVES(name, Functor, ndim, EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY)
// the five-argument functor (..., double* blobs) with `nblobs` doubles a sample; both move selectors
#define EMX_FUSED_BATCH_TARGET_BLOBS(name, Functor, ndim, nblobs)                                                        \
    extern "C" __attribute__((visibility("default"))) int name(const emx_fused_launch* launch) {                        \
        static_assert((nblobs) >= 1, "EMX_FUSED_BATCH_TARGET_BLOBS: 1 <= nblobs <= 32 (none: EMX_FUSED_BATCH_TARGET)");  \
        return emx::fused_batch_launch<Functor, (ndim), EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY, (nblobs)>(launch); \
    }
