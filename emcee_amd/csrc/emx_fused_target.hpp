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
#include <type_traits>

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

// THE launcher check of every fused batch and tempered target (fused_batch_launch below, fused_batch_data_launch, fused_pt_launch,
// fused_pt_data_launch), in the order that is part of their contract.  `before_probe(L)`: the checks ONE launcher has between the
// selectors and the probe (its answer, or FUSED_GO_ON).  Returns the answer, or FUSED_GO_ON with *stretch: the schedule is one StretchMove.
constexpr int FUSED_GO_ON = -1;
template <typename DESC, typename SITE>
int fused_launch_checks(DESC* L, uint32_t abi, size_t args_bytes, int ndim, int moves, int max_threads, bool* stretch, SITE&& before_probe) {
    if (!L || L->abi != abi || L->args_bytes != (uint32_t)args_bytes) return 1;
    if (L->ndim != ndim) return 2;
    *stretch = L->movesel == MOVE_STRETCH;
    if (!*stretch && L->movesel != SMALL_ANY_MOVE) return 3;
    if (!*stretch && !(moves & EMX_FUSED_MOVES_ANY)) return 3;
    if (const int rc = before_probe(L); rc != FUSED_GO_ON) return rc;
    if (L->grid == 0) return 0;                       // the probe of the library's setters
    if (!L->args || L->grid < 0 || L->threads < 64 || L->threads > max_threads || L->threads % 64 != 0) return 3;
    return FUSED_GO_ON;
}

// `launch(std::integral_constant<int, MOVESEL>)` under the stretch selector, the any selector, or the one of them the MOVES mask
// compiled in (a mask of 0: none), as the launcher's answer: 0, or 100 + hipError_t
template <int MOVES, typename LAUNCH>
int fused_launch_by_moves(bool stretch, LAUNCH&& launch) {
    [[maybe_unused]] hipError_t e = hipErrorInvalidValue;
    if constexpr ((MOVES & EMX_FUSED_MOVES_STRETCH) != 0) {
        if (stretch) e = launch(std::integral_constant<int, MOVE_STRETCH>{});
    }
    if constexpr ((MOVES & EMX_FUSED_MOVES_ANY) != 0) {
        if (!stretch || !(MOVES & EMX_FUSED_MOVES_STRETCH))      // the any-schedule kernel runs a single StretchMove to the same bits
            e = launch(std::integral_constant<int, SMALL_ANY_MOVE>{});
    }
    return e == hipSuccess ? 0 : 100 + (int)e;
}

// grant `kern` its dynamic LDS above 48 KiB once per device, launch it, hipGetLastError.  `lds_granted`: the CALLER's static table
// (MAX_DEVICES entries), one per kernel instantiation -- function attributes are per kernel and device, as launch_small_move's
template <typename KERN, typename ARGS>
hipError_t fused_launch_kernel(KERN kern, size_t* lds_granted, int grid, int threads, size_t lds, hipStream_t st, const ARGS& a) {
    int dev = 0;
    if (lds > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MAX_DEVICES && lds > lds_granted[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        lds_granted[dev] = lds;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, a);
    return hipGetLastError();
}

// DATA: the wave-a-row form of a model with base and term (emx_fused_target_data.hpp)
template <typename USER, int NDIM, int MOVESEL, int NBLOBS = 0, bool DATA = false>
hipError_t launch_fused_move(int grid, int threads, size_t lds, hipStream_t st, const SmallRunArgs& a) {
    static size_t lds_granted[MAX_DEVICES] = {};
    return fused_launch_kernel(k_small_run<fused_g(NDIM), fused_v(NDIM), fused_ch(NDIM), MOVESEL, false, 0, true, USER, NBLOBS, DATA>, lds_granted,
                               grid, threads, lds, st, a);
}

// the launcher behind EMX_FUSED_BATCH_TARGET: the checks, then one launch of the batch (include/emx.h: emx_fused_launch)
template <typename USER, int NDIM, int MOVES, int NBLOBS = 0>
int fused_batch_launch(const emx_fused_launch* L) {
    static_assert(NDIM >= 1 && NDIM <= 256, "a fused user target has 1 <= ndim <= 256");
    static_assert(NBLOBS >= 0 && NBLOBS <= 32, "a fused user target has 0 <= nblobs <= 32");
    static_assert((MOVES & (EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY)) != 0, "no move selector compiled in");
    bool stretch = false;
    // the blob count against the one compiled in.  (A blob-free launcher reads the field only of a descriptor that carries `args`,
    // as the library's always does: a bare probe of the four fields before it is answered from them alone.)
    const int rc = fused_launch_checks(L, EMX_FUSED_ABI, sizeof(SmallRunArgs), NDIM, MOVES, 1024, &stretch, [](const emx_fused_launch* d) {
        return (NBLOBS > 0 || d->args) && d->nblobs != NBLOBS ? 4 : FUSED_GO_ON;
    });
    if (rc != FUSED_GO_ON) return rc;
    SmallRunArgs a = *static_cast<const SmallRunArgs*>(L->args);
    if (a.D != NDIM) return 2;
    if (a.nblobs != NBLOBS || (NBLOBS > 0 && !a.blobs)) return 4;
    a.user = L->user;
    return fused_launch_by_moves<MOVES>(stretch, [&](auto sel) {
        return launch_fused_move<USER, NDIM, decltype(sel)::value, NBLOBS>(L->grid, L->threads, (size_t)L->lds_bytes, (hipStream_t)L->hip_stream, a);
    });
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
