// The launches of emx::k_small_run (emx_kernels.hpp): the template instantiations for every row layout and move selector,
// and their dispatch.  Included by emx_small.hip (single-ensemble launches, one workgroup) and emx_batch.hip (batched
// launches, one workgroup a member), so that the two instantiation sets compile in parallel.
#pragma once
#include <hip/hip_runtime.h>

#include "emx_kernels.hpp"
#include "emx_small_host.hpp"

namespace emx {

constexpr int MAX_DEVICES = 64;      // function attributes are per device: one process may drive several GPUs


template <bool BATCH, int G, int V, int CH, int MOVESEL, bool PLANNED, int DPB = 0>
hipError_t launch_small_move(int grid, int threads, size_t lds, hipStream_t st, const SmallRunArgs& a) {
    if constexpr (BATCH && PLANNED) return hipErrorInvalidValue;     // batches run in Philox mode only
    auto kern = k_small_run<G, V, CH, MOVESEL, PLANNED, DPB, BATCH>;
    static size_t lds_granted[MAX_DEVICES] = {};
    int dev = 0;
    if (lds > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MAX_DEVICES && lds > lds_granted[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        lds_granted[dev] = lds;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, a);
    return hipGetLastError();
}

template <bool BATCH, int G, int V, int CH>
hipError_t launch_small(int move, int grid, int threads, size_t lds, hipStream_t st, const SmallRunArgs& a) {
    const bool planned = a.plans != nullptr;
    switch (move) {
        case MOVE_STRETCH:
            return planned ? launch_small_move<BATCH, G, V, CH, MOVE_STRETCH, true>(grid, threads, lds, st, a)
                           : launch_small_move<BATCH, G, V, CH, MOVE_STRETCH, false>(grid, threads, lds, st, a);
        case MOVE_DE:
            return planned ? launch_small_move<BATCH, G, V, CH, MOVE_DE, true>(grid, threads, lds, st, a)
                           : launch_small_move<BATCH, G, V, CH, MOVE_DE, false>(grid, threads, lds, st, a);
        case MOVE_SNOOKER:
            return planned ? launch_small_move<BATCH, G, V, CH, MOVE_SNOOKER, true>(grid, threads, lds, st, a)
                           : launch_small_move<BATCH, G, V, CH, MOVE_SNOOKER, false>(grid, threads, lds, st, a);
        case MOVE_GAUSS:       // native mode only: the exact mode's normals come from the host
            return planned ? hipErrorInvalidValue : launch_small_move<BATCH, G, V, CH, MOVE_GAUSS, false>(grid, threads, lds, st, a);
        case SMALL_ANY_MOVE:
            return planned ? launch_small_move<BATCH, G, V, CH, SMALL_ANY_MOVE, true>(grid, threads, lds, st, a)
                           : launch_small_move<BATCH, G, V, CH, SMALL_ANY_MOVE, false>(grid, threads, lds, st, a);
    }
    return hipErrorInvalidValue;
}

// dense target in the one-workgroup kernel: a single stretch move, or any schedule (the kernel then carries all three)
template <bool BATCH, int DPB, int V>
hipError_t launch_small_dense(int move, int grid, int threads, size_t lds, hipStream_t st, const SmallRunArgs& a) {
    constexpr int cols = DPB * 16 / V;
    constexpr int G = shape_g(cols), CH = shape_ch(cols);
    const bool planned = a.plans != nullptr;
    if (move == MOVE_STRETCH)
        return planned ? launch_small_move<BATCH, G, V, CH, MOVE_STRETCH, true, DPB>(grid, threads, lds, st, a)
                       : launch_small_move<BATCH, G, V, CH, MOVE_STRETCH, false, DPB>(grid, threads, lds, st, a);
    return planned ? launch_small_move<BATCH, G, V, CH, SMALL_ANY_MOVE, true, DPB>(grid, threads, lds, st, a)
                   : launch_small_move<BATCH, G, V, CH, SMALL_ANY_MOVE, false, DPB>(grid, threads, lds, st, a);
}

// (G, V, CH): row layout picked by pick_shape (emx_small_host.hpp); dpb > 0: dense Gaussian target with Dp = 16 dpb.  `grid`
// workgroups: 1 for a single ensemble, the batch size for a batched launch (BATCH instantiations)
template <bool BATCH>
hipError_t small_dispatch(int G, int V, int CH, int dpb, int movesel, int grid, int threads, size_t lds, hipStream_t st,
                          const SmallRunArgs& a) {
    hipError_t e = hipErrorInvalidValue;
    if (dpb > 0) {
#define EMX_DCASE(b, v) \
    if (dpb == b && V == v) e = launch_small_dense<BATCH, b, v>(movesel, grid, threads, lds, st, a);
        EMX_DCASE(1, 1) EMX_DCASE(2, 1) EMX_DCASE(3, 1) EMX_DCASE(4, 1) EMX_DCASE(5, 1) EMX_DCASE(6, 1) EMX_DCASE(7, 1)
        EMX_DCASE(1, 2) EMX_DCASE(2, 2) EMX_DCASE(3, 2) EMX_DCASE(4, 2) EMX_DCASE(5, 2) EMX_DCASE(6, 2) EMX_DCASE(7, 2)
#undef EMX_DCASE
    } else {
#define EMX_CASE(g, v, ch) \
    if (G == g && V == v && CH == ch) e = launch_small<BATCH, g, v, ch>(movesel, grid, threads, lds, st, a);
        EMX_CASE(4, 1, 1) EMX_CASE(8, 1, 1) EMX_CASE(8, 1, 2) EMX_CASE(8, 1, 4) EMX_CASE(16, 1, 4) EMX_CASE(32, 1, 4) EMX_CASE(64, 1, 4)
        EMX_CASE(4, 2, 1) EMX_CASE(8, 2, 1) EMX_CASE(8, 2, 2) EMX_CASE(8, 2, 4) EMX_CASE(16, 2, 4) EMX_CASE(32, 2, 4)
#undef EMX_CASE
    }
    return e;
}

}  // namespace emx
