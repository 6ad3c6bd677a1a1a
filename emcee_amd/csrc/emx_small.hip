// Second translation unit of libemx: every single-ensemble instantiation of emx::k_small_run (one workgroup runs whole
// emx_run calls of a small ensemble; emx_kernels.hpp) and its launch dispatch (emx_small_launch.hpp).  Split from emx.hip only
// so that the two halves of the template instantiation work compile in parallel.
#include <hip/hip_runtime.h>

#include "emx_small_launch.hpp"

using namespace emx;

// (declared inside emx.hip's extern "C" region: same unmangled name here; it is not part of the public ABI)
extern "C" hipError_t emx_small_dispatch(int G, int V, int CH, int dpb, int movesel, int threads, size_t lds, hipStream_t st,
                                         const SmallRunArgs& a) {
    return small_dispatch<false>(G, V, CH, dpb, movesel, 1, threads, lds, st, a);
}
