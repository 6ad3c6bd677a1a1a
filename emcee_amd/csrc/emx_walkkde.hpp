// WalkMove / KDEMove proposals (emx_walkkde.hip): the arguments of one half-step and the launch, for emx.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace emx {

constexpr int WK_MAX_D = 128;       // ndim bound of both moves on the device (the factor's D x D matrix lives in LDS)
constexpr int WK_MAX_S = 1024;      // WalkMove(s): helper walkers per update on the device (a wave's LDS list)
constexpr int WK_LSE_MAXCH = 64;    // data-row chunks of the KDE log-sum-exp

struct WalkKdeArgs {
    const double* X;          // (N, D) ensemble: the complement is read, nothing is written
    const int32_t* order;     // the step's plan order: slot t of the split is walker order[pos0 + t]
    double* qout;             // (ns, D) proposals in slot order
    double* fout;             // (ns) log proposal ratios
    uint32_t* status;
    double* work;             // walk_kde_work_bytes(N, D)
    uint64_t seed, step;
    int32_t N, D, pos0, ns, t_lo, t_hi;
    int32_t kind;             // MOVE_WALK | MOVE_KDE
    int32_t s;                // walk: helpers per update, 0 = the whole complement
    int32_t bw_rule;          // KDE: 0 Scott, 1 Silverman, 2 scalar `bw`
    double bw;
};

size_t walk_kde_work_bytes(int64_t N, int D);
int walk_kde_lse_chunks(int64_t N, int64_t ns);
hipError_t launch_walk_kde(const WalkKdeArgs& a, hipStream_t st);

}  // namespace emx
