// Parallel tempering on a batch handle (emx_pt_* in include/emx.h; emcee_amd.PTSampler): members grouped in runs of `ntemps`,
// member g ntemps + t being rung t of group g.  The swap pass's draws (device and host twins) and the kernels' arguments.
#pragma once
#include <cstdint>

#include "emx_planlog.hpp"
#include "emx_rng.hpp"

namespace emx {

// Swap draws of pair i (rung i against rung i - 1, i = 1 ... ntemps - 1) after Philox step `step`, keyed by the group's rung-0
// seed: the pairing pi_i, a keyed bijection of [0, nwalkers) of its own tag (never the split permutation 'PERM' of that step),
// and the uniform of walker k of rung i, u53 of the words (step lo, step hi, 'SWAP', (i - 1) nwalkers + k).
constexpr uint32_t PT_PERM_TAG = 0x5357504du;    // 'SWPM'
constexpr uint32_t PT_SWAP_TAG = 0x53574150u;    // 'SWAP'

EMX_HD PermKey pt_perm_key(uint64_t n, uint64_t seed, uint64_t step, int pair) {
    return make_perm_key_tagged(n, seed, step, PT_PERM_TAG, 2u * (uint32_t)(pair - 1));
}

EMX_HD double pt_swap_uniform(uint64_t seed, uint64_t step, int pair, uint32_t k, uint32_t n) {
    const Philox4 r = philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), PT_SWAP_TAG, (uint32_t)(pair - 1) * n + k, (uint32_t)seed,
                                    (uint32_t)(seed >> 32));
    return u53(r.v[0], r.v[1]);
}

// the tempered log-probability beta L + P: two IEEE operations (the library is built with -ffp-contract=off), P alone at beta 0
// (no 0 * -inf), -inf wherever the prior is -inf whatever L is
EMX_HD double pt_tempered(double beta, double L, double P) {
    if (P == -__builtin_inf()) return P;
    if (beta == 0.0) return P;
    const double bl = beta * L;
    return bl + P;
}

struct PtSwapArgs {
    double* X;                 // (B, N, D)
    double* lp;                // (B, N)
    double* L;                 // (B, N)
    double* P;                 // (B, N)
    const double* beta;        // (B): member m's rung's beta
    const unsigned long long* seeds;      // (B): the group's draws use its rung-0 member's seed
    unsigned long long* attempts;         // (B / ntemps, ntemps - 1)
    unsigned long long* accepts;
    double* chain;             // (B, cap, N, D)
    double* chain_lp;          // (B, cap, N)
    double* chain_L;           // (B, cap, N)
    long long cap;
    long long chain_row;       // -1: not a stored step
    int32_t swap;              // 0: only write the stored rows
    int32_t T, N, D;
    unsigned long long step;
};

// one swap pass (and / or the stored rows) of every group: one workgroup a group
hipError_t pt_swap_launch(int groups, hipStream_t st, const PtSwapArgs& a);
// the initial state of a tempered batch: L := -inf where P is -inf (the box evaluated here when box_lo), lp := pt_tempered, and
// ST_NAN_LOGP where L is NaN with P > -inf or lp is NaN
hipError_t pt_init_launch(const double* X, double* lp, double* L, double* P, const double* beta, const double* box_lo,
                          const double* box_hi, uint32_t* status, int32_t B, int32_t N, int32_t D, hipStream_t st);
// out[m] = mean of chain_L rows start, start + stride, ... < stop of member m over every walker
hipError_t pt_mean_launch(const double* chain_L, long long cap, int32_t B, int32_t N, long long start, long long stop,
                          long long stride, double* out, hipStream_t st);

}  // namespace emx
