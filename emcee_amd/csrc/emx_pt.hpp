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

// exp(x) from IEEE + - * / and exponent bits only (no libm / OCML: host and device give the same bits).  x = k ln2 + r with a
// two-part ln2 (k ln2_hi exact), |r| <= ln2 / 2; e^r by its Taylor series to r^13 in Horner form (truncation < 1e-17); the
// result is e^r 2^(k/2) 2^(k - k/2), two exact-or-once-rounded scalings so that subnormal and near-overflow results stay right.
EMX_HD double pt_pow2i(int k) {      // 2^k for -1022 <= k <= 1023
    union {
        double d;
        uint64_t u;
    } v;
    v.u = (uint64_t)(k + 1023) << 52;
    return v.d;
}

EMX_HD double pt_exp(double x) {
    if (x != x) return x;
    if (x > 709.782712893384) return __builtin_inf();
    if (x < -745.2) return 0.0;
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, inv_ln2 = 1.44269504088896338700e+00;
    const double kd = x * inv_ln2;
    const int k = (int)(kd >= 0.0 ? kd + 0.5 : kd - 0.5);
    const double r = (x - (double)k * ln2_hi) - (double)k * ln2_lo;
    double p = 1.0 / 6227020800.0;                   // 1 / 13!
    const double c[13] = {1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0,
                          1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0};
    for (int n = 0; n < 13; ++n) p = p * r + c[n];
    const int k1 = k / 2;
    return p * pt_pow2i(k1) * pt_pow2i(k - k1);
}

// The adaptive ladder (Vousden, Farr & Mandel 2016; ptemcee's _get_ladder_adjustment) of one group after its t-th earlier
// update: acc[j] the accepted swaps of pair j + 1 in this pass out of n, r[j] = acc[j] / n;
//   kappa = (lag / (t + lag)) / time,  dS[j] = kappa (r[j] - r[j + 1]),  dT[j] = (1 / b[j + 1] - 1 / b[j]) pt_exp(dS[j]),
//   c_j = dT[0] + ... + dT[j] (left to right),  b'[j + 1] = 1 / (c_j + 1 / b[0])            j = 0 ... T - 3
// in that operation order.  Rungs 0 and T - 1 stay; out[0] and out[T - 1] are not written; out may be b (b[j + 1] is read
// before out[j + 1] is written).  T <= 2: nothing moves.
template <typename Count>
EMX_HD void pt_adapt_ladder(const double* b, const Count* acc, int T, long long n, double lag, double time, long long t,
                            double* out) {
    if (T <= 2) return;
    const double nd = (double)n;
    const double kappa = (lag / ((double)t + lag)) / time;
    const double inv0 = 1.0 / b[0];
    double inv = inv0, c = 0.0, rj = (double)acc[0] / nd;
    for (int j = 0; j <= T - 3; ++j) {
        const double rn = (double)acc[j + 1] / nd;
        const double dS = kappa * (rj - rn);
        const double invn = 1.0 / b[j + 1];
        const double dT = (invn - inv) * pt_exp(dS);
        c = j == 0 ? dT : c + dT;
        out[j + 1] = 1.0 / (c + inv0);
        inv = invn;
        rj = rn;
    }
}

// ntemps limit of an adaptive ladder (k_pt_swap keeps the group's ladder and pair counts in LDS)
constexpr int PT_ADAPT_MAX_T = 256;

struct PtSwapArgs {
    double* X;                 // (B, N, D)
    double* lp;                // (B, N)
    double* L;                 // (B, N)
    double* P;                 // (B, N)
    double* beta;              // (B): member m's rung's beta (moved by adaptation)
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
    double* chain_beta;        // (B, cap): each stored row's beta
    // adaptation (emx_pt_set_adaptation): after the pass, pt_adapt_ladder on the pass's counts moves rungs 1 ... T - 2 of every
    // group (in beta) and their lp; 0: the pass as without adaptation
    int32_t adapt;
    double lag, time;
    long long adapt_t;         // the update counter t before this pass
    // blobs of a target that has them (nblobs 0: none, the pass as without them): a blob belongs to the point, so an accepted pair
    // exchanges the K doubles of its two rows with x, and a stored step writes every rung's rows of the plane
    double* blobs;             // (B, N, nblobs)
    double* chain_blobs;       // (B, cap, N, nblobs)
    int32_t nblobs;
};

// one swap pass (and / or the stored rows) of every group: one workgroup a group
hipError_t pt_swap_launch(int groups, hipStream_t st, const PtSwapArgs& a);
// the initial state of a tempered batch: L := -inf where P is -inf (the box evaluated here when box_lo), lp := pt_tempered, and
// ST_NAN_LOGP where L is NaN with P > -inf or lp is NaN; blobs (B, N, nblobs; nullptr / 0: none) := NaN where P is -inf
hipError_t pt_init_launch(const double* X, double* lp, double* L, double* P, const double* beta, const double* box_lo,
                          const double* box_hi, uint32_t* status, int32_t B, int32_t N, int32_t D, hipStream_t st,
                          double* blobs = nullptr, int32_t nblobs = 0);
// lp := pt_tempered(beta[m], L, P) of every walker of every member (emx_pt_set_ladder)
hipError_t pt_relp_launch(double* lp, const double* L, const double* P, const double* beta, int32_t B, int32_t N, hipStream_t st);
// out[m] = mean of chain_L rows start, start + stride, ... < stop of member m over every walker
hipError_t pt_mean_launch(const double* chain_L, long long cap, int32_t B, int32_t N, long long start, long long stop,
                          long long stride, double* out, hipStream_t st);

}  // namespace emx
