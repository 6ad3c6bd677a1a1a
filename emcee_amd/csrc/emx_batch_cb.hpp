// Batches of independent small ensembles with the caller's batched log-prob (emx_set_batch_target_callback; csrc/emx_batch_cb.hip):
// the arguments of k_batch_cb and its dispatch, shared by the batch handle (emx_batch.hip) and the kernel's translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "emx_kernels.hpp"

namespace emx {

// One launch of k_batch_cb: commit the pending phase (the caller's log-probs of the block it was handed), then propose the
// next one.  Workgroup b is member b; every array is member-strided as in SmallRunArgs.
struct BatchCbArgs {
    double* X;                 // (B, N, D)
    double* lp;                // (B, N)
    uint8_t* acc;              // (B, N)
    uint32_t* acc_count;       // (B, N)
    uint32_t* status;          // (B, SMALL_STATUS_WORDS)
    double* chain;             // (B, cap, N, D) member-major
    double* chain_lp;          // (B, cap, N)
    long long cap;
    double* q;                 // (B, R, D): the block the caller evaluates; rows >= the member's split size are padding
    const double* lpq;         // (B, R): the caller's log-probs of q
    double* fac;               // (B, R) scratch for the commit: factor (-inf: a non-finite proposal), log-uniform, walker
    double* logu;
    int32_t* wi;
    int32_t* nrows;            // (B): real rows of the pending phase
    const unsigned long long* seeds;
    // the move schedule (as SmallRunArgs)
    double a[SMALL_MAX_MOVES], sigma[SMALL_MAX_MOVES], g0[SMALL_MAX_MOVES], gammas[SMALL_MAX_MOVES], cdf[SMALL_MAX_MOVES];
    int32_t kind[SMALL_MAX_MOVES], nsplits[SMALL_MAX_MOVES], gmode[SMALL_MAX_MOVES];
    double gsigma[SMALL_MAX_MOVES];
    const double* gscale[SMALL_MAX_MOVES];
    int32_t nmoves;
    const double* gfac;        // Gaussian moves: the proposal step's factor of member b at gfac[b * gfac_stride] (nullptr: 1)
    long long gfac_stride;
    int32_t gcol;              // the sequential Gaussian mode's column of the proposal step
    int32_t N, D, R;
    int32_t commit;            // a pending phase to commit
    long long chain_row;       // chain row of the pending phase's step (-1: not stored)
    int32_t propose;           // propose `phase` of Philox step `step`
    int32_t phase;
    unsigned long long step;
    // parallel tempering (emx_pt_set_tempering; nullptr beta: untempered, the kernel above bit for bit): lpq holds the untempered
    // log-likelihood L, the prior P is the box [box_lo, box_hi] or the caller's prior of the block (lpr), and the decision is
    // small_update's on the tempered pt_tempered(beta[b], L, P); L and P are kept per walker, chain_L holds the L rows and
    // chain_beta the beta of each stored row
    const double* beta;        // (B)
    const double* box_lo;      // (D) or nullptr
    const double* box_hi;
    const double* lpr;         // (B, R) the caller's prior of q, or nullptr
    double* L;                 // (B, N)
    double* P;                 // (B, N)
    double* chain_L;           // (B, cap, N)
    int32_t rows_in_commit;    // the commit writes the stored step's rows (0: the swap pass writes them after the step)
    double* chain_beta;        // (B, cap): the stored step's beta of each member, written with its rows
    // blobs (emx_set_batch_target_callback_blobs; nblobs 0: none, the kernel above bit for bit): the caller's blobs of q, row for
    // row with lpq; an accepted row's replace the walker's, and a stored step writes the walker's to the plane (tempered with
    // rows_in_commit 0: the swap pass writes the plane's rows, the commit only the walker's blobs)
    const double* bq;          // (B, R, nblobs)
    double* blobs;             // (B, N, nblobs)
    double* chain_blobs;       // (B, cap, N, nblobs)
    int32_t nblobs;
};

// threads of a k_batch_cb workgroup: at most 512, for 256 VGPRs a lane (with 1 024 threads' 128, 12 to 46 of them spilled)
constexpr int CB_MAX_THREADS = 512;

// (G, V, CH): pick_shape(D, D); `grid` = B workgroups of `threads`
hipError_t batch_cb_dispatch(int G, int V, int CH, int grid, int threads, hipStream_t st, const BatchCbArgs& a);
// the initial log-probs' NaN check: ST_NAN_LOGP in the status words of every member with a NaN among its N values
hipError_t batch_lp_check(const double* lp, uint32_t* status, int32_t B, int32_t N, hipStream_t st);

}  // namespace emx
