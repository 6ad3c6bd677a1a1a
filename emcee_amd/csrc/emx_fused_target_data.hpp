// Fused user targets of a batch of small ensembles whose log-probability SUMS OVER PER-MEMBER DATA (include/emx.h:
// emx_set_batch_target_fused_data; emcee_amd.targets.BatchFused(..., ndata=) / compile_fused(..., data=True)).  PUBLIC: the header a
// user's translation unit includes to compile a likelihood of the form  log p(theta) = base(theta) + sum_k term(theta; datum_k)
// into the one-workgroup kernel k_small_run (emx_kernels.hpp) with a WAVE a row in the data sum, where emx_fused_target.hpp's
// functor would loop over the member's data in one lane.  The batch counterpart of emx_fused_ensemble_data.hpp.
//
//     #include <emx_fused_target_data.hpp>        // hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -I include -I emcee_amd/csrc
//     struct MyModel {                            // stateless; `user`: the device pointer given to BatchFused, `member`: the index in the batch
//         // once a row, by one lane: prior, normalisation, all that does not run over the data
//         __device__ double base(const double* x, int ndim, int member, const void* user) const;
//         // datum k of [0, ndata[member]): pure, no LDS of its own, no barrier, no cross-lane operation
//         __device__ double term(const double* x, int ndim, int member, long long k, const void* user) const;
//     };
//     EMX_FUSED_BATCH_DATA_TARGET(my_model, MyModel, /*ndim=*/5)   // emits: extern "C" int my_model(const emx_fused_batch_data_launch*)
//
// `x` points at `ndim` doubles in LDS (the staged row).  `ndata` is a run-time value PER MEMBER, given when the target is bound
// (0 <= ndata[member] < 2^31), not a template argument: one launcher serves every catalogue, ragged ones included.
//
// THE VALUE.  The log-probability of a row is DEFINED as  base + S  where
//   * lane partial p_l, l = 0 ... 63, starts at +0.0 and adds term(x, ndim, member, k, user) for k = l, l + 64, l + 128, ... in
//     ascending k (p_l = p_l + term: a separate add, the translation unit is compiled with -ffp-contract=off);
//   * S is the balanced pairwise tree over p_0 ... p_63 -- adjacent pairs, level by level: (p_0 + p_1), (p_2 + p_3), ..., then
//     pairs of those, six levels -- which is what group_sum<64> of emx_kernels.hpp computes.
// It depends on nothing else: not the threads of the workgroup, not the plan steps a pass, not the size of the batch, not the move.
// emcee_amd.targets.fused_data_sum(terms) sums a float64 array in exactly this order on the host.
//   * base -inf or NaN: no term is evaluated for that row and the value is base (NaN raises the reference's error naming the
//     member, -inf rejects);
//   * a NaN  base + S  raises the reference's error too;
//   * a row with a non-finite coordinate is rejected without reaching the model;
//   * ndata[member] == 0 gives base + 0.0.
// Member b of such a batch is, bit for bit, the single sampler's run of the same model as an EMX_FUSED_ENSEMBLE_DATA_TARGET with
// ndata[b] data under rng="philox" and the member's seed.
//
// The kernel is k_small_run's DATA form: the first pass of a half-step (the proposals into the LDS staging rows, G lanes a row), the
// plans and the chain append are the text every fused user target runs; in the second pass each wave takes staged rows in turn --
// lane 0 calls base, all 64 lanes stride over the member's data, the reduction runs with the whole wave active outside any
// lane-divergent region, lane 0 takes the decision and the wave commits the row with all its lanes.  The initial log-probs take the
// same form over every walker.  Both move selectors are carried (a single StretchMove; any schedule), Philox plans only.
// Out of scope: blobs, the single sampler's one-workgroup form.  (PTSampler's data targets: emx_pt_fused_data.hpp.)
#pragma once
#include <type_traits>
#include <utility>

#include "emx_fused_target.hpp"

// bumped with ANY change of SmallRunArgs, of k_small_run's LDS layout or of emx_fused_batch_data_launch.  A value of its own: a data
// launcher handed emx_fused_launch, and an EMX_FUSED_BATCH_TARGET launcher handed the data descriptor, answer 1
#ifndef EMX_FUSED_BATCH_DATA_ABI
#define EMX_FUSED_BATCH_DATA_ABI 0x42444401u
#endif

namespace emx {

// whether Model has the two members of the contract (checked where the launcher is emitted: one diagnostic that names the missing
// member, not the kernels' instantiation traces)
template <typename M, typename = void>
struct has_batch_data_base : std::false_type {};
template <typename M>
struct has_batch_data_base<M, std::void_t<decltype(std::declval<const M&>().base((const double*)nullptr, 0, 0, (const void*)nullptr))>>
    : std::is_convertible<decltype(std::declval<const M&>().base((const double*)nullptr, 0, 0, (const void*)nullptr)), double> {};
template <typename M, typename = void>
struct has_batch_data_term : std::false_type {};
template <typename M>
struct has_batch_data_term<M, std::void_t<decltype(std::declval<const M&>().term((const double*)nullptr, 0, 0, 0LL, (const void*)nullptr))>>
    : std::is_convertible<decltype(std::declval<const M&>().term((const double*)nullptr, 0, 0, 0LL, (const void*)nullptr)), double> {};

// the launcher behind EMX_FUSED_BATCH_DATA_TARGET: fused_launch_checks (emx_fused_target.hpp) against the data descriptor
// (include/emx.h: emx_fused_batch_data_launch), then one launch of the batch
template <typename USER, int NDIM, int MOVES>
int fused_batch_data_launch(const emx_fused_batch_data_launch* L) {
    static_assert(NDIM >= 1 && NDIM <= 256, "a fused user target has 1 <= ndim <= 256");
    static_assert((MOVES & (EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY)) != 0, "no move selector compiled in");
    constexpr bool MODEL = has_batch_data_base<USER>::value && has_batch_data_term<USER>::value;
    static_assert(has_batch_data_base<USER>::value,
                  "EMX_FUSED_BATCH_DATA_TARGET: the model needs  __device__ double base(const double* x, int ndim, int member, const void* user) const");
    static_assert(has_batch_data_term<USER>::value,
                  "EMX_FUSED_BATCH_DATA_TARGET: the model needs  __device__ double term(const double* x, int ndim, int member, long long k, "
                  "const void* user) const");
    bool stretch = false;
    // a data target carries no blobs (4); a launch (grid != 0) needs the members' counts: one of the shape check's faults (3)
    const auto site = [](const emx_fused_batch_data_launch* d) { return d->nblobs != 0 ? 4 : d->grid != 0 && !d->ndata ? 3 : FUSED_GO_ON; };
    const int rc = fused_launch_checks(L, EMX_FUSED_BATCH_DATA_ABI, sizeof(SmallRunArgs), NDIM, MOVES, 1024, &stretch, site);
    if (rc != FUSED_GO_ON) return rc;
    SmallRunArgs a = *static_cast<const SmallRunArgs*>(L->args);
    if (a.D != NDIM) return 2;
    if (a.nblobs != 0) return 4;
    a.user = L->user;
    a.ndata = reinterpret_cast<const long long*>(L->ndata);
    return fused_launch_by_moves<MODEL ? MOVES : 0>(stretch, [&](auto sel) {
        return launch_fused_move<USER, NDIM, decltype(sel)::value, 0, true>(L->grid, L->threads, (size_t)L->lds_bytes, (hipStream_t)L->hip_stream, a);
    });
}

}  // namespace emx

#define EMX_FUSED_BATCH_DATA_TARGET_MOVES(name, Model, ndim, moves)                                        \
    extern "C" __attribute__((visibility("default"))) int name(const emx_fused_batch_data_launch* launch) { \
        return emx::fused_batch_data_launch<Model, (ndim), (moves)>(launch);                                \
    }
#define EMX_FUSED_BATCH_DATA_TARGET(name, Model, ndim) \
    EMX_FUSED_BATCH_DATA_TARGET_MOVES(name, Model, ndim, EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY)
