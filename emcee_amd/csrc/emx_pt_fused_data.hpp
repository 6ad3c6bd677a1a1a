// Fused tempered targets whose log-likelihood SUMS OVER AN OBJECT'S DATA (include/emx.h: emx_pt_set_target_fused_data;
// emcee_amd.targets.PTFused(..., ndata=) / compile_fused_pt(..., data=True)).  PUBLIC: the header a user's translation unit includes to
// compile a likelihood of the form  log L(theta) = base(theta) + sum_k term(theta; datum_k)  into the tempered one-workgroup kernel
// k_pt_run (emx_pt_fused.hpp) with a WAVE a row in the data sum, where emx_pt_fused.hpp's functor would loop over the object's data in
// one of the T R lanes its second pass keeps busy.  The tempered counterpart of emx_fused_target_data.hpp.
//
//     #include <emx_pt_fused_data.hpp>            // hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -I include -I emcee_amd/csrc
//     struct MyModel {                            // stateless; `user`: the device pointer given to PTFused, member = object * ntemps + rung
//         // once a row, by one lane: normalisation, all of the likelihood that does not run over the data
//         __device__ double base(const double* x, int ndim, int member, const void* user) const;
//         // datum k of [0, ndata[member]): pure, no LDS of its own, no barrier, no cross-lane operation
//         __device__ double term(const double* x, int ndim, int member, long long k, const void* user) const;
//     };
//     struct MyPrior { __device__ double operator()(const double* x, int ndim, int member, const void* user) const; };
//     EMX_FUSED_PT_DATA_TARGET(my_model, MyModel, MyPrior, /*ndim=*/5)            // emits: extern "C" int my_model(emx_pt_fused_launch*)
//     EMX_FUSED_PT_DATA_TARGET(my_flat, MyModel, emx::NoFusedPrior, 5)            // no prior functor: the handle's box, or a flat prior
//
// The model has EMX_FUSED_BATCH_DATA_TARGET's contract and the prior EMX_FUSED_PT_TARGET's.  `ndata` is a run-time value PER MEMBER,
// given when the target is bound (0 <= ndata[member] < 2^31; every rung of an object is given the object's count).
//
// THE VALUE of the untempered likelihood is emx_fused_target_data.hpp's, "THE VALUE": base + S with the 64 lane partials in ascending
// k and the balanced pairwise tree (emcee_amd.targets.fused_data_sum on the host).
//   * base -inf or NaN: no term is evaluated and the value is base (NaN where the prior is finite raises the reference's error naming
//     (object, rung));
//   * ndata[member] == 0 gives base + 0.0;
//   * a row outside the prior (-inf) does not reach the model at all, and its likelihood is kept as -inf;
//   * a non-finite proposal is rejected without reaching prior or model.
// The tempered log-probability, the decision, the swap pass and the ladder update are k_pt_run's: the run is bit for bit the
// EMX_FUSED_PT_TARGET run of a one-lane functor that computes the same value.
// Out of scope: blobs, rng="mt19937", an object's data sum spread over more than one workgroup.
#pragma once
#include "emx_fused_target_data.hpp"
#include "emx_pt_fused.hpp"

// bumped with ANY change of PtRunArgs, of k_pt_run's LDS layout or of the DATA form's launch rules.  A value of its own: a data
// launcher handed EMX_FUSED_PT_ABI, and an EMX_FUSED_PT_TARGET launcher handed this one, answer 1
#ifndef EMX_FUSED_PT_DATA_ABI
#define EMX_FUSED_PT_DATA_ABI 0x50544403u
#endif

namespace emx {

// the launcher behind EMX_FUSED_PT_DATA_TARGET: fused_launch_checks (emx_fused_target.hpp) against the data ABI, then one launch of every
// object with a wave a row in the second pass (include/emx.h: emx_pt_fused_launch; PtRunArgs::ndata is the library's)
template <typename MODEL, typename PRIOR, int NDIM, int MOVES>
int fused_pt_data_launch(emx_pt_fused_launch* L) {
    static_assert(NDIM >= 1 && NDIM <= 256, "a fused tempered target has 1 <= ndim <= 256");
    static_assert((MOVES & (EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY)) != 0, "no move selector compiled in");
    constexpr bool OK = has_batch_data_base<MODEL>::value && has_batch_data_term<MODEL>::value;
    static_assert(has_batch_data_base<MODEL>::value,
                  "EMX_FUSED_PT_DATA_TARGET: the model needs  __device__ double base(const double* x, int ndim, int member, const void* user) const");
    static_assert(has_batch_data_term<MODEL>::value,
                  "EMX_FUSED_PT_DATA_TARGET: the model needs  __device__ double term(const double* x, int ndim, int member, long long k, "
                  "const void* user) const");
    bool stretch = false;
    const int rc = fused_launch_checks(L, EMX_FUSED_PT_DATA_ABI, sizeof(PtRunArgs), NDIM, MOVES, PT_RUN_MAX_THREADS, &stretch, [](emx_pt_fused_launch* d) {
        d->has_prior = std::is_same<PRIOR, NoFusedPrior>::value ? 0 : 1;      // the probe reports it
        return FUSED_GO_ON;
    });
    if (rc != FUSED_GO_ON) return rc;
    PtRunArgs a = *static_cast<const PtRunArgs*>(L->args);
    if (a.D != NDIM) return 2;
    if (!a.ndata) return 3;                           // the members' counts are the library's to fill
    if (a.nblobs != 0) return 4;                      // the DATA form carries no blobs
    a.user = L->user;
    return fused_launch_by_moves<OK ? MOVES : 0>(stretch, [&](auto sel) {
        return launch_pt_move<MODEL, PRIOR, NDIM, decltype(sel)::value, true>(L->grid, L->threads, (size_t)L->lds_bytes, (hipStream_t)L->hip_stream, a);
    });
}

}  // namespace emx

#define EMX_FUSED_PT_DATA_TARGET_MOVES(name, Model, PriorFunctor, ndim, moves)                        \
    extern "C" __attribute__((visibility("default"))) int name(emx_pt_fused_launch* launch) {         \
        return emx::fused_pt_data_launch<Model, PriorFunctor, (ndim), (moves)>(launch);               \
    }
#define EMX_FUSED_PT_DATA_TARGET(name, Model, PriorFunctor, ndim) \
    EMX_FUSED_PT_DATA_TARGET_MOVES(name, Model, PriorFunctor, ndim, EMX_FUSED_MOVES_STRETCH | EMX_FUSED_MOVES_ANY)
