// The answers of the three half-step launchers of a fused user target (emx_fused_ensemble.hpp: fused_ens_launch_checks) to
// descriptors they refuse, or accept without launching: every row of the header's list of checks, and the pairs of simultaneous
// faults whose answers differ -- the order of the checks is part of the contract.  A stand-alone host program: no descriptor here
// reaches a launch (the split of every one is empty, so one that passed every check would still launch nothing), no HIP call is
// made, no device is needed.  Prints one line a call: launcher case answer.  tests/test_ensemble_fused_launch_answers_cpu.py
// compares them with a table.
//
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -I emcee_amd/csrc fused_launch_answers.hip -o fused_launch_answers
#include <emx_fused_ensemble_data.hpp>

#include <cstdio>

struct Plain {
    __device__ double operator()(const double* x, int ndim, int, const void*) const { return -0.5 * x[ndim - 1] * x[ndim - 1]; }
};
struct WithBlobs {
    __device__ double operator()(const double* x, int ndim, int, const void*, double* blobs) const {
        blobs[0] = x[0];
        blobs[1] = x[ndim - 1];
        return -0.5 * x[0] * x[0];
    }
};
struct WithData {
    __device__ double base(const double* x, int, const void*) const { return -0.5 * x[0] * x[0]; }
    __device__ double term(const double* x, int, long long k, const void*) const { return -x[1] * x[1] * (double)(k + 1); }
};

EMX_FUSED_ENSEMBLE_TARGET(plain, Plain, 5)
EMX_FUSED_ENSEMBLE_TARGET_BLOBS(blobs, WithBlobs, 5, 2)
EMX_FUSED_ENSEMBLE_DATA_TARGET(data, WithData, 5)

namespace {

constexpr int ND = 5, TILE = emx::fused_ens_tile_rule(ND);
double blob_store[2];

// a descriptor that passes every check; `a`: ndim 5 and an EMPTY split, so that nothing is ever launched
template <typename DESC>
DESC good(uint32_t abi, const emx::HalfStepArgs* a) {
    DESC L{};
    L.abi = abi;
    L.args_bytes = (uint32_t)sizeof(emx::HalfStepArgs);
    L.ndim = ND;
    L.move = emx::MOVE_STRETCH;
    L.grid = 8;
    L.threads = emx::FUSED_ENS_THREADS;
    L.lds_bytes = emx::fused_ens_lds_of(ND, TILE);
    L.args = a;
    return L;
}
emx_fused_ensemble_launch good_plain(const emx::HalfStepArgs* a) { return good<emx_fused_ensemble_launch>(EMX_FUSED_ENSEMBLE_ABI, a); }
emx_fused_ensemble_blobs_launch good_blobs(const emx::HalfStepArgs* a) {
    auto L = good<emx_fused_ensemble_blobs_launch>(EMX_FUSED_ENSEMBLE_BLOBS_ABI, a);
    L.nblobs = 2;
    L.blobs_cur = blob_store;
    return L;
}
emx_fused_ensemble_data_launch good_data(const emx::HalfStepArgs* a) {
    auto L = good<emx_fused_ensemble_data_launch>(EMX_FUSED_ENSEMBLE_DATA_ABI, a);
    L.ndata = 100;
    L.rows = 8;
    L.lds_bytes = emx::fused_ens_lds_of(ND, 8);
    return L;
}
emx::HalfStepArgs empty_split() {
    emx::HalfStepArgs a{};
    a.D = ND;
    a.t_lo = a.t_hi = 7;
    return a;
}

// the cases every launcher shares; `mk`: its good descriptor, `fn`: the launcher
template <typename DESC, typename MK, typename FN>
void common(const char* who, MK mk, FN fn, uint32_t other_abi) {
    auto say = [&](const char* what, const DESC* L) { printf("%s %s %d\n", who, what, fn(L)); };
    auto with = [&](const char* what, auto&& change_desc, auto&& change_args) {
        emx::HalfStepArgs a = empty_split();
        change_args(a);
        DESC L = mk(&a);
        change_desc(L);
        say(what, &L);
    };
    auto keep = [](auto&) {};
    static int something;
    say("null_descriptor", nullptr);
    with("other_abi", [&](DESC& L) { L.abi = other_abi; }, keep);
    with("other_args_bytes", [](DESC& L) { L.args_bytes += 8; }, keep);
    with("other_ndim", [](DESC& L) { L.ndim = ND + 1; }, keep);
    with("move_5", [](DESC& L) { L.move = 5; }, keep);
    with("move_minus_1", [](DESC& L) { L.move = -1; }, keep);
    with("probe", [](DESC& L) { L.grid = 0; }, keep);
    with("null_args", [](DESC& L) { L.args = nullptr; }, keep);
    with("negative_grid", [](DESC& L) { L.grid = -1; }, keep);
    with("threads_128", [](DESC& L) { L.threads = 128; }, keep);
    with("lds_one_byte_short", [](DESC& L) { L.lds_bytes -= 1; }, keep);
    with("args_other_ndim", keep, [](emx::HalfStepArgs& a) { a.D = ND + 1; });
    with("args_sendbuf", keep, [](emx::HalfStepArgs& a) { a.sendbuf = (decltype(a.sendbuf))&something; });
    with("args_desc", keep, [](emx::HalfStepArgs& a) { a.desc = (decltype(a.desc))&something; });
    with("args_t_hi_dev", keep, [](emx::HalfStepArgs& a) { a.t_hi_dev = (decltype(a.t_hi_dev))&something; });
    with("args_peers", keep, [](emx::HalfStepArgs& a) { a.peers = (decltype(a.peers))&something; });
    with("args_npeer", keep, [](emx::HalfStepArgs& a) { a.npeer = 2; });
    with("args_declp", keep, [](emx::HalfStepArgs& a) { a.declp = (decltype(a.declp))&something; });
    with("args_push_peers", keep, [](emx::HalfStepArgs& a) { a.push_peers = (decltype(a.push_peers))&something; });
    with("args_npush", keep, [](emx::HalfStepArgs& a) { a.npush = 1; });
    with("empty_split", keep, keep);
    with("reversed_split", keep, [](emx::HalfStepArgs& a) { a.t_hi = a.t_lo - 3; });
    // two faults at once: the earlier check answers
    with("other_abi+other_ndim", [&](DESC& L) { L.abi = other_abi; L.ndim = ND + 1; }, keep);
    with("other_ndim+move_5", [](DESC& L) { L.ndim = ND + 1; L.move = 5; }, keep);
    with("move_5+probe", [](DESC& L) { L.move = 5; L.grid = 0; }, keep);
    with("probe+threads_128", [](DESC& L) { L.grid = 0; L.threads = 128; }, keep);
    with("probe+null_args", [](DESC& L) { L.grid = 0; L.args = nullptr; }, keep);
    with("threads_128+args_other_ndim", [](DESC& L) { L.threads = 128; }, [](emx::HalfStepArgs& a) { a.D = ND + 1; });
    with("threads_128+args_npeer", [](DESC& L) { L.threads = 128; }, [](emx::HalfStepArgs& a) { a.npeer = 2; });
    with("args_other_ndim+args_npeer", keep, [](emx::HalfStepArgs& a) { a.D = ND + 1; a.npeer = 2; });
    with("args_npeer+reversed_split", keep, [](emx::HalfStepArgs& a) { a.npeer = 2; a.t_hi = a.t_lo - 3; });
}

}  // namespace

int main() {
    using emx::HalfStepArgs;
    common<emx_fused_ensemble_launch>("plain", good_plain, plain, EMX_FUSED_ENSEMBLE_BLOBS_ABI);
    common<emx_fused_ensemble_blobs_launch>("blobs", good_blobs, blobs, EMX_FUSED_ENSEMBLE_ABI);
    common<emx_fused_ensemble_data_launch>("data", good_data, data, EMX_FUSED_ENSEMBLE_ABI);

    // the blob launcher's own checks: the count ahead of the probe and of the launch shape, the walkers' array behind the shape
    auto blob_case = [&](const char* what, auto&& change_desc, auto&& change_args) {
        HalfStepArgs a = empty_split();
        change_args(a);
        auto L = good_blobs(&a);
        change_desc(L);
        printf("blobs %s %d\n", what, blobs(&L));
    };
    auto keep = [](auto&) {};
    using BL = emx_fused_ensemble_blobs_launch;
    blob_case("nblobs_3", [](BL& L) { L.nblobs = 3; }, keep);
    blob_case("null_blobs_cur", [](BL& L) { L.blobs_cur = nullptr; }, keep);
    blob_case("move_5+nblobs_3", [](BL& L) { L.move = 5; L.nblobs = 3; }, keep);
    blob_case("nblobs_3+probe", [](BL& L) { L.nblobs = 3; L.grid = 0; }, keep);
    blob_case("nblobs_3+threads_128", [](BL& L) { L.nblobs = 3; L.threads = 128; }, keep);
    blob_case("probe+null_blobs_cur", [](BL& L) { L.grid = 0; L.blobs_cur = nullptr; }, keep);
    blob_case("threads_128+null_blobs_cur", [](BL& L) { L.threads = 128; L.blobs_cur = nullptr; }, keep);
    blob_case("null_args+null_blobs_cur", [](BL& L) { L.args = nullptr; L.blobs_cur = nullptr; }, keep);
    blob_case("null_blobs_cur+args_other_ndim", [](BL& L) { L.blobs_cur = nullptr; }, [](HalfStepArgs& a) { a.D = ND + 1; });
    blob_case("null_blobs_cur+args_npeer", [](BL& L) { L.blobs_cur = nullptr; }, [](HalfStepArgs& a) { a.npeer = 2; });

    // the data launcher's own checks: rows a workgroup and the count of data behind the probe, ahead of the launch shape
    auto data_case = [&](const char* what, auto&& change_desc, auto&& change_args) {
        HalfStepArgs a = empty_split();
        change_args(a);
        auto L = good_data(&a);
        change_desc(L);
        printf("data %s %d\n", what, data(&L));
    };
    using DL = emx_fused_ensemble_data_launch;
    data_case("rows_3", [](DL& L) { L.rows = 3; }, keep);
    data_case("rows_4", [](DL& L) { L.rows = 4; }, keep);
    data_case("rows_tile", [](DL& L) { L.rows = TILE; L.lds_bytes = emx::fused_ens_lds_of(ND, TILE); }, keep);
    data_case("rows_tile+lds_of_8_rows", [](DL& L) { L.rows = TILE; }, keep);
    data_case("rows_tile_plus_1", [](DL& L) { L.rows = TILE + 1; L.lds_bytes = emx::fused_ens_lds_of(ND, TILE + 1); }, keep);
    data_case("ndata_minus_1", [](DL& L) { L.ndata = -1; }, keep);
    data_case("ndata_0", [](DL& L) { L.ndata = 0; }, keep);
    data_case("ndata_2^31", [](DL& L) { L.ndata = 1ll << 31; }, keep);
    data_case("probe+rows_3", [](DL& L) { L.grid = 0; L.rows = 3; }, keep);
    data_case("rows_3+null_args", [](DL& L) { L.rows = 3; L.args = nullptr; }, keep);
    data_case("rows_3+args_other_ndim", [](DL& L) { L.rows = 3; }, [](HalfStepArgs& a) { a.D = ND + 1; });
    data_case("rows_3+args_npeer", [](DL& L) { L.rows = 3; }, [](HalfStepArgs& a) { a.npeer = 2; });
    data_case("ndata_2^31+args_other_ndim", [](DL& L) { L.ndata = 1ll << 31; }, [](HalfStepArgs& a) { a.D = ND + 1; });
    return 0;
}
