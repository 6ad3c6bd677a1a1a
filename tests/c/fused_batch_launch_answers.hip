// The answers of the launchers of a fused batch target and of a fused tempered target (emx_fused_target.hpp: fused_launch_checks,
// and the checks each launcher keeps at its call site) to descriptors they refuse, or accept without launching: one descriptor
// per check of each ladder, and the pairs of simultaneous faults whose answers depend on the order -- the order of the checks is
// part of the contract.  A stand-alone host program.  EVERY descriptor with grid != 0 carries at least one fault that its launcher
// refuses, so none reaches a launch; the program refuses to run at all where a device is visible (the test hides them).
// Prints one line a call: launcher case answer, and for the tempered launchers has_prior as the call left it (-1: not written).
// tests/test_batch_fused_launch_answers_cpu.py compares them with a table.
//
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -I emcee_amd/csrc fused_batch_launch_answers.hip -o fused_batch_launch_answers
#include <emx_pt_fused_data.hpp>

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
    __device__ double base(const double* x, int, int, const void*) const { return -0.5 * x[0] * x[0]; }
    __device__ double term(const double* x, int, int, long long k, const void*) const { return -x[1] * x[1] * (double)(k + 1); }
};
struct Prior {
    __device__ double operator()(const double* x, int, int, const void*) const { return x[0] > -10.0 && x[0] < 10.0 ? 0.0 : -INFINITY; }
};

EMX_FUSED_BATCH_TARGET(plain, Plain, 5)
EMX_FUSED_BATCH_TARGET_BLOBS(blobs, WithBlobs, 5, 2)
EMX_FUSED_BATCH_DATA_TARGET(data, WithData, 5)
EMX_FUSED_BATCH_TARGET_MOVES(stretch_only, Plain, 5, EMX_FUSED_MOVES_STRETCH)
EMX_FUSED_PT_TARGET(pt, Plain, emx::NoFusedPrior, 5)
EMX_FUSED_PT_TARGET(pt_prior, Plain, Prior, 5)
EMX_FUSED_PT_DATA_TARGET(pt_data, WithData, Prior, 5)

namespace {

constexpr int ND = 5;
constexpr int SEL_ANY = 7;      // include/emx.h: emx_fused_launch::movesel
double blob_store[2];
long long count_store[8];

// the descriptor a case starts from: right in every field, grid 8 -- so every case that keeps the grid adds a fault
template <typename DESC, typename ARGS>
DESC start(uint32_t abi, const ARGS* a) {
    DESC L{};
    L.abi = abi;
    L.args_bytes = (uint32_t)sizeof(ARGS);
    L.ndim = ND;
    L.movesel = emx::MOVE_STRETCH;
    L.grid = 8;
    L.threads = 64;
    L.args = a;
    return L;
}

template <typename DESC>
int has_prior_of(const DESC&) { return -2; }
int has_prior_of(const emx_pt_fused_launch& L) { return L.has_prior; }

// one launcher: its descriptor and argument types, its name, what its right descriptor and arguments carry beyond start()
template <typename DESC, typename ARGS, typename FN, typename FIXD, typename FIXA>
struct Cases {
    const char* who;
    FN fn;
    uint32_t abi;
    FIXD fix_desc;
    FIXA fix_args;

    void say(const char* what, DESC* L) const {
        const int rc = fn(L);
        if (L && has_prior_of(*L) != -2)
            printf("%s %s %d %d\n", who, what, rc, has_prior_of(*L));
        else if (has_prior_of(DESC{}) != -2)
            printf("%s %s %d %d\n", who, what, rc, -1);
        else
            printf("%s %s %d\n", who, what, rc);
    }
    template <typename CD, typename CA>
    void with(const char* what, CD&& change_desc, CA&& change_args) const {
        ARGS a{};
        a.D = ND;
        fix_args(a);
        change_args(a);
        DESC L = start<DESC, ARGS>(abi, &a);
        fix_desc(L);
        change_desc(L);
        say(what, &L);
    }

    // the ladder every launcher shares.  `sibling_abi`: the ABI constant of the same sampler's other form; `over`: threads above the cap
    void common(uint32_t sibling_abi, int over) const {
        auto keep = [](auto&) {};
        say("null_descriptor", nullptr);
        with("other_abi", [&](DESC& L) { L.abi = abi + 0x1000u; }, keep);
        with("sibling_abi", [&](DESC& L) { L.abi = sibling_abi; }, keep);
        with("other_args_bytes", [](DESC& L) { L.args_bytes += 8; }, keep);
        with("other_ndim", [](DESC& L) { L.ndim = ND + 1; }, keep);
        with("movesel_5", [](DESC& L) { L.movesel = 5; }, keep);
        with("movesel_minus_1", [](DESC& L) { L.movesel = -1; }, keep);
        with("probe", [](DESC& L) { L.grid = 0; }, keep);
        with("any_selector+probe", [](DESC& L) { L.movesel = SEL_ANY; L.grid = 0; }, keep);
        with("null_args", [](DESC& L) { L.args = nullptr; }, keep);
        with("negative_grid", [](DESC& L) { L.grid = -1; }, keep);
        with("threads_0", [](DESC& L) { L.threads = 0; }, keep);
        with("threads_32", [](DESC& L) { L.threads = 32; }, keep);
        with("threads_96", [](DESC& L) { L.threads = 96; }, keep);
        with("threads_over", [&](DESC& L) { L.threads = over; }, keep);
        with("args_other_ndim", keep, [](ARGS& a) { a.D = ND + 1; });
        // two faults at once: the earlier check answers
        with("other_abi+other_ndim", [&](DESC& L) { L.abi = abi + 0x1000u; L.ndim = ND + 1; }, keep);
        with("other_args_bytes+other_ndim", [](DESC& L) { L.args_bytes += 8; L.ndim = ND + 1; }, keep);
        with("other_ndim+movesel_5", [](DESC& L) { L.ndim = ND + 1; L.movesel = 5; }, keep);
        with("movesel_5+probe", [](DESC& L) { L.movesel = 5; L.grid = 0; }, keep);
        with("probe+threads_96", [](DESC& L) { L.grid = 0; L.threads = 96; }, keep);
        with("probe+null_args", [](DESC& L) { L.grid = 0; L.args = nullptr; }, keep);
        with("probe+args_other_ndim", [](DESC& L) { L.grid = 0; }, [](ARGS& a) { a.D = ND + 1; });
        with("threads_96+args_other_ndim", [](DESC& L) { L.threads = 96; }, [](ARGS& a) { a.D = ND + 1; });
        with("negative_grid+args_other_ndim", [](DESC& L) { L.grid = -1; }, [](ARGS& a) { a.D = ND + 1; });
    }

    // the blob count of a batch descriptor and of its arguments
    void batch_blobs() const {
        auto keep = [](auto&) {};
        with("nblobs_other", [](DESC& L) { L.nblobs += 1; }, keep);
        with("nblobs_other+null_args", [](DESC& L) { L.nblobs += 1; L.args = nullptr; }, keep);
        with("nblobs_other+null_args+probe", [](DESC& L) { L.nblobs += 1; L.args = nullptr; L.grid = 0; }, keep);
        with("movesel_5+nblobs_other", [](DESC& L) { L.movesel = 5; L.nblobs += 1; }, keep);
        with("nblobs_other+probe", [](DESC& L) { L.nblobs += 1; L.grid = 0; }, keep);
        with("nblobs_other+threads_96", [](DESC& L) { L.nblobs += 1; L.threads = 96; }, keep);
        with("args_nblobs_other", keep, [](ARGS& a) { a.nblobs += 1; });
        with("threads_96+args_nblobs_other", [](DESC& L) { L.threads = 96; }, [](ARGS& a) { a.nblobs += 1; });
        with("args_other_ndim+args_nblobs_other", keep, [](ARGS& a) { a.D = ND + 1; a.nblobs += 1; });
    }
};
template <typename DESC, typename ARGS, typename FN, typename FIXD, typename FIXA>
Cases<DESC, ARGS, FN, FIXD, FIXA> cases(const char* who, FN fn, uint32_t abi, FIXD fix_desc, FIXA fix_args) {
    return {who, fn, abi, fix_desc, fix_args};
}

}  // namespace

int main() {
    using emx::PtRunArgs;
    using emx::SmallRunArgs;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        printf("a device is visible (%d): this program runs with every device hidden\n", ndev);
        return 2;
    }
    auto keep = [](auto&) {};
    using BL = emx_fused_launch;
    using DL = emx_fused_batch_data_launch;
    using PL = emx_pt_fused_launch;

    const auto c_plain = cases<BL, SmallRunArgs>("plain", plain, EMX_FUSED_ABI, keep, keep);
    c_plain.common(EMX_FUSED_BATCH_DATA_ABI, 1088);
    c_plain.batch_blobs();

    const auto c_blobs = cases<BL, SmallRunArgs>("blobs", blobs, EMX_FUSED_ABI, [](BL& L) { L.nblobs = 2; },
                                                 [](SmallRunArgs& a) { a.nblobs = 2; a.blobs = blob_store; });
    c_blobs.common(EMX_FUSED_BATCH_DATA_ABI, 1088);
    c_blobs.batch_blobs();
    c_blobs.with("args_null_blobs", keep, [](SmallRunArgs& a) { a.blobs = nullptr; });
    c_blobs.with("probe+args_null_blobs", [](BL& L) { L.grid = 0; }, [](SmallRunArgs& a) { a.blobs = nullptr; });
    c_blobs.with("threads_96+args_null_blobs", [](BL& L) { L.threads = 96; }, [](SmallRunArgs& a) { a.blobs = nullptr; });
    c_blobs.with("args_other_ndim+args_null_blobs", keep, [](SmallRunArgs& a) { a.D = ND + 1; a.blobs = nullptr; });

    const auto c_data = cases<DL, SmallRunArgs>("data", data, EMX_FUSED_BATCH_DATA_ABI,
                                                [](DL& L) { L.ndata = reinterpret_cast<const int64_t*>(count_store); }, keep);
    c_data.common(EMX_FUSED_ABI, 1088);
    c_data.batch_blobs();
    c_data.with("null_ndata", [](DL& L) { L.ndata = nullptr; }, keep);
    c_data.with("probe+null_ndata", [](DL& L) { L.grid = 0; L.ndata = nullptr; }, keep);
    c_data.with("nblobs_other+null_ndata", [](DL& L) { L.nblobs = 1; L.ndata = nullptr; }, keep);
    c_data.with("null_ndata+args_other_ndim", [](DL& L) { L.ndata = nullptr; }, [](SmallRunArgs& a) { a.D = ND + 1; });
    c_data.with("null_ndata+args_nblobs_other", [](DL& L) { L.ndata = nullptr; }, [](SmallRunArgs& a) { a.nblobs = 1; });

    const auto c_stretch = cases<BL, SmallRunArgs>("stretch_only", stretch_only, EMX_FUSED_ABI, keep, keep);
    c_stretch.common(EMX_FUSED_BATCH_DATA_ABI, 1088);
    c_stretch.batch_blobs();
    c_stretch.with("any_selector", [](BL& L) { L.movesel = SEL_ANY; }, keep);
    c_stretch.with("other_ndim+any_selector", [](BL& L) { L.ndim = ND + 1; L.movesel = SEL_ANY; }, keep);
    c_stretch.with("any_selector+nblobs_other", [](BL& L) { L.movesel = SEL_ANY; L.nblobs = 1; }, keep);
    c_stretch.with("any_selector+args_other_ndim", [](BL& L) { L.movesel = SEL_ANY; }, [](SmallRunArgs& a) { a.D = ND + 1; });

    auto unwritten = [](PL& L) { L.has_prior = -1; };
    const auto c_pt = cases<PL, PtRunArgs>("pt", pt, EMX_FUSED_PT_ABI, unwritten, keep);
    c_pt.common(EMX_FUSED_PT_DATA_ABI, 576);
    c_pt.with("threads_1088", [](PL& L) { L.threads = 1088; }, keep);
    const auto c_prior = cases<PL, PtRunArgs>("pt_prior", pt_prior, EMX_FUSED_PT_ABI, unwritten, keep);
    c_prior.common(EMX_FUSED_PT_DATA_ABI, 576);
    const auto c_ptd = cases<PL, PtRunArgs>("pt_data", pt_data, EMX_FUSED_PT_DATA_ABI, unwritten, [](PtRunArgs& a) { a.ndata = count_store; });
    c_ptd.common(EMX_FUSED_PT_ABI, 576);
    c_ptd.with("args_null_ndata", keep, [](PtRunArgs& a) { a.ndata = nullptr; });
    c_ptd.with("probe+args_null_ndata", [](PL& L) { L.grid = 0; }, [](PtRunArgs& a) { a.ndata = nullptr; });
    c_ptd.with("threads_96+args_null_ndata", [](PL& L) { L.threads = 96; }, [](PtRunArgs& a) { a.ndata = nullptr; });
    c_ptd.with("args_other_ndim+args_null_ndata", keep, [](PtRunArgs& a) { a.D = ND + 1; a.ndata = nullptr; });
    return 0;
}
