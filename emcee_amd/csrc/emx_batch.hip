// Batches of independent small ensembles (include/emx.h: emx_batch_*; emcee_amd.EnsembleBatch): B ensembles of one shape
// (nwalkers, ndim), each with its own state, Philox seed, target parameters, status and chain, run by ONE launch of
// k_small_run<..., BATCH = true> per chunk of steps -- workgroup b runs member b exactly as a single-ensemble launch runs that
// ensemble, so every member's bits are those of an emx_ctx with the same seed, target and initial state.  Philox mode only.
// Host side of the handle and the batched instantiations of the kernel (emx_small_launch.hpp).  With the caller's batched
// log-prob (emx_set_batch_target_callback) a run is k_batch_cb launches and calls of that function instead (emx_batch_cb.hip).
// With a fused user target (emx_set_batch_target_fused) the launch is the caller's own instantiation of k_small_run around their
// device function (emx_fused_target.hpp), through the launcher their translation unit exports; everything else is shared.
// With a fused tempered target (emx_pt_set_target_fused) a run is launches of the caller's instantiation of k_pt_run
// (emx_pt_fused.hpp), one workgroup an object, one launch a chunk of steps (launch_pt below).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/emx.h"
#include "emx_batch_cb.hpp"
#include "emx_fused_target.hpp"
#include "emx_fused_target_data.hpp"
#include "emx_internal.hpp"
#include "emx_pt.hpp"
#include "emx_pt_fused.hpp"
#include "emx_pt_fused_data.hpp"
#include "emx_rng.hpp"
#include "emx_small_host.hpp"
#include "emx_small_launch.hpp"

using namespace emx;

struct emx_batch {
    int device = 0;
    int32_t B = 0, D = 0;
    int64_t N = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // member-strided state: X (B, N, D), lp (B, N), acc (B, N), acc_count (B, N); status: SMALL_STATUS_WORDS words a member
    double *X = nullptr, *lp = nullptr;
    uint8_t* acc = nullptr;
    uint32_t* acc_count = nullptr;
    uint32_t *status_host = nullptr, *status = nullptr;
    // target: kind, per-member parameters at their strides (0: shared), per-member scales
    int32_t target = -1;
    int Dp = 0;
    double *tp0 = nullptr, *tp1 = nullptr, *tscales = nullptr;
    int64_t tp0_stride = 0, tp1_stride = 0;
    // moves
    std::vector<emx_move_desc> moves;
    std::vector<double> cdf;
    std::vector<double*> mscale;
    // Philox
    unsigned long long* seeds = nullptr;       // device copy
    std::vector<uint64_t> seeds_host;
    uint64_t step = 0;
    // chain: member-major (B, cap, N, D) and (B, cap, N)
    double *chain = nullptr, *chain_lp = nullptr;
    int64_t cap = 0, stored = 0, proposals = 0;
    // per-launch Gaussian-move factors (B x steps) and columns
    double* fac_dev = nullptr;
    int32_t* col_dev = nullptr;
    size_t fac_cap = 0, col_cap = 0;
    // tuning: batch_threads / batch_plan_steps (0: auto); what the last launch used
    int64_t tune_threads = 0, tune_plan_steps = 0;
    int32_t last_threads = 0, last_plan_steps = 0;
    int64_t launches = 0;
    // EMX_TARGET_DEVICE_CALLBACK: the caller's function, the (B, R, D) block it is handed and its (B, R) results, the commit's
    // scratch (factor, log-uniform, walker of every row; real rows of every member)
    emx_batch_log_prob_fn cb_fn = nullptr;
    void* cb_user = nullptr;
    double *cb_q = nullptr, *cb_lp = nullptr, *cb_fac = nullptr, *cb_logu = nullptr;
    int32_t *cb_wi = nullptr, *cb_nrows = nullptr;
    size_t cb_rows = 0;       // B R rows allocated
    // EMX_TARGET_FUSED_USER: the caller's launcher of k_small_run around their device function, and their device pointer
    emx_fused_batch_fn fused_fn = nullptr;
    const void* fused_user = nullptr;
    // ... whose log-probability sums over per-member data (emx_set_batch_target_fused_data): the data launcher instead of
    // fused_fn, and the library's device copy of the members' counts (B values)
    emx_fused_batch_data_fn fused_data_fn = nullptr;
    int64_t* fused_ndata = nullptr;
    // blobs (emx_set_batch_target_fused_blobs / emx_set_batch_target_callback_blobs; 0: none): the walkers' current ones (B, N,
    // nblobs), the blob plane (B, cap, N, nblobs) next to the chain, the callback's function and its (B, R, nblobs) block
    int32_t nblobs = 0;
    double *blobs = nullptr, *chain_blobs = nullptr, *cb_bq = nullptr;
    emx_batch_log_prob_blobs_fn cbb_fn = nullptr;
    // emx_autocorr_batch (emx_batch_acf.hip): its hipFFT plans and scratch; tuning "batch_acf_series" (0: auto)
    BatchAcf* acf = nullptr;
    int64_t tune_acf_series = 0;
    // emx_summary_batch (emx_batch_summary.hip): its scratch; tuning "batch_summary_members" (0: auto)
    BatchSummary* summary = nullptr;
    int64_t tune_summary_members = 0;
    // emx_histograms_batch (emx_batch_summary.hip): tuning "batch_hist_members" / "batch_hist_rows" (0: auto); its scratch is summary's
    int64_t tune_hist_members = 0, tune_hist_rows = 0;
    // emx_rhat_batch (emx_rhat.hip): its scratch; tuning "batch_rhat_members" (0: auto)
    RhatScratch* rhat = nullptr;
    int64_t tune_rhat_members = 0;
    // emx_pt_evidence (emx_pt_evidence.hip): its scratch
    PtEvidenceScratch* pt_evidence = nullptr;
    // parallel tempering (emx_pt_set_tempering; pt_T 0: untempered): groups of pt_T members, member m at rung m % pt_T; each
    // member's beta, the box prior, L and P per walker, the L chain, the caller's prior, the swap cadence and counters
    int32_t pt_T = 0;
    std::vector<double> pt_betas;              // (pt_T)
    double *pt_beta = nullptr, *pt_lo = nullptr, *pt_hi = nullptr, *pt_L = nullptr, *pt_P = nullptr, *chain_L = nullptr;
    emx_batch_log_prob_fn pr_fn = nullptr;
    void* pr_user = nullptr;
    double* cb_pr = nullptr;                   // (B, R) the caller's prior of the block
    int64_t swap_every = 1;
    unsigned long long *sw_att = nullptr, *sw_acc = nullptr;     // (B / pt_T, pt_T - 1)
    double* chain_beta = nullptr;              // (B, cap): the beta of every stored row of every member
    // the adaptive ladder (emx_pt_set_adaptation): on / off, ptemcee's lag and time, the updates made so far (t)
    int32_t pt_adapt = 0;
    double pt_lag = 10000.0, pt_time = 100.0;
    int64_t pt_updates = 0;
    // EMX_TARGET_FUSED_PT: the caller's launcher of k_pt_run around their likelihood (and prior), their device pointer, and
    // whether the launcher carries a prior functor (its answer to the probe)
    emx_pt_fused_fn ptf_fn = nullptr;
    const void* ptf_user = nullptr;
    int32_t ptf_has_prior = 0;
    // ... whose likelihood sums over the object's data (emx_pt_set_target_fused_data): the launcher carries k_pt_run's DATA form, and
    // the library's device copy of the members' counts (B values)
    bool ptf_data = false;
    int64_t* ptf_ndata = nullptr;
};

namespace {

int fail(emx_batch* b, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (b) b->err = buf;
    return code;
}

#define BNEED(b, cond, ...) \
    do { \
        if (!(cond)) return fail(b, -1, __VA_ARGS__); \
    } while (0)
#define BHIP(b, expr) \
    do { \
        hipError_t e_ = (expr); \
        if (e_ != hipSuccess) return fail(b, -2, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// splits of a move (a Gaussian move is one split of the whole ensemble)
int move_splits(const emx_move_desc& mv) { return mv.kind == EMX_MOVE_GAUSS ? 1 : (int)mv.nsplits; }

// rows of a fused user target's staging area: the largest split of the schedule
int64_t fused_stage_rows(int64_t N, int32_t nmoves, const emx_move_desc* moves) {
    int smin = 1 << 30;
    for (int m = 0; m < nmoves; ++m) smin = std::min(smin, std::max(1, move_splits(moves[m])));
    return nmoves > 0 ? (N + smin - 1) / smin : N;
}

// small_eligible's rules (emx.hip) applied to one member's shape; nullptr when the kernel takes it, else why not
const char* shape_refusal(int64_t N, int32_t D, int32_t target, int32_t nmoves, const emx_move_desc* moves, char* buf, size_t n,
                          int32_t nblobs = 0) {
    if (N < 2 || D < 1) return "nwalkers must be >= 2 and ndim >= 1";
    if (nblobs < 0 || nblobs > BATCH_MAX_BLOBS) {
        snprintf(buf, n, "a batch target carries 1 ... %d blobs a sample; got %d", BATCH_MAX_BLOBS, nblobs);
        return buf;
    }
    if (nblobs > 0 && target != EMX_TARGET_DEVICE_CALLBACK && target != EMX_TARGET_FUSED_USER && target != EMX_TARGET_FUSED_PT)
        return "blobs come from a batched callback (emx_set_batch_target_callback_blobs), a fused user target "
               "(emx_set_batch_target_fused_blobs) or a fused tempered target (emx_pt_set_target_fused_blobs): the built-in targets have none";
    if (N > 4096 || D > 256) {
        snprintf(buf, n, "nwalkers x ndim = %lld x %d is outside the one-workgroup kernel (nwalkers <= 4096, ndim <= 256)", (long long)N, D);
        return buf;
    }
    // the caller's batched log-prob (k_batch_cb); a fused tempered target takes the same schedules, and its LDS bound depends on
    // ntemps (pt_fused_refusal)
    const bool callback = target == EMX_TARGET_DEVICE_CALLBACK || target == EMX_TARGET_FUSED_PT;
    const bool fused_user = target == EMX_TARGET_FUSED_USER;         // the caller's device function inside k_small_run
    if (!callback && !fused_user && target != EMX_TARGET_ISO_GAUSS && target != EMX_TARGET_DIAG_GAUSS && target != EMX_TARGET_DENSE_GAUSS &&
        target != EMX_TARGET_ROSENBROCK && target != EMX_TARGET_BOX)
        return "the batch runs the fused device targets only (IsoGaussian, DiagGaussian, DenseGaussian, Rosenbrock, UniformBox) "
               "or a batched callback (emx_set_batch_target_callback) or a fused user target (emx_set_batch_target_fused)";
    if (nmoves < 1 || nmoves > SMALL_MAX_MOVES) {
        snprintf(buf, n, "the batch takes 1 ... %d moves; got %d", SMALL_MAX_MOVES, nmoves);
        return buf;
    }
    for (int m = 0; m < nmoves; ++m) {
        const emx_move_desc& mv = moves[m];
        if (mv.kind != EMX_MOVE_STRETCH && mv.kind != EMX_MOVE_DE && mv.kind != EMX_MOVE_SNOOKER && mv.kind != EMX_MOVE_GAUSS)
            return "the batch runs StretchMove, DEMove, DESnookerMove and GaussianMove only";
        if (mv.kind != EMX_MOVE_GAUSS && (mv.nsplits < 1 || mv.nsplits > N)) return "nsplits must be in [1, nwalkers]";
        if (mv.kind == EMX_MOVE_DE && N - (N + mv.nsplits - 1) / mv.nsplits < 2) {
            snprintf(buf, n, "DEMove with %d splits of %lld walkers: a complement has fewer than 2 walkers", mv.nsplits, (long long)N);
            return buf;
        }
        if (callback && mv.kind == EMX_MOVE_GAUSS && nmoves > 1)
            return "with a batched callback target a GaussianMove runs only as the one move of the schedule";
    }
    if (callback) return nullptr;         // k_batch_cb keeps no member in LDS
    if (fused_user) {                     // the member, at least one step's plans and the staging rows of the largest split
        const size_t need = small_lds_bytes(N, D, 0, 0, 1) + small_fused_stage_bytes(fused_stage_rows(N, nmoves, moves), D);
        if (need > SMALL_LDS_MAX) {
            snprintf(buf, n, "nwalkers x ndim = %lld x %d with a fused user target does not fit one workgroup's LDS (%zu bytes > %zu)",
                     (long long)N, D, need, SMALL_LDS_MAX);
            return buf;
        }
        if (need + small_blob_bytes(N, nblobs) > SMALL_LDS_MAX) {
            snprintf(buf, n, "nwalkers x ndim = %lld x %d with a fused user target and %d blobs a walker does not fit one workgroup's LDS "
                             "(%zu bytes > %zu; %zu without the blobs)", (long long)N, D, nblobs, need + small_blob_bytes(N, nblobs),
                     SMALL_LDS_MAX, need);
            return buf;
        }
        return nullptr;
    }
    if (target == EMX_TARGET_DENSE_GAUSS) {
        const int Dp = (D + 15) / 16 * 16;
        if (Dp > DENSE_FUSED_MAX_DP || N * (int64_t)Dp * Dp > 65536 || small_lds_bytes(N, D, Dp, 1) > SMALL_LDS_MAX) {
            snprintf(buf, n, "dense Gaussian target at %lld x %d is outside the one-workgroup kernel (nwalkers x padded ndim^2 <= 65536)",
                     (long long)N, D);
            return buf;
        }
    } else if (small_lds_bytes(N, D) > SMALL_LDS_MAX) {
        snprintf(buf, n, "nwalkers x ndim = %lld x %d does not fit one workgroup's LDS (%zu bytes > %zu)", (long long)N, D,
                 small_lds_bytes(N, D), SMALL_LDS_MAX);
        return buf;
    }
    return nullptr;
}

template <typename T>
int grow(emx_batch* b, T*& p, size_t& cap, size_t n) {
    if (n <= cap) return 0;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    BHIP(b, hipMalloc((void**)&p, n * sizeof(T)));
    cap = n;
    return 0;
}

// launch shape of a batched launch: `threads` of one workgroup and the plan steps a pass holds in LDS.  Auto: while the batch
// has no more members than the device has CUs, each member has a CU of its own and the single-ensemble (latency) shape
// is kept; beyond, the workgroup is cut to one half-step's lanes (>= one wave) with plan steps for one entry a thread, so
// that several members share a CU (32 waves, 160 KB of LDS).  Neither changes a bit: plans do not depend on the state.
// extra_lds: a fused user target's staging area, on top of small_lds_bytes.  data: a data target, whose second pass takes a
// WAVE a staged row: the cut is to a wave a row of the largest split, where G lanes a row would leave one wave for 64 / G rows.
void launch_shape(const emx_batch* b, int num_cu, const Shape& sh, int minsplits, bool dense, size_t extra_lds, int* threads, int* plan_steps,
                  bool data = false) {
    int t = small_threads(b->N, b->D, b->Dp, sh.G, minsplits, dense), ps = small_batch(b->N);
    if (b->B > num_cu) {
        const int64_t nsmax = (b->N + minsplits - 1) / minsplits;
        const int64_t want = dense ? ((nsmax + 15) / 16) * 64 : data ? nsmax * 64 : nsmax * sh.G;
        t = std::min(t, (int)std::min<int64_t>(1024, std::max<int64_t>(64, (want + 63) / 64 * 64)));
        ps = (int)std::max<int64_t>(1, std::min<int64_t>(64, t / b->N));
    }
    if (b->tune_threads > 0) t = (int)b->tune_threads;
    if (b->tune_plan_steps > 0) ps = (int)b->tune_plan_steps;
    if (dense)      // one LDS tile per wave
        while (t > 64 && small_lds_bytes(b->N, b->D, b->Dp, t / 64, ps) > SMALL_LDS_MAX) t = (t / 64 + 1) / 2 * 64;
    while (ps > 1 && small_lds_bytes(b->N, b->D, dense ? b->Dp : 0, t / 64, ps) + extra_lds > SMALL_LDS_MAX) ps = (ps + 1) / 2;
    *threads = t;
    *plan_steps = ps;
}

// the fields the three fused descriptors share (emx_fused_launch, emx_fused_batch_data_launch, emx_pt_fused_launch).  grid 0: the
// setters' probe, which carries no launch shape, stream or user pointer
template <typename DESC>
DESC fused_desc(const emx_batch* b, uint32_t abi, size_t args_bytes, int movesel, const void* args, int grid = 0, int threads = 0, size_t lds = 0,
                const void* user = nullptr) {
    DESC fl{};
    fl.abi = abi;
    fl.args_bytes = (uint32_t)args_bytes;
    fl.ndim = b->D;
    fl.movesel = movesel;
    fl.grid = grid;
    fl.threads = threads;
    fl.lds_bytes = lds;
    fl.hip_stream = grid ? (void*)b->stream : nullptr;
    fl.args = args;
    fl.user = user;
    return fl;
}

// what a fused user target's launcher answered (include/emx.h: emx_fused_batch_fn), as the handle's error; 0: it launched (or probed).
// nblobs: the count that answer 4 is about
int fused_refusal(emx_batch* b, int rc, int movesel, int nblobs, bool data = false) {
    if (rc == 0) return 0;
    if (rc == 1 && data)
        return fail(b, -8, "the fused user target's launcher was built against another version of emx_fused_target_data.hpp (the library "
                           "has EMX_FUSED_BATCH_DATA_ABI 0x%x and %zu bytes of kernel arguments): rebuild it with this library's headers",
                    (unsigned)EMX_FUSED_BATCH_DATA_ABI, sizeof(SmallRunArgs));
    if (rc == 1)
        return fail(b, -8, "the fused user target's launcher was built against another version of emx_fused_target.hpp (the library has "
                           "EMX_FUSED_ABI %u and %zu bytes of kernel arguments): rebuild it with this library's headers",
                    (unsigned)EMX_FUSED_ABI, sizeof(SmallRunArgs));
    if (rc == 2) return fail(b, -1, "the fused user target's launcher was compiled for another ndim than the batch's %d", b->D);
    if (rc == 4)
        return fail(b, -1, "the fused user target's launcher was compiled for another number of blobs than the %d asked for "
                           "(EMX_FUSED_BATCH_TARGET_BLOBS's nblobs; EMX_FUSED_BATCH_TARGET has none)", nblobs);
    if (rc == 3)
        return fail(b, -1, "the fused user target's launcher does not carry the kernel of this schedule (move selector %d): compile it with "
                           "EMX_FUSED_MOVES_ANY", movesel);
    if (rc >= 100)
        return fail(b, -2, "k_small_run fused user target launch failed (ndim=%d): %s", b->D, hipGetErrorString((hipError_t)(rc - 100)));
    return fail(b, -7, "the fused user target's launcher failed (returned %d)", rc);
}

// one launch: `nsteps` steps (nsteps 0 with eval0: the initial log-probs only)
int launch(emx_batch* b, int64_t i0, int64_t nsteps, int32_t thin_by, int32_t store, bool eval0) {
    const int nm = (int)b->moves.size();
    const bool dense = b->target == EMX_TARGET_DENSE_GAUSS;
    const Shape sh = pick_shape(b->D, dense ? b->Dp : b->D);
    SmallRunArgs a{};
    int minsplits = 64;
    bool any_gauss = false;
    for (int m = 0; m < nm; ++m) {
        const emx_move_desc& mv = b->moves[m];
        a.kind[m] = mv.kind;
        a.nsplits[m] = mv.nsplits;
        a.a[m] = mv.a;
        a.sigma[m] = mv.sigma;
        a.g0[m] = mv.g0;
        a.gammas[m] = mv.gammas;
        a.cdf[m] = b->cdf[m];
        a.gmode[m] = mv.reserved;
        a.gsigma[m] = mv.sigma;
        a.gscale[m] = b->mscale[m];
        any_gauss = any_gauss || mv.kind == EMX_MOVE_GAUSS;
        minsplits = std::min(minsplits, (int)mv.nsplits);
    }
    a.nmoves = nm;
    a.X = b->X;
    a.lp = b->lp;
    a.acc = b->acc;
    a.acc_count = b->acc_count;
    a.status = b->status;
    if (store && nsteps > 0) {
        a.chain = b->chain + (size_t)b->stored * b->N * b->D;
        a.chain_lp = b->chain_lp + (size_t)b->stored * b->N;
    }
    a.cap = b->cap;
    a.tp0 = b->tp0;
    a.tp1 = b->tp1;
    a.tp0_stride = b->tp0_stride;
    a.tp1_stride = b->tp1_stride;
    a.tscales = b->tscales;
    a.seeds = b->seeds;
    a.step0 = b->step;
    a.i0 = i0;
    a.N = (int32_t)b->N;
    a.D = b->D;
    a.target = b->target;
    a.nsteps = (int32_t)nsteps;
    a.thin_by = thin_by;
    a.store = store;
    a.eval0 = eval0 ? 1 : 0;
    if (any_gauss && nsteps > 0) {
        // per member and step the step-size factor (a function of the member's seed and the step: run_small's arithmetic),
        // per step the sequential mode's column (a function of the step alone: one cursor for every member)
        std::vector<double> facs((size_t)b->B * nsteps, 1.0);
        std::vector<int32_t> cols((size_t)nsteps, 0);
        for (int64_t s2 = 0; s2 < nsteps; ++s2) {
            const uint64_t step = b->step + (uint64_t)s2;
            for (int32_t mb = 0; mb < b->B; ++mb) {
                const uint64_t seed = b->seeds_host[mb];
                const int mi = nm == 1 ? 0 : native_move_choice(seed, step, b->cdf.data(), nm);
                const emx_move_desc& mv = b->moves[mi];
                if (mv.kind != EMX_MOVE_GAUSS || mv.a == 0.0) continue;
                const Philox4 r = philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), 0x46414354u /*'FACT'*/, 0, (uint32_t)seed,
                                                (uint32_t)(seed >> 32));
                facs[(size_t)mb * nsteps + s2] = std::exp(-mv.g0 + 2.0 * mv.g0 * u53(r.v[0], r.v[1]));
            }
        }
        // the sequential cursor advances on the steps that draw a Gaussian move -- the same steps for every member only when
        // the move choice does not depend on the seed, i.e. with one move (emx_batch_set_moves refuses the other case)
        for (int64_t s2 = 0; s2 < nsteps; ++s2) {
            emx_move_desc& mv = b->moves[0];
            if (mv.kind == EMX_MOVE_GAUSS && mv.reserved == EMX_GAUSS_SEQUENTIAL) {
                cols[s2] = (int32_t)((int64_t)mv.gammas % b->D);
                mv.gammas = (double)(((int64_t)mv.gammas + 1) % b->D);
            }
        }
        BHIP(b, hipStreamSynchronize(b->stream));        // the previous launch no longer reads the buffers
        if (grow(b, b->fac_dev, b->fac_cap, facs.size())) return -2;
        if (grow(b, b->col_dev, b->col_cap, cols.size())) return -2;
        BHIP(b, hipMemcpy(b->fac_dev, facs.data(), facs.size() * 8, hipMemcpyHostToDevice));
        BHIP(b, hipMemcpy(b->col_dev, cols.data(), cols.size() * 4, hipMemcpyHostToDevice));
        a.step_fac = b->fac_dev;
        a.step_col = b->col_dev;
    }
    hipDeviceProp_t prop;
    int num_cu = 256;
    if (hipGetDeviceProperties(&prop, b->device) == hipSuccess) num_cu = prop.multiProcessorCount;
    const bool fused_user = b->target == EMX_TARGET_FUSED_USER;
    const bool fused_data = fused_user && b->fused_data_fn != nullptr;
    if (fused_user) {
        BNEED(b, fused_data || b->fused_fn != nullptr, "fused user target without a launcher (emx_set_batch_target_fused)");
        BNEED(b, !fused_data || (b->fused_ndata != nullptr && b->nblobs == 0), "data target without its counts (emx_set_batch_target_fused_data)");
        a.target = TGT_USER;
        a.user = b->fused_user;
        a.stage_rows = (int32_t)fused_stage_rows(b->N, nm, b->moves.data());
        if (b->nblobs > 0) {
            a.nblobs = b->nblobs;
            a.blobs = b->blobs;
            if (store && nsteps > 0) {
                BNEED(b, b->chain_blobs != nullptr, "no blob plane (emx_batch_chain_config)");
                a.chain_blobs = b->chain_blobs + (size_t)b->stored * b->N * b->nblobs;
            }
        }
    }
    const size_t extra_lds = fused_user ? small_fused_stage_bytes(a.stage_rows, b->D) + small_blob_bytes(b->N, b->nblobs) : 0;
    int threads = 0, plan_steps = 0;
    launch_shape(b, num_cu, sh, minsplits, dense, extra_lds, &threads, &plan_steps, fused_data);
    a.batch = plan_steps;
    const size_t lds = small_lds_bytes(b->N, b->D, dense ? b->Dp : 0, threads / 64, plan_steps) + extra_lds;
    BNEED(b, lds <= SMALL_LDS_MAX && threads >= 64 && threads <= 1024 && threads % 64 == 0,
          "batch launch shape: %d threads and %d plan steps need %zu bytes of LDS", threads, plan_steps, lds);
    // (a fused user target's translation unit carries the single-StretchMove selector and the any-schedule one)
    const int movesel = (nm == 1 && ((!dense && !fused_user) || b->moves[0].kind == EMX_MOVE_STRETCH)) ? (int)b->moves[0].kind : SMALL_ANY_MOVE;
    if (fused_data) {
        auto fl = fused_desc<emx_fused_batch_data_launch>(b, EMX_FUSED_BATCH_DATA_ABI, sizeof(SmallRunArgs), movesel, &a, b->B, threads, lds, b->fused_user);
        fl.ndata = b->fused_ndata;
        if (int rc = fused_refusal(b, b->fused_data_fn(&fl), movesel, 0, true)) return rc;
    } else if (fused_user) {
        auto fl = fused_desc<emx_fused_launch>(b, EMX_FUSED_ABI, sizeof(SmallRunArgs), movesel, &a, b->B, threads, lds, b->fused_user);
        fl.nblobs = b->nblobs;
        if (int rc = fused_refusal(b, b->fused_fn(&fl), movesel, b->nblobs)) return rc;
    } else {
        const hipError_t e = small_dispatch<true>(sh.G, sh.V, sh.CH, dense ? b->Dp / 16 : 0, movesel, b->B, threads, lds, b->stream, a);
        if (e != hipSuccess)
            return fail(b, -2, "k_small_run batch launch failed (G=%d V=%d CH=%d ndim=%d): %s", sh.G, sh.V, sh.CH, b->D, hipGetErrorString(e));
    }
    b->last_threads = threads;
    b->last_plan_steps = plan_steps;
    ++b->launches;
    if (nsteps > 0) {
        int64_t nstored = 0;
        if (store)
            for (int64_t s2 = 0; s2 < nsteps; ++s2) nstored += ((i0 + s2 + 1) % thin_by == 0) ? 1 : 0;
        b->stored += nstored;
        b->proposals += nsteps;
        b->step += (uint64_t)nsteps;
    }
    return 0;
}

// ---- fused tempered targets (EMX_TARGET_FUSED_PT; emx_pt_fused.hpp) ----

// staging rows a rung: the largest split, halved until the object fits with one plan step (k_pt_run then runs a half-step in chunks)
int64_t pt_stage_rows(int32_t T, int64_t N, int32_t D, int32_t nmoves, const emx_move_desc* moves, int32_t nblobs = 0) {
    int64_t R = fused_stage_rows(N, nmoves, moves);
    while (R > 1 && pt_lds_layout(T, N, D, 1, R, nblobs).total > SMALL_LDS_MAX) R = (R + 1) / 2;
    return R;
}

// one workgroup's LDS for an object of T rungs with `plan_steps` plan steps; the staging rows a rung: the largest split
size_t pt_fused_lds(int32_t T, int64_t N, int32_t D, int32_t nmoves, const emx_move_desc* moves, int plan_steps, int32_t nblobs = 0) {
    return pt_lds_layout(T, N, D, plan_steps, pt_stage_rows(T, N, D, nmoves, moves, nblobs), nblobs).total;
}

// nullptr when one workgroup holds the object with at least one plan step, else why not (the bytes needed)
// (nblobs > 0: a shape that fits only without the blobs is refused in words of its own)
const char* pt_fused_refusal(int32_t T, int64_t N, int32_t D, int32_t nmoves, const emx_move_desc* moves, char* buf, size_t n,
                             int32_t nblobs = 0) {
    if (T < 1) return "ntemps must be >= 1";
    if (const char* why = shape_refusal(N, D, EMX_TARGET_FUSED_PT, nmoves, moves, buf, n, nblobs)) return why;
    // (the coordinates alone bound T N D: the products below stay far inside 64 bits)
    const double coords = (double)T * (double)N * (double)D * 8.0;
    const size_t need = coords > 1e12 ? (size_t)1 << 40 : pt_fused_lds(T, N, D, nmoves, moves, 1);
    if (need > SMALL_LDS_MAX) {
        snprintf(buf, n, "ntemps x nwalkers x ndim = %d x %lld x %d with a fused tempered target does not fit one workgroup's LDS (%zu "
                         "bytes > %zu): an object is not split across workgroups; run it on the callback path (targets.BatchKernel)",
                 T, (long long)N, D, need, SMALL_LDS_MAX);
        return buf;
    }
    if (nblobs > 0) {
        const size_t with = pt_fused_lds(T, N, D, nmoves, moves, 1, nblobs);
        if (with > SMALL_LDS_MAX) {
            snprintf(buf, n, "ntemps x nwalkers x ndim = %d x %lld x %d with a fused tempered target and %d blobs a walker does not fit one "
                             "workgroup's LDS (%zu bytes > %zu; %zu without the blobs): run it on the callback path (targets.BatchKernel)",
                     T, (long long)N, D, nblobs, with, SMALL_LDS_MAX, need);
            return buf;
        }
    }
    return nullptr;
}

// what a fused tempered target's launcher answered, as the handle's error; 0: it launched (or probed)
int pt_fused_launcher_refusal(emx_batch* b, int rc, int movesel, bool data = false, int nblobs = 0) {
    if (rc == 0) return 0;
    if (rc == 4)
        return fail(b, -1, "the fused tempered target's launcher was compiled for another number of blobs than the %d asked for "
                           "(EMX_FUSED_PT_TARGET_BLOBS's nblobs; EMX_FUSED_PT_TARGET and the data form have none)", nblobs);
    if (rc == 1 && data)
        return fail(b, -8, "the fused tempered data target's launcher was built against another version of emx_pt_fused_data.hpp, or is "
                           "not an EMX_FUSED_PT_DATA_TARGET launcher (the library has EMX_FUSED_PT_DATA_ABI 0x%x and %zu bytes of kernel "
                           "arguments): rebuild it with this library's headers",
                    (unsigned)EMX_FUSED_PT_DATA_ABI, sizeof(PtRunArgs));
    if (rc == 1)
        return fail(b, -8, "the fused tempered target's launcher was built against another version of emx_pt_fused.hpp (the library has "
                           "EMX_FUSED_PT_ABI %u and %zu bytes of kernel arguments): rebuild it with this library's headers",
                    (unsigned)EMX_FUSED_PT_ABI, sizeof(PtRunArgs));
    if (rc == 2) return fail(b, -1, "the fused tempered target's launcher was compiled for another ndim than the batch's %d", b->D);
    if (rc == 3)
        return fail(b, -1, "the fused tempered target's launcher does not carry the kernel of this schedule (move selector %d): compile it "
                           "with EMX_FUSED_MOVES_ANY", movesel);
    if (rc >= 100) return fail(b, -2, "k_pt_run launch failed (ndim=%d): %s", b->D, hipGetErrorString((hipError_t)(rc - 100)));
    return fail(b, -7, "the fused tempered target's launcher failed (returned %d)", rc);
}

// one launch of k_pt_run: `nsteps` steps of every object (nsteps 0 with eval0: the initial P, L and lp only).  The launch shape
// follows launch_shape's rule for the rows of one half-step of ALL rungs, plan steps for one entry a thread, shrunk to fit.
int launch_pt(emx_batch* b, int64_t i0, int64_t nsteps, int32_t thin_by, int32_t store, bool eval0) {
    BNEED(b, b->ptf_fn != nullptr, "fused tempered target without a launcher (emx_pt_set_target_fused)");
    BNEED(b, !b->ptf_data || b->ptf_ndata != nullptr, "fused tempered data target without its counts (emx_pt_set_target_fused_data)");
    BNEED(b, b->pt_T > 0, "a fused tempered target runs on a tempered handle (emx_pt_set_tempering)");
    const int nm = (int)b->moves.size();
    const int32_t T = b->pt_T;
    PtRunArgs a{};
    int smin = 1 << 30, smax = 0;
    bool any_gauss = false;
    for (int m = 0; m < nm; ++m) {
        const emx_move_desc& mv = b->moves[m];
        smin = std::min(smin, move_splits(mv));
        smax = std::max(smax, move_splits(mv));
        any_gauss = any_gauss || mv.kind == EMX_MOVE_GAUSS;
        a.kind[m] = mv.kind;
        a.nsplits[m] = mv.nsplits;
        a.a[m] = mv.a;
        a.sigma[m] = mv.sigma;
        a.g0[m] = mv.g0;
        a.gammas[m] = mv.gammas;
        a.cdf[m] = b->cdf[m];
        a.gmode[m] = mv.reserved;
        a.gsigma[m] = mv.sigma;
        a.gscale[m] = b->mscale[m];
    }
    a.nmoves = nm;
    a.smax = smax;
    a.X = b->X;
    a.lp = b->lp;
    a.L = b->pt_L;
    a.P = b->pt_P;
    a.beta = b->pt_beta;
    a.acc = b->acc;
    a.acc_count = b->acc_count;
    a.status = b->status;
    a.seeds = b->seeds;
    a.attempts = b->sw_att;
    a.accepts = b->sw_acc;
    a.chain = b->chain;
    a.chain_lp = b->chain_lp;
    a.chain_L = b->chain_L;
    a.chain_beta = b->chain_beta;
    a.cap = b->cap;
    a.row0 = b->stored;
    a.box_lo = b->pt_lo;
    a.box_hi = b->pt_hi;
    a.step0 = b->step;
    a.i0 = i0;
    a.T = T;
    a.N = (int32_t)b->N;
    a.D = b->D;
    a.nsteps = (int32_t)nsteps;
    a.thin_by = thin_by;
    a.store = (store && nsteps > 0) ? 1 : 0;
    a.eval0 = eval0 ? 1 : 0;
    a.stage_rows = (int32_t)pt_stage_rows(T, b->N, b->D, nm, b->moves.data());
    a.max_rows = (int32_t)fused_stage_rows(b->N, nm, b->moves.data());
    a.swap_every = b->swap_every;
    a.adapt = b->pt_adapt ? 1 : 0;
    a.lag = b->pt_lag;
    a.time = b->pt_time;
    a.adapt_t0 = (long long)b->pt_updates;
    a.user = b->ptf_user;
    a.ndata = b->ptf_data ? reinterpret_cast<const long long*>(b->ptf_ndata) : nullptr;
    const int32_t K = b->nblobs;
    if (K > 0) {
        BNEED(b, !b->ptf_data && b->blobs != nullptr, "fused tempered target with blobs without their storage (emx_pt_set_target_fused_blobs)");
        BNEED(b, !a.store || b->chain_blobs != nullptr, "no blob plane (emx_batch_chain_config)");
        a.nblobs = K;
        a.blobs = b->blobs;
        a.chain_blobs = b->chain_blobs;
        a.stage_rows = (int32_t)pt_stage_rows(T, b->N, b->D, nm, b->moves.data(), K);
    }
    if (any_gauss && nsteps > 0) {
        // the step-size factors and the sequential column: launch's host arithmetic
        std::vector<double> facs((size_t)b->B * nsteps, 1.0);
        std::vector<int32_t> cols((size_t)nsteps, 0);
        for (int64_t s2 = 0; s2 < nsteps; ++s2) {
            const uint64_t step = b->step + (uint64_t)s2;
            for (int32_t mb = 0; mb < b->B; ++mb) {
                const uint64_t seed = b->seeds_host[mb];
                const int mi = nm == 1 ? 0 : native_move_choice(seed, step, b->cdf.data(), nm);
                const emx_move_desc& mv = b->moves[mi];
                if (mv.kind != EMX_MOVE_GAUSS || mv.a == 0.0) continue;
                const Philox4 r = philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), 0x46414354u /*'FACT'*/, 0, (uint32_t)seed,
                                                (uint32_t)(seed >> 32));
                facs[(size_t)mb * nsteps + s2] = std::exp(-mv.g0 + 2.0 * mv.g0 * u53(r.v[0], r.v[1]));
            }
            emx_move_desc& mv = b->moves[0];
            if (mv.kind == EMX_MOVE_GAUSS && mv.reserved == EMX_GAUSS_SEQUENTIAL) {
                cols[s2] = (int32_t)((int64_t)mv.gammas % b->D);
                mv.gammas = (double)(((int64_t)mv.gammas + 1) % b->D);
            }
        }
        BHIP(b, hipStreamSynchronize(b->stream));        // the previous launch no longer reads the buffers
        if (grow(b, b->fac_dev, b->fac_cap, facs.size())) return -2;
        if (grow(b, b->col_dev, b->col_cap, cols.size())) return -2;
        BHIP(b, hipMemcpy(b->fac_dev, facs.data(), facs.size() * 8, hipMemcpyHostToDevice));
        BHIP(b, hipMemcpy(b->col_dev, cols.data(), cols.size() * 4, hipMemcpyHostToDevice));
        a.step_fac = b->fac_dev;
        a.step_col = b->col_dev;
    }
    const Shape sh = pick_shape(b->D, b->D);
    const int64_t rows = (int64_t)T * a.stage_rows;
    int threads = (int)std::min<int64_t>(PT_RUN_MAX_THREADS, std::max<int64_t>(64, (rows * sh.G + 63) / 64 * 64));
    if (b->ptf_data) threads = (int)std::min<int64_t>(PT_RUN_MAX_THREADS, std::max<int64_t>(64, rows * 64));      // a wave a row
    int plan_steps = (int)std::max<int64_t>(1, std::min<int64_t>(64, threads / ((int64_t)T * b->N)));
    if (b->tune_threads > 0) threads = (int)b->tune_threads;
    if (b->tune_plan_steps > 0) plan_steps = (int)b->tune_plan_steps;
    while (plan_steps > 1 && pt_fused_lds(T, b->N, b->D, nm, b->moves.data(), plan_steps, K) > SMALL_LDS_MAX) plan_steps = (plan_steps + 1) / 2;
    a.plan_steps = plan_steps;
    const size_t lds = pt_fused_lds(T, b->N, b->D, nm, b->moves.data(), plan_steps, K);
    BNEED(b, threads <= PT_RUN_MAX_THREADS, "batch_threads: at most %d with a fused tempered target", PT_RUN_MAX_THREADS);
    BNEED(b, lds <= SMALL_LDS_MAX && threads >= 64 && threads % 64 == 0,
          "fused tempered launch shape: %d threads and %d plan steps need %zu bytes of LDS", threads, plan_steps, lds);
    const int movesel = (nm == 1 && b->moves[0].kind == EMX_MOVE_STRETCH) ? (int)EMX_MOVE_STRETCH : SMALL_ANY_MOVE;
    auto fl = fused_desc<emx_pt_fused_launch>(b, b->ptf_data ? EMX_FUSED_PT_DATA_ABI : EMX_FUSED_PT_ABI, sizeof(PtRunArgs), movesel, &a, b->B / T, threads,
                                              lds, b->ptf_user);
    fl.nblobs = K;
    if (int rc = pt_fused_launcher_refusal(b, b->ptf_fn(&fl), movesel, b->ptf_data, K)) return rc;
    b->last_threads = threads;
    b->last_plan_steps = plan_steps;
    ++b->launches;
    if (nsteps > 0) {
        int64_t nstored = 0, npass = 0;
        for (int64_t s2 = 0; s2 < nsteps; ++s2) {
            if (store && (i0 + s2 + 1) % thin_by == 0) ++nstored;
            if (b->swap_every > 0 && (b->step + (uint64_t)s2 + 1) % (uint64_t)b->swap_every == 0) ++npass;
        }
        if (b->pt_adapt) b->pt_updates += npass;      // one update a pass, as swap_pass counts them
        b->stored += nstored;
        b->proposals += nsteps;
        b->step += (uint64_t)nsteps;
    }
    return 0;
}

// ---- the caller's batched log-prob (EMX_TARGET_DEVICE_CALLBACK) ----

// the caller's function on `rows` rows of every member: coords (B, rows, D) -> log_prob (B, rows), enqueued on the stream
// (a target with blobs: and their blobs (B, rows, nblobs) -> blobs_out)
int call_back(emx_batch* b, const double* coords, int64_t rows, double* out, double* blobs_out = nullptr) {
    const int rc = b->nblobs > 0 ? b->cbb_fn(b->cb_user, coords, b->B, rows, b->D, out, b->nblobs, blobs_out, (void*)b->stream)
                                 : b->cb_fn(b->cb_user, coords, b->B, rows, b->D, out, (void*)b->stream);
    if (rc != 0) return fail(b, -7, "the batched device log-prob callback failed (returned %d)", rc);
    return 0;
}

// the caller's prior (emx_set_batch_prior_callback) on `rows` rows of every member
int call_prior(emx_batch* b, const double* coords, int64_t rows, double* out) {
    const int rc = b->pr_fn(b->pr_user, coords, b->B, rows, b->D, out, (void*)b->stream);
    if (rc != 0) return fail(b, -7, "the batched device log-prior callback failed (returned %d)", rc);
    return 0;
}

// a ladder row of group g (betas[0 ... T - 1]) as emx_pt_set_tempering checks it, plus betas[0 ... T - 2] > 0 when adapting
int check_ladder_row(emx_batch* b, const double* betas, int32_t T, int64_t g, bool adapting) {
    BNEED(b, betas[0] == 1.0, "group %lld: betas[0] must be 1", (long long)g);
    for (int t = 0; t < T; ++t) {
        BNEED(b, betas[t] >= 0.0 && betas[t] <= 1.0, "group %lld: betas must lie in [0, 1]; betas[%d] = %g", (long long)g, t, betas[t]);
        if (t > 0) BNEED(b, betas[t] <= betas[t - 1], "group %lld: betas must not increase (betas[%d] = %g, betas[%d] = %g)",
                         (long long)g, t - 1, betas[t - 1], t, betas[t]);
        if (adapting && t < T - 1) BNEED(b, betas[t] > 0.0, "group %lld: an adaptive ladder needs betas[%d] > 0", (long long)g, t);
    }
    return 0;
}

// one k_pt_swap launch after Philox step `step`: the swap pass (swap) and / or the stored rows of chain row `row` (-1: none)
int swap_pass(emx_batch* b, uint64_t step, int64_t row, bool swap) {
    PtSwapArgs s{};
    s.X = b->X;
    s.lp = b->lp;
    s.L = b->pt_L;
    s.P = b->pt_P;
    s.beta = b->pt_beta;
    s.seeds = b->seeds;
    s.attempts = b->sw_att;
    s.accepts = b->sw_acc;
    s.chain = b->chain;
    s.chain_lp = b->chain_lp;
    s.chain_L = b->chain_L;
    s.cap = b->cap;
    s.chain_row = row;
    s.swap = swap ? 1 : 0;
    s.T = b->pt_T;
    s.N = (int32_t)b->N;
    s.D = b->D;
    s.step = step;
    s.chain_beta = b->chain_beta;
    s.adapt = swap && b->pt_adapt ? 1 : 0;
    s.lag = b->pt_lag;
    s.time = b->pt_time;
    s.adapt_t = (long long)b->pt_updates;
    if (b->nblobs > 0) {
        BNEED(b, b->blobs != nullptr && (row < 0 || b->chain_blobs != nullptr), "no blob plane (emx_batch_chain_config)");
        s.blobs = b->blobs;
        s.chain_blobs = b->chain_blobs;
        s.nblobs = b->nblobs;
    }
    BHIP(b, pt_swap_launch(b->B / b->pt_T, b->stream, s));
    ++b->launches;
    if (s.adapt) ++b->pt_updates;
    return 0;
}

// the initial log-probs: one call on the whole state, then the per-member NaN check
int eval_callback(emx_batch* b) {
    BNEED(b, b->cb_fn != nullptr || b->cbb_fn != nullptr, "device callback target without a callback (emx_set_batch_target_callback)");
    if (b->pt_T > 0) {       // tempered: P (the caller's prior, the box or 0), L, then lp and the NaN check in one launch
        if (b->pr_fn) {
            if (int rc = call_prior(b, b->X, b->N, b->pt_P)) return rc;
        } else {
            BHIP(b, hipMemsetAsync(b->pt_P, 0, (size_t)b->B * b->N * 8, b->stream));
        }
        if (int rc = call_back(b, b->X, b->N, b->pt_L, b->blobs)) return rc;      // the state's blobs by the same call
        BHIP(b, pt_init_launch(b->X, b->lp, b->pt_L, b->pt_P, b->pt_beta, b->pr_fn ? nullptr : b->pt_lo, b->pt_hi, b->status, b->B,
                               (int32_t)b->N, b->D, b->stream, b->blobs, b->nblobs));
        ++b->launches;
        return 0;
    }
    if (int rc = call_back(b, b->X, b->N, b->lp, b->blobs)) return rc;      // the state's blobs by the same call
    BHIP(b, batch_lp_check(b->lp, b->status, b->B, (int32_t)b->N, b->stream));
    ++b->launches;
    return 0;
}

// `total` proposal steps: per step and phase k < S_max one k_batch_cb launch (commit phase k - 1, propose phase k) and one call of
// the caller's function on the (B, R, D) block; one commit-only launch at the end.  Nothing is synchronised inside the loop
// except, with Gaussian moves, the upload of the step-size factors once per chunk of steps (as the fused path does).
int run_callback(emx_batch* b, int64_t total, int32_t thin_by, int32_t store) {
    BNEED(b, b->cb_fn != nullptr || b->cbb_fn != nullptr, "device callback target without a callback (emx_set_batch_target_callback)");
    if (total == 0) return 0;
    const int nm = (int)b->moves.size();
    int smin = 1 << 30, smax = 0;
    bool any_gauss = false;
    BatchCbArgs a{};
    for (int m = 0; m < nm; ++m) {
        const emx_move_desc& mv = b->moves[m];
        smin = std::min(smin, move_splits(mv));
        smax = std::max(smax, move_splits(mv));
        any_gauss = any_gauss || mv.kind == EMX_MOVE_GAUSS;
        a.kind[m] = mv.kind;
        a.nsplits[m] = mv.nsplits;
        a.a[m] = mv.a;
        a.sigma[m] = mv.sigma;
        a.g0[m] = mv.g0;
        a.gammas[m] = mv.gammas;
        a.cdf[m] = b->cdf[m];
        a.gmode[m] = mv.reserved;
        a.gsigma[m] = mv.sigma;
        a.gscale[m] = b->mscale[m];
    }
    const int64_t R = (b->N + smin - 1) / smin;
    const size_t rows = (size_t)b->B * R;
    if (rows > b->cb_rows) {
        BHIP(b, hipStreamSynchronize(b->stream));
        for (void* p : {(void*)b->cb_q, (void*)b->cb_lp, (void*)b->cb_fac, (void*)b->cb_logu, (void*)b->cb_wi, (void*)b->cb_pr, (void*)b->cb_bq})
            if (p) hipFree(p);
        b->cb_q = b->cb_lp = b->cb_fac = b->cb_logu = b->cb_pr = b->cb_bq = nullptr;
        b->cb_wi = nullptr;
        b->cb_rows = 0;
        BHIP(b, hipMalloc((void**)&b->cb_q, rows * b->D * 8));
        BHIP(b, hipMalloc((void**)&b->cb_lp, rows * 8));
        BHIP(b, hipMalloc((void**)&b->cb_fac, rows * 8));
        BHIP(b, hipMalloc((void**)&b->cb_logu, rows * 8));
        BHIP(b, hipMalloc((void**)&b->cb_wi, rows * 4));
        b->cb_rows = rows;
    }
    if (!b->cb_nrows) BHIP(b, hipMalloc((void**)&b->cb_nrows, (size_t)b->B * 4));
    if (b->nblobs > 0) {
        if (!b->cb_bq) BHIP(b, hipMalloc((void**)&b->cb_bq, b->cb_rows * b->nblobs * 8));
        BNEED(b, !store || b->chain_blobs != nullptr, "no blob plane (emx_batch_chain_config)");
        a.nblobs = b->nblobs;
        a.bq = b->cb_bq;
        a.blobs = b->blobs;
        a.chain_blobs = b->chain_blobs;
    }
    a.nmoves = nm;
    a.X = b->X;
    a.lp = b->lp;
    a.acc = b->acc;
    a.acc_count = b->acc_count;
    a.status = b->status;
    a.chain = b->chain;
    a.chain_lp = b->chain_lp;
    a.cap = b->cap;
    a.q = b->cb_q;
    a.lpq = b->cb_lp;
    a.fac = b->cb_fac;
    a.logu = b->cb_logu;
    a.wi = b->cb_wi;
    a.nrows = b->cb_nrows;
    a.seeds = b->seeds;
    a.N = (int32_t)b->N;
    a.D = b->D;
    a.R = (int32_t)R;
    const bool pt = b->pt_T > 0;
    if (pt) {
        if (b->pr_fn && !b->cb_pr) BHIP(b, hipMalloc((void**)&b->cb_pr, b->cb_rows * 8));
        a.beta = b->pt_beta;
        a.box_lo = b->pt_lo;
        a.box_hi = b->pt_hi;
        a.lpr = b->pr_fn ? b->cb_pr : nullptr;
        a.L = b->pt_L;
        a.P = b->pt_P;
        a.chain_L = b->chain_L;
        a.chain_beta = b->chain_beta;
    }
    const Shape sh = pick_shape(b->D, b->D);
    // one phase's rows in one pass (R G lanes); no bit depends on the shape
    int threads = (int)std::min<int64_t>(CB_MAX_THREADS, std::max<int64_t>(64, (R * sh.G + 63) / 64 * 64));
    if (b->tune_threads > 0) threads = (int)b->tune_threads;
    BNEED(b, threads <= CB_MAX_THREADS, "batch_threads: at most %d with a batched callback target", CB_MAX_THREADS);
    b->last_threads = threads;
    b->last_plan_steps = 0;
    const int64_t most = any_gauss ? std::max<int64_t>(1, std::min<int64_t>(4096, (4 << 20) / b->B)) : total;
    int64_t stored_row = -1, nstored = 0;     // chain row of the pending phase's step
    bool pending = false, pending_swap = false;
    auto launch_cb = [&](bool propose, int phase, uint64_t step) -> int {
        a.commit = pending ? 1 : 0;
        a.chain_row = stored_row;
        a.rows_in_commit = pending_swap ? 0 : 1;
        a.propose = propose ? 1 : 0;
        a.phase = phase;
        a.step = step;
        const hipError_t e = batch_cb_dispatch(sh.G, sh.V, sh.CH, b->B, threads, b->stream, a);
        if (e != hipSuccess)
            return fail(b, -2, "k_batch_cb launch failed (G=%d V=%d CH=%d ndim=%d): %s", sh.G, sh.V, sh.CH, b->D, hipGetErrorString(e));
        ++b->launches;
        return 0;
    };
    for (int64_t i = 0; i < total;) {
        const int64_t chunk = std::min<int64_t>(total - i, most);
        std::vector<int32_t> cols((size_t)chunk, 0);
        if (any_gauss) {
            // the step-size factors and the sequential column: the fused path's host arithmetic (launch)
            std::vector<double> facs((size_t)b->B * chunk, 1.0);
            for (int64_t s2 = 0; s2 < chunk; ++s2) {
                const uint64_t step = b->step + (uint64_t)(i + s2);
                for (int32_t mb = 0; mb < b->B; ++mb) {
                    const uint64_t seed = b->seeds_host[mb];
                    const int mi = nm == 1 ? 0 : native_move_choice(seed, step, b->cdf.data(), nm);
                    const emx_move_desc& mv = b->moves[mi];
                    if (mv.kind != EMX_MOVE_GAUSS || mv.a == 0.0) continue;
                    const Philox4 r = philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), 0x46414354u /*'FACT'*/, 0, (uint32_t)seed,
                                                    (uint32_t)(seed >> 32));
                    facs[(size_t)mb * chunk + s2] = std::exp(-mv.g0 + 2.0 * mv.g0 * u53(r.v[0], r.v[1]));
                }
                emx_move_desc& mv = b->moves[0];
                if (mv.kind == EMX_MOVE_GAUSS && mv.reserved == EMX_GAUSS_SEQUENTIAL) {
                    cols[s2] = (int32_t)((int64_t)mv.gammas % b->D);
                    mv.gammas = (double)(((int64_t)mv.gammas + 1) % b->D);
                }
            }
            BHIP(b, hipStreamSynchronize(b->stream));        // the previous chunk's launches no longer read the factors
            if (grow(b, b->fac_dev, b->fac_cap, facs.size())) return -2;
            BHIP(b, hipMemcpy(b->fac_dev, facs.data(), facs.size() * 8, hipMemcpyHostToDevice));
            a.gfac_stride = chunk;
        }
        for (int64_t s2 = 0; s2 < chunk; ++s2) {
            const int64_t s = i + s2;
            const uint64_t step = b->step + (uint64_t)s;
            a.gfac = any_gauss ? b->fac_dev + s2 : nullptr;
            a.gcol = cols[s2];
            const int64_t row = (store && (s + 1) % thin_by == 0) ? b->stored + nstored : -1;
            const bool swap = pt && b->swap_every > 0 && (step + 1) % (uint64_t)b->swap_every == 0;
            for (int k = 0; k < smax; ++k) {
                if (int rc = launch_cb(true, k, step)) return rc;
                if (pt && b->pr_fn)                  // the prior first, on the same block
                    if (int rc = call_prior(b, b->cb_q, R, b->cb_pr)) return rc;
                if (int rc = call_back(b, b->cb_q, R, b->cb_lp, b->cb_bq)) return rc;
                pending = true;
                pending_swap = swap;
                stored_row = row;
            }
            if (swap) {                          // commit the last phase, then the swap pass (it writes the stored rows)
                if (int rc = launch_cb(false, 0, 0)) return rc;
                pending = pending_swap = false;
                if (int rc = swap_pass(b, step, row, true)) return rc;
            }
            if (row >= 0) ++nstored;
        }
        i += chunk;
    }
    if (pending)
        if (int rc = launch_cb(false, 0, 0)) return rc;      // commit the last phase
    b->stored += nstored;
    b->proposals += total;
    b->step += (uint64_t)total;
    return 0;
}

// the handle's blob count becomes K (0: none): the walkers' blobs and, where a chain is configured, the blob plane.  The cb
// block is dropped (its width changes); nothing may be stored yet when K > 0 (the plane would miss those rows)
int set_blobs(emx_batch* b, int32_t K) {
    BNEED(b, K >= 0 && K <= BATCH_MAX_BLOBS, "a batch target carries 1 ... %d blobs a sample; got %d", BATCH_MAX_BLOBS, K);
    BNEED(b, K == 0 || b->stored == 0, "a target with blobs is set before the first stored step");
    if (K == b->nblobs && (K == 0 || b->blobs)) return 0;
    BHIP(b, hipStreamSynchronize(b->stream));
    for (double** p : {&b->blobs, &b->chain_blobs, &b->cb_bq})
        if (*p) {
            hipFree(*p);
            *p = nullptr;
        }
    b->nblobs = 0;
    if (K > 0) {
        const size_t BNK = (size_t)b->B * b->N * K;
        BHIP(b, hipMalloc((void**)&b->blobs, BNK * 8));
        BHIP(b, hipMemsetAsync(b->blobs, 0, BNK * 8, b->stream));
        if (b->cap > 0) BHIP(b, hipMalloc((void**)&b->chain_blobs, (size_t)b->cap * BNK * 8));
        b->nblobs = K;
    }
    return 0;
}

// the built-in target's parameter arrays go: every other target has none
void drop_builtin_params(emx_batch* b) {
    for (double** p : {&b->tp0, &b->tp1, &b->tscales})
        if (*p) {
            hipFree(*p);
            *p = nullptr;
        }
    b->tp0_stride = b->tp1_stride = 0;
}

// the settle step of every target setter: the handle takes `nblobs` blobs a sample, no kernel still reads the old target's
// parameters, and they go
int settle_target(emx_batch* b, int32_t nblobs) {
    BHIP(b, hipSetDevice(b->device));
    if (int rc = set_blobs(b, nblobs)) return rc;
    BHIP(b, hipStreamSynchronize(b->stream));
    drop_builtin_params(b);
    return 0;
}

// the checks of the four fused setters ahead of the probe, in the order their callers rely on.  `who`: the setter, `kind`:
// EMX_TARGET_FUSED_USER or EMX_TARGET_FUSED_PT, `data`: a setter that takes per-member counts (`ndata_host`)
int fused_bind_checks(emx_batch* b, const char* who, int32_t kind, bool have_fn, int32_t ndim_compiled, bool data, const int64_t* ndata_host,
                      int32_t nblobs = 0) {
    const bool pt = kind == EMX_TARGET_FUSED_PT;
    BNEED(b, have_fn, "%s: no launcher", who);
    BNEED(b, !data || ndata_host != nullptr, "%s: no data counts (%s)", who, pt ? "one value a member of the handle" : "nbatch values");
    BNEED(b, nblobs >= 0 && nblobs <= BATCH_MAX_BLOBS, "emx_set_batch_target_fused_blobs: 0 <= nblobs <= %d; got %d", BATCH_MAX_BLOBS, nblobs);
    BNEED(b, ndim_compiled == b->D, "the fused %s target was compiled for ndim %d; the batch has ndim %d", pt ? "tempered" : "user", ndim_compiled,
          b->D);
    if (pt)
        BNEED(b, b->pt_T == 0, "%s comes before emx_pt_set_tempering", who);
    else
        BNEED(b, b->pt_T == 0, "a tempered batch does not take a fused user target: the tempered commit and the swap pass belong to the "
                               "batched callback path (emx_set_batch_target_callback)");
    for (int32_t m = 0; data && m < b->B; ++m)
        BNEED(b, ndata_host[m] >= 0 && ndata_host[m] < ((int64_t)1 << 31), "%s: 0 <= ndata < 2^31 for every member; member %d has %lld", who, m,
              (long long)ndata_host[m]);
    if (!b->moves.empty()) {
        char buf[256];
        const char* why = shape_refusal(b->N, b->D, kind, (int32_t)b->moves.size(), b->moves.data(), buf, sizeof buf, nblobs);
        BNEED(b, !why, "%s", why);
    }
    return 0;
}

// the per-member data counts of a fused data target, on the device
int upload_counts(emx_batch* b, int64_t** dev, const int64_t* ndata_host) {
    if (!*dev) BHIP(b, hipMalloc((void**)dev, (size_t)b->B * sizeof(int64_t)));
    BHIP(b, hipMemcpy(*dev, ndata_host, (size_t)b->B * sizeof(int64_t), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

int emx_internal_batch_view(emx_batch* b, EmxBatchView* v) {
    if (!b || !v) return -1;
    v->chain = b->chain;
    v->chain_lp = b->chain_lp;
    v->B = b->B;
    v->D = b->D;
    v->N = b->N;
    v->cap = b->cap;
    v->stored = b->stored;
    v->acf_series = b->tune_acf_series;
    v->stream = b->stream;
    v->device = b->device;
    v->acf = &b->acf;
    v->summary_members = b->tune_summary_members;
    v->summary = &b->summary;
    v->chain_blobs = b->chain_blobs;
    v->nblobs = b->nblobs;
    v->hist_members = b->tune_hist_members;
    v->hist_rows = b->tune_hist_rows;
    v->rhat_members = b->tune_rhat_members;
    v->rhat = &b->rhat;
    v->pt_T = b->pt_T;
    v->chain_L = b->chain_L;
    v->chain_beta = b->chain_beta;
    v->pt_evidence = &b->pt_evidence;
    return 0;
}

int emx_internal_batch_fail(emx_batch* b, int code, const char* msg) { return fail(b, code, "%s", msg); }

#pragma GCC visibility push(default)
extern "C" {

const char* emx_batch_last_error(emx_batch* b) { return b ? b->err.c_str() : "no batch"; }

int emx_batch_check(int64_t nwalkers, int32_t ndim, int32_t target, int32_t nmoves, const emx_move_desc* moves, char* msg,
                    int32_t msglen) {
    char buf[256];
    const char* why = (nmoves > 0 && !moves) ? "no moves" : shape_refusal(nwalkers, ndim, target, nmoves, moves, buf, sizeof buf);
    if (!why) return 0;
    if (msg && msglen > 0) snprintf(msg, (size_t)msglen, "%s", why);
    return -1;
}

int emx_check_batch_blobs(int64_t nwalkers, int32_t ndim, int32_t target, int32_t nmoves, const emx_move_desc* moves, int32_t nblobs,
                          char* msg, int32_t msglen) {
    char buf[320];
    // (a fused tempered target's blobs live in k_pt_run's LDS map, whose bound depends on ntemps: emx_pt_fused_check_blobs)
    const char* why = (nmoves > 0 && !moves) ? "no moves"
                      : (target == EMX_TARGET_FUSED_PT && nblobs > 0)
                          ? "the blobs of a fused tempered target are checked with its ntemps (emx_pt_fused_check_blobs), not as a batch member's"
                          : shape_refusal(nwalkers, ndim, target, nmoves, moves, buf, sizeof buf, nblobs);
    if (!why) return 0;
    if (msg && msglen > 0) snprintf(msg, (size_t)msglen, "%s", why);
    return -1;
}

int emx_batch_create(int32_t device, int32_t nbatch, int64_t nwalkers, int32_t ndim, emx_batch** out) {
    if (!out) return -1;
    *out = nullptr;
    if (nbatch < 1 || nwalkers < 2 || nwalkers > 4096 || ndim < 1 || ndim > 256) return -1;
    emx_batch* b = new emx_batch();
    b->device = device;
    b->B = nbatch;
    b->N = nwalkers;
    b->D = ndim;
    const size_t BN = (size_t)nbatch * nwalkers;
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc((void**)&b->X, BN * ndim * 8) == hipSuccess && hipMalloc((void**)&b->lp, BN * 8) == hipSuccess &&
              hipMalloc((void**)&b->acc, BN) == hipSuccess && hipMalloc((void**)&b->acc_count, BN * 4) == hipSuccess &&
              hipMalloc((void**)&b->seeds, (size_t)nbatch * 8) == hipSuccess &&
              hipHostMalloc((void**)&b->status_host, (size_t)nbatch * SMALL_STATUS_WORDS * 4, hipHostMallocMapped) == hipSuccess &&
              hipHostGetDevicePointer((void**)&b->status, b->status_host, 0) == hipSuccess;
    if (ok) {
        std::memset(b->status_host, 0, (size_t)nbatch * SMALL_STATUS_WORDS * 4);
        ok = hipMemset(b->X, 0, BN * ndim * 8) == hipSuccess && hipMemset(b->lp, 0, BN * 8) == hipSuccess &&
             hipMemset(b->acc, 0, BN) == hipSuccess && hipMemset(b->acc_count, 0, BN * 4) == hipSuccess &&
             hipMemset(b->seeds, 0, (size_t)nbatch * 8) == hipSuccess;
        b->seeds_host.assign(nbatch, 0);
    }
    if (!ok) {
        emx_batch_destroy(b);
        return -2;
    }
    *out = b;
    return 0;
}

int emx_batch_destroy(emx_batch* b) {
    if (!b) return 0;
    hipSetDevice(b->device);
    if (b->stream) hipStreamSynchronize(b->stream);
    if (b->acf) emx_internal_batch_acf_release(b->acf);
    if (b->summary) emx_internal_batch_summary_release(b->summary);
    emx_internal_rhat_release(b->rhat);
    emx_internal_pt_evidence_release(b->pt_evidence);
    for (void* p : {(void*)b->X, (void*)b->lp, (void*)b->acc, (void*)b->acc_count, (void*)b->seeds, (void*)b->tp0, (void*)b->tp1,
                    (void*)b->tscales, (void*)b->chain, (void*)b->chain_lp, (void*)b->fac_dev, (void*)b->col_dev, (void*)b->cb_q,
                    (void*)b->cb_lp, (void*)b->cb_fac, (void*)b->cb_logu, (void*)b->cb_wi, (void*)b->cb_nrows, (void*)b->pt_beta,
                    (void*)b->pt_lo, (void*)b->pt_hi, (void*)b->pt_L, (void*)b->pt_P, (void*)b->chain_L, (void*)b->cb_pr, (void*)b->sw_att,
                    (void*)b->sw_acc, (void*)b->chain_beta, (void*)b->blobs, (void*)b->chain_blobs, (void*)b->cb_bq,
                    (void*)b->fused_ndata, (void*)b->ptf_ndata})
        if (p) hipFree(p);
    for (double* p : b->mscale)
        if (p) hipFree(p);
    if (b->status_host) hipHostFree(b->status_host);
    if (b->stream) hipStreamDestroy(b->stream);
    delete b;
    return 0;
}

int emx_batch_set_tuning(emx_batch* b, const char* key, int64_t value) {
    BNEED(b, key != nullptr, "no tuning key");
    if (!std::strcmp(key, "batch_threads")) {
        BNEED(b, value == 0 || (value >= 64 && value <= 1024 && value % 64 == 0), "batch_threads: 0 or a multiple of 64 in [64, 1024]");
        b->tune_threads = value;
    } else if (!std::strcmp(key, "batch_plan_steps")) {
        BNEED(b, value >= 0 && value <= 64, "batch_plan_steps: 0 ... 64");
        b->tune_plan_steps = value;
    } else if (!std::strcmp(key, "batch_acf_series")) {
        BNEED(b, value >= 0, "batch_acf_series: 0 (auto) or a positive number of series");
        b->tune_acf_series = value;
    } else if (!std::strcmp(key, "batch_summary_members")) {
        BNEED(b, value >= 0, "batch_summary_members: 0 (auto) or a positive number of members");
        b->tune_summary_members = value;
    } else if (!std::strcmp(key, "batch_hist_members")) {
        BNEED(b, value >= 0, "batch_hist_members: 0 (auto) or a positive number of members");
        b->tune_hist_members = value;
    } else if (!std::strcmp(key, "batch_hist_rows")) {
        BNEED(b, value >= 0, "batch_hist_rows: 0 (auto) or a positive number of rows");
        b->tune_hist_rows = value;
    } else if (!std::strcmp(key, "batch_rhat_members")) {
        BNEED(b, value >= 0, "batch_rhat_members: 0 (auto) or a positive number of members");
        b->tune_rhat_members = value;
    } else {
        return fail(b, -1, "unknown batch tuning key '%s'", key);
    }
    return 0;
}

int emx_batch_set_target(emx_batch* b, int32_t kind, const double* p0, const double* p1, const double* scales, int32_t per_member) {
    BNEED(b, kind >= EMX_TARGET_ISO_GAUSS && kind <= EMX_TARGET_BOX, "the batch runs the fused device targets only (kind %d)", kind);
    BHIP(b, hipSetDevice(b->device));
    const int D = b->D, Dp = (D + 15) / 16 * 16;
    const int64_t nset = per_member ? b->B : 1;
    std::vector<double> h0, h1;
    int64_t s0 = 0, s1 = 0;
    if (kind == EMX_TARGET_DIAG_GAUSS || kind == EMX_TARGET_DENSE_GAUSS) {
        BNEED(b, p0 && p1, "target needs (mu, ivar|icov)");
        if (kind == EMX_TARGET_DIAG_GAUSS) {
            s0 = s1 = D;
            h0.assign(p0, p0 + nset * D);
            h1.assign(p1, p1 + nset * D);
        } else {
            BNEED(b, Dp <= DENSE_FUSED_MAX_DP, "dense Gaussian target in a batch: ndim <= %d", DENSE_FUSED_MAX_DP);
            s0 = D;
            s1 = (int64_t)dense_img_doubles(Dp) + Dp;
            h0.assign(p0, p0 + nset * D);
            h1.resize((size_t)nset * s1);
            std::vector<double> img;
            for (int64_t m = 0; m < nset; ++m) {
                const int bad = dense_image(D, p0 + m * D, p1 + m * (int64_t)D * D, img);
                BNEED(b, bad < 0, "dense Gaussian target of member %lld: icov must be symmetric positive definite (Cholesky failed at row %d)",
                      (long long)m, bad);
                const std::vector<double> packed = dense_pack(Dp, img);
                std::copy(packed.begin(), packed.end(), h1.begin() + m * s1);
            }
        }
    }
    std::vector<double> sc((size_t)b->B, 1.0);
    if (kind == EMX_TARGET_ROSENBROCK)
        for (int32_t m = 0; m < b->B; ++m) {
            const double v = scales ? scales[per_member ? m : 0] : 0.0;
            sc[m] = v != 0.0 ? v : 20.0;
        }
    if (int rc = settle_target(b, 0)) return rc;       // the built-in targets have no blobs
    if (!h0.empty()) {
        BHIP(b, hipMalloc((void**)&b->tp0, h0.size() * 8));
        BHIP(b, hipMemcpy(b->tp0, h0.data(), h0.size() * 8, hipMemcpyHostToDevice));
        BHIP(b, hipMalloc((void**)&b->tp1, h1.size() * 8));
        BHIP(b, hipMemcpy(b->tp1, h1.data(), h1.size() * 8, hipMemcpyHostToDevice));
    }
    BHIP(b, hipMalloc((void**)&b->tscales, sc.size() * 8));
    BHIP(b, hipMemcpy(b->tscales, sc.data(), sc.size() * 8, hipMemcpyHostToDevice));
    b->tp0_stride = per_member ? s0 : 0;
    b->tp1_stride = per_member ? s1 : 0;
    b->target = kind;
    b->Dp = kind == EMX_TARGET_DENSE_GAUSS ? Dp : D;
    return 0;
}

int emx_set_batch_target_callback_blobs(emx_batch* b, emx_batch_log_prob_blobs_fn fn, void* user, int32_t nblobs) {
    BNEED(b, fn != nullptr, "emx_set_batch_target_callback_blobs: no function");
    BNEED(b, nblobs >= 1 && nblobs <= BATCH_MAX_BLOBS, "emx_set_batch_target_callback_blobs: 1 <= nblobs <= %d; got %d", BATCH_MAX_BLOBS, nblobs);
    BNEED(b, b->pt_T == 0 || b->target == EMX_TARGET_DEVICE_CALLBACK, "a fused tempered handle has the blobs of its launcher "
                                                                      "(emx_pt_set_target_fused_blobs), not a callback's");
    if (int rc = settle_target(b, nblobs)) return rc;
    b->cb_fn = nullptr;
    b->cbb_fn = fn;
    b->cb_user = user;
    b->target = EMX_TARGET_DEVICE_CALLBACK;
    b->Dp = b->D;
    return 0;
}

int emx_set_batch_target_callback(emx_batch* b, emx_batch_log_prob_fn fn, void* user) {
    BNEED(b, fn != nullptr, "emx_set_batch_target_callback: no function");
    BHIP(b, hipSetDevice(b->device));
    if (int rc = set_blobs(b, 0)) return rc;
    b->cbb_fn = nullptr;       // (ahead of the synchronise: settle_target's steps, with this between them)
    BHIP(b, hipStreamSynchronize(b->stream));
    drop_builtin_params(b);
    b->cb_fn = fn;
    b->cb_user = user;
    b->target = EMX_TARGET_DEVICE_CALLBACK;
    b->Dp = b->D;
    return 0;
}

int emx_set_batch_target_fused(emx_batch* b, emx_fused_batch_fn fn, int32_t ndim_compiled, const void* user_dev) {
    return emx_set_batch_target_fused_blobs(b, fn, ndim_compiled, user_dev, 0);
}

int emx_set_batch_target_fused_blobs(emx_batch* b, emx_fused_batch_fn fn, int32_t ndim_compiled, const void* user_dev, int32_t nblobs) {
    if (int rc = fused_bind_checks(b, "emx_set_batch_target_fused", EMX_TARGET_FUSED_USER, fn != nullptr, ndim_compiled, false, nullptr, nblobs)) return rc;
    // the probe: abi, args_bytes, ndim and nblobs against what the launcher was compiled with; nothing is launched
    SmallRunArgs probe_args{};
    probe_args.D = b->D;
    probe_args.nblobs = nblobs;
    auto fl = fused_desc<emx_fused_launch>(b, EMX_FUSED_ABI, sizeof(SmallRunArgs), MOVE_STRETCH, &probe_args);
    fl.nblobs = nblobs;
    if (int rc = fused_refusal(b, fn(&fl), fl.movesel, nblobs)) return rc;
    if (int rc = settle_target(b, nblobs)) return rc;
    b->fused_fn = fn;
    b->fused_data_fn = nullptr;
    b->fused_user = user_dev;
    b->target = EMX_TARGET_FUSED_USER;
    b->Dp = b->D;
    return 0;
}

int emx_set_batch_target_fused_data(emx_batch* b, emx_fused_batch_data_fn fn, int32_t ndim_compiled, const void* user_dev,
                                    const int64_t* ndata_host) {
    if (int rc = fused_bind_checks(b, "emx_set_batch_target_fused_data", EMX_TARGET_FUSED_USER, fn != nullptr, ndim_compiled, true, ndata_host)) return rc;
    // the probe: abi, args_bytes and ndim against what the launcher was compiled with; nothing is launched
    SmallRunArgs probe_args{};
    probe_args.D = b->D;
    auto fl = fused_desc<emx_fused_batch_data_launch>(b, EMX_FUSED_BATCH_DATA_ABI, sizeof(SmallRunArgs), MOVE_STRETCH, &probe_args);
    if (int rc = fused_refusal(b, fn(&fl), fl.movesel, 0, true)) return rc;
    if (int rc = settle_target(b, 0)) return rc;
    if (int rc = upload_counts(b, &b->fused_ndata, ndata_host)) return rc;
    b->fused_data_fn = fn;
    b->fused_fn = nullptr;
    b->fused_user = user_dev;
    b->target = EMX_TARGET_FUSED_USER;
    b->Dp = b->D;
    return 0;
}

// emx_pt_set_target_fused and emx_pt_set_target_fused_data (`ndata_host` non-null: the data ABI, a plain EMX_FUSED_PT_TARGET launcher
// answers 1)
static int pt_set_target_fused(emx_batch* b, const char* who, emx_pt_fused_fn fn, int32_t ndim_compiled, const void* user_dev, bool data,
                               const int64_t* ndata_host, int32_t nblobs = 0) {
    if (int rc = fused_bind_checks(b, who, EMX_TARGET_FUSED_PT, fn != nullptr, ndim_compiled, data, ndata_host, nblobs)) return rc;
    // the probe: abi, args_bytes, ndim and nblobs against what the launcher was compiled with; nothing is launched
    auto fl = fused_desc<emx_pt_fused_launch>(b, data ? EMX_FUSED_PT_DATA_ABI : EMX_FUSED_PT_ABI, sizeof(PtRunArgs), MOVE_STRETCH, nullptr);
    fl.nblobs = nblobs;
    if (int rc = pt_fused_launcher_refusal(b, fn(&fl), fl.movesel, data, nblobs)) return rc;
    if (int rc = settle_target(b, nblobs)) return rc;
    if (data)
        if (int rc = upload_counts(b, &b->ptf_ndata, ndata_host)) return rc;
    b->ptf_fn = fn;
    b->ptf_data = data;
    b->ptf_user = user_dev;
    b->ptf_has_prior = fl.has_prior ? 1 : 0;
    b->target = EMX_TARGET_FUSED_PT;
    b->Dp = b->D;
    return 0;
}

int emx_pt_set_target_fused(emx_batch* b, emx_pt_fused_fn fn, int32_t ndim_compiled, const void* user_dev) {
    return pt_set_target_fused(b, "emx_pt_set_target_fused", fn, ndim_compiled, user_dev, false, nullptr);
}

int emx_pt_set_target_fused_blobs(emx_batch* b, emx_pt_fused_fn fn, int32_t ndim_compiled, const void* user_dev, int32_t nblobs) {
    return pt_set_target_fused(b, "emx_pt_set_target_fused", fn, ndim_compiled, user_dev, false, nullptr, nblobs);
}

int emx_pt_set_target_fused_data(emx_batch* b, emx_pt_fused_fn fn, int32_t ndim_compiled, const void* user_dev, const int64_t* ndata_host) {
    return pt_set_target_fused(b, "emx_pt_set_target_fused_data", fn, ndim_compiled, user_dev, true, ndata_host);
}

int emx_pt_fused_check(int32_t ntemps, int64_t nwalkers, int32_t ndim, int32_t nmoves, const emx_move_desc* moves, char* msg,
                       int32_t msglen) {
    return emx_pt_fused_check_blobs(ntemps, nwalkers, ndim, nmoves, moves, 0, msg, msglen);
}

int emx_pt_fused_check_blobs(int32_t ntemps, int64_t nwalkers, int32_t ndim, int32_t nmoves, const emx_move_desc* moves, int32_t nblobs,
                             char* msg, int32_t msglen) {
    char buf[400];
    const char* why = (nmoves < 1 || !moves) ? "no moves" : pt_fused_refusal(ntemps, nwalkers, ndim, nmoves, moves, buf, sizeof buf, nblobs);
    if (!why) return 0;
    if (msg && msglen > 0) snprintf(msg, (size_t)msglen, "%s", why);
    return -1;
}

int emx_batch_set_moves(emx_batch* b, int32_t nmoves, const emx_move_desc* moves, const double* cdf) {
    BNEED(b, moves && cdf && nmoves >= 1, "need at least one move and its cdf");
    char buf[256];
    const char* why = shape_refusal(b->N, b->D, b->target >= 0 ? b->target : EMX_TARGET_ISO_GAUSS, nmoves, moves, buf, sizeof buf, b->nblobs);
    BNEED(b, !why, "%s", why);
    for (int m = 0; m < nmoves; ++m)
        BNEED(b, !(moves[m].kind == EMX_MOVE_GAUSS && moves[m].reserved == EMX_GAUSS_SEQUENTIAL && nmoves > 1),
              "the batch runs the sequential GaussianMove as the only move");
    BHIP(b, hipStreamSynchronize(b->stream));
    for (double* p : b->mscale)
        if (p) hipFree(p);
    b->moves.assign(moves, moves + nmoves);
    b->cdf.assign(cdf, cdf + nmoves);
    b->mscale.assign(nmoves, nullptr);
    return 0;
}

int emx_batch_set_move_scale(emx_batch* b, int32_t move, const double* scale, int32_t n) {
    BNEED(b, move >= 0 && move < (int32_t)b->moves.size() && b->moves[move].kind == EMX_MOVE_GAUSS, "move %d is not a Gaussian move", move);
    BNEED(b, scale && n == b->D, "the scale vector must have ndim entries");
    BHIP(b, hipStreamSynchronize(b->stream));
    if (!b->mscale[move]) BHIP(b, hipMalloc((void**)&b->mscale[move], (size_t)n * 8));
    BHIP(b, hipMemcpy(b->mscale[move], scale, (size_t)n * 8, hipMemcpyHostToDevice));
    return 0;
}

int emx_batch_get_move(emx_batch* b, int32_t move, emx_move_desc* out) {
    BNEED(b, move >= 0 && move < (int32_t)b->moves.size() && out, "no move %d", move);
    *out = b->moves[move];
    return 0;
}

int emx_batch_set_philox(emx_batch* b, const uint64_t* seeds, uint64_t step) {
    BNEED(b, seeds != nullptr, "no seeds");
    BHIP(b, hipStreamSynchronize(b->stream));
    b->seeds_host.assign(seeds, seeds + b->B);
    BHIP(b, hipMemcpy(b->seeds, seeds, (size_t)b->B * 8, hipMemcpyHostToDevice));
    b->step = step;
    return 0;
}

int emx_batch_get_philox(emx_batch* b, uint64_t* seeds, uint64_t* step) {
    if (seeds) std::copy(b->seeds_host.begin(), b->seeds_host.end(), seeds);
    if (step) *step = b->step;
    return 0;
}

int emx_batch_set_state(emx_batch* b, const double* coords, const double* log_prob) {
    BNEED(b, coords != nullptr, "no coordinates");
    const size_t BN = (size_t)b->B * b->N;
    BHIP(b, hipMemcpyAsync(b->X, coords, BN * b->D * 8, hipMemcpyHostToDevice, b->stream));
    if (log_prob) BHIP(b, hipMemcpyAsync(b->lp, log_prob, BN * 8, hipMemcpyHostToDevice, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    return 0;
}

int emx_batch_get_state(emx_batch* b, double* coords, double* log_prob) {
    const size_t BN = (size_t)b->B * b->N;
    if (coords) BHIP(b, hipMemcpyAsync(coords, b->X, BN * b->D * 8, hipMemcpyDeviceToHost, b->stream));
    if (log_prob) BHIP(b, hipMemcpyAsync(log_prob, b->lp, BN * 8, hipMemcpyDeviceToHost, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    return 0;
}

int emx_get_blobs_batch(emx_batch* b, double* out, int32_t* nblobs_out) {
    if (nblobs_out) *nblobs_out = b->nblobs;
    BNEED(b, b->nblobs > 0 && b->blobs, "the handle's target has no blobs");
    if (out) {
        BHIP(b, hipMemcpyAsync(out, b->blobs, (size_t)b->B * b->N * b->nblobs * 8, hipMemcpyDeviceToHost, b->stream));
        BHIP(b, hipStreamSynchronize(b->stream));
    }
    return 0;
}

int emx_batch_eval_state_log_prob(emx_batch* b) {
    BNEED(b, b->target >= 0, "no target set");
    BNEED(b, !b->moves.empty(), "no moves set");
    BHIP(b, hipSetDevice(b->device));
    if (b->target == EMX_TARGET_DEVICE_CALLBACK) return eval_callback(b);
    if (b->target == EMX_TARGET_FUSED_PT) return launch_pt(b, 0, 0, 1, 0, true);
    return launch(b, 0, 0, 1, 0, true);
}

int emx_batch_chain_config(emx_batch* b, int64_t capacity) {
    BNEED(b, capacity >= 0, "negative capacity");
    if (capacity <= b->cap) return 0;
    BHIP(b, hipSetDevice(b->device));
    const size_t ND = (size_t)b->N * b->D, N = (size_t)b->N, NK = (size_t)b->N * b->nblobs;
    double* nB = nullptr;                 // the blob plane, only for a target with blobs
    if (NK > 0) BHIP(b, hipMalloc((void**)&nB, (size_t)b->B * capacity * NK * 8));
    double *nc = nullptr, *nl = nullptr;
    if (hipMalloc((void**)&nc, (size_t)b->B * capacity * ND * 8) != hipSuccess) {
        if (nB) hipFree(nB);
        return fail(b, -2, "chain allocation failed");
    }
    if (hipMalloc((void**)&nl, (size_t)b->B * capacity * N * 8) != hipSuccess) {
        hipFree(nc);
        if (nB) hipFree(nB);
        return fail(b, -2, "chain allocation failed");
    }
    double *nL = nullptr, *nb = nullptr;
    if (b->pt_T > 0 && (hipMalloc((void**)&nL, (size_t)b->B * capacity * N * 8) != hipSuccess ||
                        hipMalloc((void**)&nb, (size_t)b->B * capacity * 8) != hipSuccess)) {
        hipFree(nc);
        hipFree(nl);
        if (nL) hipFree(nL);
        if (nB) hipFree(nB);
        return fail(b, -2, "chain allocation failed");
    }
    if (b->stored > 0) {      // what is stored stays: member by member, into the longer rows
        BHIP(b, hipMemcpy2DAsync(nc, capacity * ND * 8, b->chain, b->cap * ND * 8, b->stored * ND * 8, b->B, hipMemcpyDeviceToDevice, b->stream));
        BHIP(b, hipMemcpy2DAsync(nl, capacity * N * 8, b->chain_lp, b->cap * N * 8, b->stored * N * 8, b->B, hipMemcpyDeviceToDevice, b->stream));
        if (nL) BHIP(b, hipMemcpy2DAsync(nL, capacity * N * 8, b->chain_L, b->cap * N * 8, b->stored * N * 8, b->B, hipMemcpyDeviceToDevice, b->stream));
        if (nb) BHIP(b, hipMemcpy2DAsync(nb, capacity * 8, b->chain_beta, b->cap * 8, b->stored * 8, b->B, hipMemcpyDeviceToDevice, b->stream));
        if (nB && b->chain_blobs)
            BHIP(b, hipMemcpy2DAsync(nB, capacity * NK * 8, b->chain_blobs, b->cap * NK * 8, b->stored * NK * 8, b->B, hipMemcpyDeviceToDevice, b->stream));
    }
    BHIP(b, hipStreamSynchronize(b->stream));
    if (b->chain_blobs) hipFree(b->chain_blobs);
    b->chain_blobs = nB;
    if (b->chain_L) hipFree(b->chain_L);
    b->chain_L = nL;
    if (b->chain_beta) hipFree(b->chain_beta);
    b->chain_beta = nb;
    if (b->chain) hipFree(b->chain);
    if (b->chain_lp) hipFree(b->chain_lp);
    b->chain = nc;
    b->chain_lp = nl;
    b->cap = capacity;
    return 0;
}

int emx_batch_run(emx_batch* b, int64_t nsteps, int32_t thin_by, int32_t store) {
    BNEED(b, thin_by >= 1, "Invalid thinning argument");
    BNEED(b, nsteps >= 0, "negative nsteps");
    BNEED(b, b->target >= 0, "no target set");
    BNEED(b, !b->moves.empty(), "no moves set");
    if (store) BNEED(b, b->stored + nsteps <= b->cap, "chain capacity exhausted (call emx_batch_chain_config)");
    BHIP(b, hipSetDevice(b->device));
    if (b->target == EMX_TARGET_DEVICE_CALLBACK) return run_callback(b, nsteps * thin_by, thin_by, store);
    bool any_gauss = false;
    for (const auto& mv : b->moves) any_gauss = any_gauss || mv.kind == EMX_MOVE_GAUSS;
    // up to 4 096 steps a launch (as a single ensemble's); with Gaussian moves the per-member factors stay <= 32 MB a launch
    const int64_t total = nsteps * thin_by;
    const int64_t most = any_gauss ? std::max<int64_t>(1, std::min<int64_t>(4096, (4 << 20) / b->B)) : 4096;
    const bool ptf = b->target == EMX_TARGET_FUSED_PT;
    for (int64_t i = 0; i < total;) {
        const int64_t chunk = std::min<int64_t>(total - i, most);
        const int rc = ptf ? launch_pt(b, i, chunk, thin_by, store, false) : launch(b, i, chunk, thin_by, store, false);
        if (rc) return rc;
        i += chunk;
    }
    return 0;
}

int emx_batch_iteration(emx_batch* b, int64_t* stored, int64_t* proposals) {
    if (stored) *stored = b->stored;
    if (proposals) *proposals = b->proposals;
    return 0;
}

int emx_batch_chain_read(emx_batch* b, int32_t what, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop,
                         int64_t stride, double* out) {
    BNEED(b, what == 0 || what == 1 || ((what == 2 || what == 3) && b->chain_L) || (what == 4 && b->chain_blobs),
          "what: 0 coordinates, 1 log-probs, 2 log-likelihoods, 3 betas (the last two tempered), 4 blobs (a target with blobs)");
    BNEED(b, 0 <= member_lo && member_lo <= member_hi && member_hi <= b->B, "members [%d, %d) outside [0, %d)", member_lo, member_hi, b->B);
    BNEED(b, stride >= 1 && 0 <= start && start <= stop && stop <= b->stored, "rows [%lld, %lld) outside the %lld stored",
          (long long)start, (long long)stop, (long long)b->stored);
    BNEED(b, out != nullptr, "no output buffer");
    const int64_t nsel = (stop - start + stride - 1) / stride;
    if (nsel == 0 || member_hi == member_lo) return 0;
    BHIP(b, hipSetDevice(b->device));
    const size_t row = what == 3 ? 1 : (size_t)b->N * (what == 0 ? b->D : what == 4 ? b->nblobs : 1);
    const double* base = what == 0 ? b->chain : what == 1 ? b->chain_lp : what == 2 ? b->chain_L : what == 3 ? b->chain_beta : b->chain_blobs;
    for (int32_t m = member_lo; m < member_hi; ++m)
        BHIP(b, hipMemcpy2DAsync(out + (size_t)(m - member_lo) * nsel * row, row * 8, base + ((size_t)m * b->cap + start) * row, stride * row * 8,
                                 row * 8, nsel, hipMemcpyDeviceToHost, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    return 0;
}

int emx_batch_accepted_counts(emx_batch* b, double* out) {
    const size_t BN = (size_t)b->B * b->N;
    std::vector<uint32_t> h(BN);
    BHIP(b, hipMemcpyAsync(h.data(), b->acc_count, BN * 4, hipMemcpyDeviceToHost, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    for (size_t k = 0; k < BN; ++k) out[k] = (double)h[k];
    return 0;
}

int emx_batch_status(emx_batch* b, uint32_t* bits) {
    BHIP(b, hipStreamSynchronize(b->stream));      // every launch that could still raise a bit has finished
    for (int32_t m = 0; m < b->B; ++m) {
        uint32_t v = 0;
        for (int k = 0; k < SMALL_STATUS_WORDS; ++k)
            if (__atomic_exchange_n(&b->status_host[(size_t)m * SMALL_STATUS_WORDS + k], 0u, __ATOMIC_ACQ_REL)) v |= 1u << k;
        if (bits) bits[m] = v;
    }
    return 0;
}

int emx_batch_launch_info(emx_batch* b, int32_t* threads, int32_t* plan_steps, int64_t* launches) {
    if (threads) *threads = b->last_threads;
    if (plan_steps) *plan_steps = b->last_plan_steps;
    if (launches) *launches = b->launches;
    return 0;
}

// ---- parallel tempering (emx_pt.hip) ----

int emx_pt_set_tempering(emx_batch* b, int32_t ntemps, const double* betas, const double* box_lo, const double* box_hi) {
    BNEED(b, b->target != EMX_TARGET_FUSED_USER, "tempering does not run a fused user target (emx_set_batch_target_fused): the tempered "
                                                 "commit and the swap pass belong to the batched callback path (emx_set_batch_target_callback)");
    BNEED(b, b->target == EMX_TARGET_DEVICE_CALLBACK || b->target == EMX_TARGET_FUSED_PT,
          "tempering needs a batched callback target (emx_set_batch_target_callback)");
    // (a callback handle takes its blobs once it is tempered; a fused tempered target brings them with its launcher)
    BNEED(b, b->nblobs == 0 || b->target == EMX_TARGET_FUSED_PT,
          "tempering does not take over a batch's target with blobs: emx_set_batch_target_callback_blobs comes after emx_pt_set_tempering");
    if (b->target == EMX_TARGET_FUSED_PT) {
        BNEED(b, !(b->ptf_has_prior && box_lo), "the fused tempered target's launcher carries a prior functor: a box prior on top is refused");
        if (!b->moves.empty()) {
            char buf[400];
            const char* why = pt_fused_refusal(ntemps, b->N, b->D, (int32_t)b->moves.size(), b->moves.data(), buf, sizeof buf, b->nblobs);
            BNEED(b, !why, "%s", why);
        }
    }
    BNEED(b, ntemps >= 1 && b->B % ntemps == 0, "ntemps = %d does not divide the batch of %d members", ntemps, b->B);
    BNEED(b, !b->pt_adapt || ntemps <= PT_ADAPT_MAX_T, "an adaptive ladder has at most %d rungs; ntemps = %d", PT_ADAPT_MAX_T, ntemps);
    BNEED(b, betas != nullptr, "no betas");
    BNEED(b, betas[0] == 1.0, "betas[0] must be 1");
    for (int t = 0; t < ntemps; ++t) {
        BNEED(b, betas[t] >= 0.0 && betas[t] <= 1.0, "betas must lie in [0, 1]; betas[%d] = %g", t, betas[t]);
        if (t > 0) BNEED(b, betas[t] <= betas[t - 1], "betas must not increase (betas[%d] = %g, betas[%d] = %g)", t - 1,
                         betas[t - 1], t, betas[t]);
    }
    BNEED(b, (box_lo == nullptr) == (box_hi == nullptr), "a box prior needs both bounds");
    BNEED(b, b->stored == 0, "tempering is set before anything is stored");
    BHIP(b, hipSetDevice(b->device));
    BHIP(b, hipStreamSynchronize(b->stream));
    for (double** p : {&b->pt_beta, &b->pt_lo, &b->pt_hi, &b->pt_L, &b->pt_P, &b->chain_L, &b->chain_beta})
        if (*p) {
            hipFree(*p);
            *p = nullptr;
        }
    for (unsigned long long** p : {&b->sw_att, &b->sw_acc})
        if (*p) {
            hipFree(*p);
            *p = nullptr;
        }
    const size_t BN = (size_t)b->B * b->N;
    std::vector<double> mb((size_t)b->B);
    for (int32_t m = 0; m < b->B; ++m) mb[m] = betas[m % ntemps];
    BHIP(b, hipMalloc((void**)&b->pt_beta, mb.size() * 8));
    BHIP(b, hipMemcpy(b->pt_beta, mb.data(), mb.size() * 8, hipMemcpyHostToDevice));
    if (box_lo) {
        for (int d = 0; d < b->D; ++d) BNEED(b, box_lo[d] <= box_hi[d], "box prior: lo[%d] > hi[%d]", d, d);
        BHIP(b, hipMalloc((void**)&b->pt_lo, (size_t)b->D * 8));
        BHIP(b, hipMalloc((void**)&b->pt_hi, (size_t)b->D * 8));
        BHIP(b, hipMemcpy(b->pt_lo, box_lo, (size_t)b->D * 8, hipMemcpyHostToDevice));
        BHIP(b, hipMemcpy(b->pt_hi, box_hi, (size_t)b->D * 8, hipMemcpyHostToDevice));
    }
    BHIP(b, hipMalloc((void**)&b->pt_L, BN * 8));
    BHIP(b, hipMalloc((void**)&b->pt_P, BN * 8));
    BHIP(b, hipMemset(b->pt_L, 0, BN * 8));
    BHIP(b, hipMemset(b->pt_P, 0, BN * 8));
    const size_t npairs = (size_t)(b->B / ntemps) * (ntemps > 1 ? ntemps - 1 : 1);
    BHIP(b, hipMalloc((void**)&b->sw_att, npairs * 8));
    BHIP(b, hipMalloc((void**)&b->sw_acc, npairs * 8));
    BHIP(b, hipMemset(b->sw_att, 0, npairs * 8));
    BHIP(b, hipMemset(b->sw_acc, 0, npairs * 8));
    if (b->cap > 0) BHIP(b, hipMalloc((void**)&b->chain_L, (size_t)b->B * b->cap * b->N * 8));
    if (b->cap > 0) BHIP(b, hipMalloc((void**)&b->chain_beta, (size_t)b->B * b->cap * 8));
    b->pt_betas.assign(betas, betas + ntemps);
    b->pt_T = ntemps;
    b->pt_updates = 0;
    return 0;
}

int emx_set_batch_prior_callback(emx_batch* b, emx_batch_log_prob_fn fn, void* user) {
    BNEED(b, b->pt_T > 0, "a prior callback needs tempering (emx_pt_set_tempering)");
    BNEED(b, b->pt_lo == nullptr || fn == nullptr, "the batch has a box prior already");
    BNEED(b, b->target != EMX_TARGET_FUSED_PT || fn == nullptr, "a fused tempered target takes its prior as a functor of its launcher (or a box), "
                                                                "not as a callback");
    BHIP(b, hipStreamSynchronize(b->stream));
    b->pr_fn = fn;
    b->pr_user = user;
    return 0;
}

int emx_pt_set_swap_every(emx_batch* b, int64_t n) {
    BNEED(b, n >= 0, "swap_every must be >= 0 (0: never)");
    b->swap_every = n;
    return 0;
}

int emx_pt_swap(emx_batch* b) {
    BNEED(b, b->pt_T > 0, "no tempering set (emx_pt_set_tempering)");
    BNEED(b, b->step > 0, "no step taken: the swap pass uses the draws of the last step");
    BHIP(b, hipSetDevice(b->device));
    if (b->pt_T < 2) {
        if (b->pt_adapt) ++b->pt_updates;      // no pair, nothing moves; the update still counts
        return 0;
    }
    return swap_pass(b, b->step - 1, -1, true);
}

int emx_pt_swap_counts(emx_batch* b, uint64_t* attempts, uint64_t* accepts) {
    BNEED(b, b->pt_T > 0, "no tempering set (emx_pt_set_tempering)");
    const size_t n = (size_t)(b->B / b->pt_T) * (b->pt_T - 1);
    if (n == 0) return 0;
    if (attempts) BHIP(b, hipMemcpyAsync(attempts, b->sw_att, n * 8, hipMemcpyDeviceToHost, b->stream));
    if (accepts) BHIP(b, hipMemcpyAsync(accepts, b->sw_acc, n * 8, hipMemcpyDeviceToHost, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    return 0;
}

int emx_pt_mean_loglike(emx_batch* b, int64_t start, int64_t stop, int64_t stride, double* out) {
    BNEED(b, b->pt_T > 0 && b->chain_L, "no tempered chain");
    BNEED(b, stride >= 1 && 0 <= start && start < stop && stop <= b->stored, "rows [%lld, %lld) outside the %lld stored",
          (long long)start, (long long)stop, (long long)b->stored);
    BNEED(b, out != nullptr, "no output buffer");
    BHIP(b, hipSetDevice(b->device));
    double* dev = nullptr;
    BHIP(b, hipMalloc((void**)&dev, (size_t)b->B * 8));
    hipError_t e = pt_mean_launch(b->chain_L, b->cap, b->B, (int32_t)b->N, start, stop, stride, dev, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dev, (size_t)b->B * 8, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    hipStreamSynchronize(b->stream);
    hipFree(dev);
    BHIP(b, e);
    ++b->launches;
    return 0;
}

int emx_pt_set_state(emx_batch* b, const double* coords, const double* loglike, const double* logprior) {
    BNEED(b, b->pt_T > 0, "no tempering set (emx_pt_set_tempering)");
    BNEED(b, coords && loglike && logprior, "coords, loglike and logprior are all needed");
    const size_t BN = (size_t)b->B * b->N;
    std::vector<double> mb((size_t)b->B), lp(BN);       // each member's current beta (the ladder may have adapted)
    BHIP(b, hipMemcpyAsync(mb.data(), b->pt_beta, mb.size() * 8, hipMemcpyDeviceToHost, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    for (size_t r = 0; r < BN; ++r) lp[r] = pt_tempered(mb[r / b->N], loglike[r], logprior[r]);
    BHIP(b, hipMemcpyAsync(b->X, coords, BN * b->D * 8, hipMemcpyHostToDevice, b->stream));
    BHIP(b, hipMemcpyAsync(b->pt_L, loglike, BN * 8, hipMemcpyHostToDevice, b->stream));
    BHIP(b, hipMemcpyAsync(b->pt_P, logprior, BN * 8, hipMemcpyHostToDevice, b->stream));
    BHIP(b, hipMemcpyAsync(b->lp, lp.data(), BN * 8, hipMemcpyHostToDevice, b->stream));
    // the state bypassed the likelihood: the blobs of a handle that has them are NaN (every byte 0xff is a quiet NaN)
    if (b->nblobs > 0 && b->blobs) BHIP(b, hipMemsetAsync(b->blobs, 0xff, BN * b->nblobs * 8, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    return 0;
}

int emx_pt_set_adaptation(emx_batch* b, int32_t on, double lag, double time) {
    BNEED(b, b->pt_T > 0, "no tempering set (emx_pt_set_tempering)");
    BNEED(b, lag > 0.0 && lag < __builtin_inf(), "adaptation_lag must be finite and > 0; got %g", lag);
    BNEED(b, time > 0.0 && time < __builtin_inf(), "adaptation_time must be finite and > 0; got %g", time);
    if (on) {
        BNEED(b, b->pt_T <= PT_ADAPT_MAX_T, "an adaptive ladder has at most %d rungs; ntemps = %d", PT_ADAPT_MAX_T, b->pt_T);
        if (!b->pt_adapt) {       // the current ladders must suit the update
            std::vector<double> mb((size_t)b->B);
            BHIP(b, hipMemcpyAsync(mb.data(), b->pt_beta, mb.size() * 8, hipMemcpyDeviceToHost, b->stream));
            BHIP(b, hipStreamSynchronize(b->stream));
            for (int64_t g = 0; g < b->B / b->pt_T; ++g)
                if (int rc = check_ladder_row(b, mb.data() + g * b->pt_T, b->pt_T, g, true)) return rc;
        }
    }
    b->pt_adapt = on ? 1 : 0;
    b->pt_lag = lag;
    b->pt_time = time;
    return 0;
}

int emx_pt_get_ladder(emx_batch* b, double* betas, int64_t* updates) {
    BNEED(b, b->pt_T > 0, "no tempering set (emx_pt_set_tempering)");
    if (betas) {
        BHIP(b, hipMemcpyAsync(betas, b->pt_beta, (size_t)b->B * 8, hipMemcpyDeviceToHost, b->stream));
        BHIP(b, hipStreamSynchronize(b->stream));
    }
    if (updates) *updates = b->pt_updates;
    return 0;
}

int emx_pt_set_ladder(emx_batch* b, const double* betas, const int64_t* updates) {
    BNEED(b, b->pt_T > 0, "no tempering set (emx_pt_set_tempering)");
    BNEED(b, betas != nullptr, "no betas");
    BNEED(b, !updates || *updates >= 0, "updates must be >= 0");
    for (int64_t g = 0; g < b->B / b->pt_T; ++g)
        if (int rc = check_ladder_row(b, betas + g * b->pt_T, b->pt_T, g, b->pt_adapt != 0)) return rc;
    BHIP(b, hipSetDevice(b->device));
    BHIP(b, hipMemcpyAsync(b->pt_beta, betas, (size_t)b->B * 8, hipMemcpyHostToDevice, b->stream));
    BHIP(b, pt_relp_launch(b->lp, b->pt_L, b->pt_P, b->pt_beta, b->B, (int32_t)b->N, b->stream));
    ++b->launches;
    BHIP(b, hipStreamSynchronize(b->stream));
    if (updates) b->pt_updates = *updates;
    return 0;
}

int emx_pt_get_state(emx_batch* b, double* loglike, double* logprior) {
    BNEED(b, b->pt_T > 0, "no tempering set (emx_pt_set_tempering)");
    const size_t BN = (size_t)b->B * b->N;
    if (loglike) BHIP(b, hipMemcpyAsync(loglike, b->pt_L, BN * 8, hipMemcpyDeviceToHost, b->stream));
    if (logprior) BHIP(b, hipMemcpyAsync(logprior, b->pt_P, BN * 8, hipMemcpyDeviceToHost, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    return 0;
}

int emx_pt_get_blobs(emx_batch* b, double* out) {
    BNEED(b, b->pt_T > 0, "no tempering set (emx_pt_set_tempering)");
    BNEED(b, b->nblobs > 0 && b->blobs, "the handle's likelihood has no blobs");
    BNEED(b, out != nullptr, "no output buffer");
    BHIP(b, hipMemcpyAsync(out, b->blobs, (size_t)b->B * b->N * b->nblobs * 8, hipMemcpyDeviceToHost, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
