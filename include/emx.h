/* libemx -- C ABI of the MI355X split-ensemble sampler hot path.
 *
 * The reference (dfm/emcee) has no FFI: its boundary for this path is the duck-typed Python
 * protocol  EnsembleSampler.sample -> Move.propose(model, state) -> model.compute_log_prob_fn
 * (SURVEY.md 8b).  Each entry point below names the reference code it replaces (paths relative
 * to /root/reference/src/emcee).  The Python host layer (emcee_amd/) binds these through ctypes;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions: every function returns 0 on success and a negative code on error, with a
 * message available from emx_last_error(); no C++ exception crosses the boundary; the caller
 * owns all host buffers, the library owns all device buffers; a context is bound to one
 * device and is not thread-safe; all device work is asynchronous on the context's stream
 * except calls that copy results to host memory.  Arrays are C-contiguous float64 unless
 * noted.  There is NO CPU fallback: without a usable HIP device emx_create fails.
 */
#ifndef EMX_H
#define EMX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emx_ctx emx_ctx;

enum emx_target_kind {
    EMX_TARGET_HOST = 0,       /* log-prob evaluated by the caller (split-phase API)            */
    EMX_TARGET_ISO_GAUSS = 1,  /* -0.5 sum x^2            tests/integration/test_proposal.py:21 */
    EMX_TARGET_DIAG_GAUSS = 2, /* -0.5 sum ivar (x-mu)^2  docs/index.rst:41-45                 */
    EMX_TARGET_DENSE_GAUSS = 3,/* -0.5 (x-mu)^T icov (x-mu)  docs/tutorials/quickstart.ipynb:76 */
    EMX_TARGET_ROSENBROCK = 4, /* -sum[100 (x_{i+1}-x_i^2)^2 + (1-x_i)^2] / scale (BASELINE C3) */
    EMX_TARGET_BOX = 5,        /* 0 inside [0,1]^D else -inf   test_proposal.py:25-28           */
    EMX_TARGET_DEVICE_CALLBACK = 6,/* the caller's batched log-prob on device buffers (emx_set_target_callback) */
    EMX_TARGET_FUSED_USER = 8,     /* batches only: the caller's per-row device function compiled into the one-workgroup kernel
                                      (emx_set_batch_target_fused; 7 is taken inside the kernels) */
    EMX_TARGET_FUSED_PT = 9,       /* tempered batches only: the caller's likelihood (and prior) compiled into the tempered
                                      one-workgroup kernel k_pt_run (emx_pt_set_target_fused) */
    EMX_TARGET_FUSED_ENSEMBLE = 10 /* a single ensemble: the caller's per-row device function compiled into the half-step kernel
                                      k_halfstep_user (emx_set_target_fused) */
};

enum emx_move_kind {
    EMX_MOVE_STRETCH = 0, EMX_MOVE_DE = 1, EMX_MOVE_SNOOKER = 2,
    /* moves/gaussian.py + moves/mh.py: Metropolis step with an isotropic / axis-aligned Gaussian proposal,
     * every walker at once from its own position (nsplits must be 1).  Fields: reserved = mode
     * (emx_gauss_mode), sigma = isotropic standard deviation (emx_set_move_scale installs a per-coordinate
     * vector instead), a != 0 enables the step-size factor exp(U(-g0, g0)) with g0 = ln(factor)
     * (gaussian.py:81-84), gammas = the sequential mode's coordinate cursor (gaussian.py:96-97; the library
     * advances it, emx_get_move reads it back). */
    EMX_MOVE_GAUSS = 3,
    /* (4 is not a public kind: the kernels' proposal-evaluation pass carries it) */
    /* moves/walk.py: WalkMove, rng mode EMX_RNG_PHILOX only, ndim <= 128.  Fields: reserved = s, the helper walkers per update
     * (0: the whole complement; otherwise 2 <= s <= 1024 and s <= the complement of every split). */
    EMX_MOVE_WALK = 5,
    /* moves/kde.py: KDEMove, rng mode EMX_RNG_PHILOX only, ndim <= 128.  Fields: reserved = the bandwidth rule (0 Scott,
     * 1 Silverman, 2 scalar), a = the scalar factor of rule 2.  A complement covariance that is not positive definite sets
     * status bit 5 (scipy.stats.gaussian_kde's LinAlgError). */
    EMX_MOVE_KDE = 6
};
enum emx_gauss_mode { EMX_GAUSS_VECTOR = 0, EMX_GAUSS_RANDOM = 1, EMX_GAUSS_SEQUENTIAL = 2 };

enum emx_rng_mode {
    EMX_RNG_INPUTS = 0,  /* every step's plan is supplied with emx_plan_set                     */
    EMX_RNG_MT19937 = 1, /* NumPy legacy RandomState stream: same seed => same chain as emcee   */
    EMX_RNG_PHILOX = 2   /* counter-based, generated inside the kernels (throughput mode)       */
};

/* moves/red_blue.py:37-42, moves/stretch.py:22, moves/de.py:28-31,33-38, moves/de_snooker.py:26-29 */
typedef struct emx_move_desc {
    int32_t kind;            /* emx_move_kind                                   */
    int32_t nsplits;         /* RedBlueMove.nsplits (snooker: 4)                */
    int32_t randomize_split; /* RedBlueMove.randomize_split                     */
    int32_t reserved;
    double a;                /* StretchMove.a                                   */
    double sigma;            /* DEMove.sigma                                    */
    double g0;               /* DEMove.g0 = gamma0 or 2.38/sqrt(2 ndim)         */
    double gammas;           /* DESnookerMove.gammas                            */
} emx_move_desc;

/* ---- library / context ---------------------------------------------------------------- */
const char* emx_version(void);
const char* emx_last_error(const emx_ctx* ctx); /* ctx may be NULL: last creation error */
int emx_device_count(int32_t* n);
/* EnsembleSampler.__init__ (ensemble.py:79-137): one context per (device, ensemble). */
int emx_create(int32_t device, int64_t nwalkers, int32_t ndim, emx_ctx** out);
int emx_destroy(emx_ctx* ctx);
/* adopt an external hipStream_t (e.g. torch's current stream); NULL restores the own stream */
int emx_set_stream(emx_ctx* ctx, void* hip_stream);
int emx_sync(emx_ctx* ctx);
/* sticky device status: bit0 NaN log-prob (ensemble.py:550-551), bit1 non-finite coordinate
 * (ensemble.py:476-479), bit2 pull-exchange record capacity exceeded (a >8 sigma event: the run is
 * invalid, never silently wrong), bit3 direct / replay exchange: a peer did not reach the device-side barrier in time
 * (raised again by every later barrier of that attachment), bit4 the device producer of exact-mode plans (rng mode MT19937,
 * large ensembles) stalled -- a stage waited 20 s for another -- or its stream ran out under the tokenizer: the steps taken from
 * it are void; the call that retires the producer (emx_run's next start, emx_rng_get_mt19937, emx_set_moves ...) returns the
 * error as well and leaves the generator where it stood before the producer started; bit5 EMX_MOVE_KDE: the complement's
 * covariance is not positive definite (the proposals of that half-step are rejected).  Reading clears it. */
int emx_status(emx_ctx* ctx, uint32_t* bits);
/* Tuning keys (A/B measurements, parity tests; defaults are what the product runs).  An unknown key is an error.  The environment
 * variable EMX_TUNE="key=value,key=value" applies keys to every context at creation.  One table -- nothing measured-and-rejected is
 * left behind a key (round 6: the p2p form, the fused wide propose and the split upload were removed from the library):
 *
 *   key                        default   meaning
 *   -- launch shape of the per-half-step kernels --
 *   "spw"                      0 (auto)  slots per wave                      "blocks_per_cu"     2         workgroups a CU is given
 *   "waves_per_block"          0 (auto)  1 / 2 / 4 / 8                       "throttle"          0         half-steps in flight (0: unbounded)
 *   "graph"                    0         1: a 16-step block of Philox launches replayed as a hipGraph
 *   "prep_hint"                1         steps a caller of emx_step_begin will take (Philox plan batch size)
 *   "full_plan"                0         1: Philox plans carry every column (default: the ones the step's fused kernel reads)
 *   "small_kernel"             1         ensembles that fit one workgroup's LDS run whole emx_run calls in one workgroup (2: a fused
 *                                        user target's too wherever they fit, not only where that is faster: emx_small_fused_pays)
 *   "gauss_materialize"        0         Gaussian move: 1: proposals through memory (parity tests of the register form)
 *   -- dense targets --
 *   "dense_wide"               0         1: the propose / log-prob / commit path whatever the ndim; 2: ... with the single-role log-prob kernel
 *   "slab"                     1         0: never the slab form (emx_slab.hip); 1: from padded ndim 112; 2: from padded ndim 80
 *   "slab_skew"                1         0 ... 4: when the second wave of a SIMD starts its first tile's row loads
 *   -- persistent kernels (emx_persist_info) --
 *   "persist"                  1         0: never a persistent launch
 *   "persist_local"            1         0: never the one-XCD form        "persist_local_max_walkers"  8192
 *   "persist_valu"             1         0: element-wise targets on the per-half-step launches
 *   "persist_slab"             1         0: dense targets of padded ndim 80 ... 128 on the per-half-step launches (1: k_persist_slab, emx_pslab.hip)
 *   "persist_slab_skew"        1         k_persist_slab: 0 ... 4, as "slab_skew"   "persist_slab_local_max_walkers"  4096   its one-XCD form's largest ensemble
 *   "persist_odd"              1         0: dense targets of odd ndim on the per-half-step launches (1: k_persist with one coordinate per lane, emx_podd.hip)
 *   "persist_mix"              1         0: DE and snooker steps of a mixture in launches of their own
 *   "persist_span"             1         0: a launch ends with its Philox plan batch
 *   "persist_min_walkers"      512       smallest ensemble             "persist_timeout_ms"   2000      bound of a barrier wait
 *   "persist_rows_late"        1         launches that store chain rows (stretch move, even ndim <= 64) ask for the next half-step's own rows behind the
 *                                        MFMA phase instead of in front of it (k_persist<..., ROWS_LATE>): 1 the one-XCD form and device-wide launches
 *                                        with eight tiles a CU and half-step (65 536 walkers), 2 always, 0 never
 *   "persist_carry"            1         device-wide stretch launches that store no rows, over Philox plans arranged after the step before, keep own rows
 *                                        over the step boundary in registers (k_persist<..., CARRY>, emx_persist_carry_launches); 0: never.  0 or 1, else an error
 *   "persist_partner_prefetch" 1         the CARRY form asks for the partner rows of a step's first half-step that nobody writes during the half-step
 *                                        before (the partner was in split 0 of the step before: emx_plan_partner_stable) under that half-step's MFMA
 *                                        phase, not behind the barrier (emx_persist_pprefetch_launches); 0: every partner row behind the barrier.  0 or 1, else an error
 *   "persist_stagger"          -1        how * 256 + n: some waves of a k_persist / k_persist_mix workgroup ask for their partner rows n x 64 clocks
 *                                        after the others (how 0: waves 4-7, 1: odd waves, 2: the waves of SIMDs 2 and 3, 4: SIMD k waits k n); -1: 516
 *                                        for device-wide stretch launches without stored rows, 528 for the DE move and DE + snooker mixtures (k_persist_mix), else 0
 *                                        (profiles/r06/stagger_ab.md)
 *   "persist_max_halfsteps"    40        half-steps a launch may hold (<= 40: twenty stretch / DE steps; a launch never reads plans of more than two batches)
 *   "persist_gauss_wpb"        0 (auto)  waves per workgroup of k_persist_gauss
 *   "persist_exact"            1         0: exact mode (EMX_RNG_MT19937) on the per-half-step launches with an upload per step
 *   "persist_exact_mix"        1         0: ... for one move only      "persist_exact_steps"  16        steps per launch (<= 16)
 *   "persist_exact_max_walkers" 32768    largest ensemble of the device-wide form in exact mode
 *   "fetch_blocks"             64        k_plan_fetch's workgroups beside a device-wide launch (0: one per 256 entries)
 *   "fetch_avoid"              1         k_plan_fetch's workgroups decline on the XCD of a one-XCD launch
 *   -- exact-mode plan producers --
 *   "mt_pipeline"              -1        -1: host pipeline, finisher threads from the core count; k > 0: k finishers; 0: inline, calling thread
 *   "mt_device_finish"         1         0: the finisher threads convert every draw (1: k_plan_raw does, on the device)
 *   "mt_regen_min_walkers"     16384     stretch steps of ensembles this large go up as generator STATES (k_plan_regen makes the draws again); 0: never
 *   "mt_device"                1         0: never the device producer; 1: from "mt_device_min_walkers" (147456) on -- from "mt_device_min_walkers_regen"
 *                                        (786432) where the host pipeline's stretch steps are regen steps; 2: from 8192 on
 *   "persist_exact_regen_max_walkers"  131072   exact mode: largest ensemble of the device-wide persistent form when its plans go up as generator states
 *   "mt_tok_wshift" / "mt_tok_tail"  11 / 2048   the device tokenizer's window rule    "mt_device_lookahead"  batches ahead
 *   -- summaries --
 *   "summary_compact"          1         emx_summary's order statistics: 0 every pass reads the chain, 1 passes 2 ... 7 read a compacted list where at
 *                                        most a quarter of the selection is left, 2 wherever the list's table fits (no bit depends on it)
 *   "hist_chunk_rows"          0 (auto)  emx_histograms: selected rows a chunk of the one-byte bin-code plane (auto: about 256 MB of codes); no count
 *                                        depends on it
 *   -- exchanges --
 *   "direct_timeout_ms"        bound of the device-side barriers of the direct and replay exchanges (the first of an emx_run: 6x)
 *   "replay_two_pass"          0         1: the replay exchange's own pass and replay pass as separate launches
 *   -- tests / instrumented builds only --
 *   "persist_test_skew", "test_fetch_delay_us"   make a barrier unmeetable / a fetch late (tests of the give-up and wait paths)
 *   "phase_clock"              0         instrumented builds (-DEMX_OPT_STAMPS=1): phase timestamps of every launch
 *   "ablate"                   0         experiments flavour only (EMX_BUILD_FLAVOUR=exp, -DEMX_EXPERIMENTS=1): skip-phase masks; refused otherwise
 *
 * After a barrier timeout (status bit 3) the context refuses further sharded half-steps until the peers are attached again
 * (emx_direct_export / _import or _attach on every rank). */
int emx_set_tuning(emx_ctx* ctx, const char* key, int64_t value);

/* ---- state: State(coords, log_prob) (state.py:10-45) ---------------------------------- */
int emx_set_state(emx_ctx* ctx, const double* coords, const double* log_prob /* or NULL */);
int emx_get_state(emx_ctx* ctx, double* coords /* or NULL */, double* log_prob /* or NULL */);
int emx_get_accepted(emx_ctx* ctx, uint8_t* mask /* N */); /* `accepted` of the last propose */
/* Snapshots (slots 0..7): run_mcmc returns a State and accepts it back (ensemble.py:441-447, 312) -- a State that is the
 * device state needs no PCIe round trip.  The host layer hands out a lazy State; when a later call is about to change the
 * ensemble while that object is still alive, emx_snapshot_save keeps its values in HBM (device-to-device copy on the context
 * stream); emx_snapshot_read materialises them on demand, emx_snapshot_restore makes a snapshot the current state again. */
int emx_snapshot_save(emx_ctx* ctx, int32_t slot);
int emx_snapshot_read(emx_ctx* ctx, int32_t slot, double* coords /* or NULL */, double* log_prob /* or NULL */);
int emx_snapshot_restore(emx_ctx* ctx, int32_t slot);
int emx_snapshot_free(emx_ctx* ctx, int32_t slot);

/* The caller's own batched log-prob, on device memory: the reference's vectorize=True contract -- ONE call of log_prob_fn on the
 * (Ns, ndim) block of a split's proposals (ensemble.py:486-487, called at red_blue.py:93) -- without the block or the result
 * leaving HBM.  The function is called on the host thread that drives the step; it must ENQUEUE work on `hip_stream` (a kernel
 * launch, a library call) that reads the n rows of coords_dev (row-major, ndim doubles each, in the order the reference passes
 * them: ascending walker index within the split) and writes n log-probabilities to log_prob_dev, and return 0 (non-zero aborts
 * the step with an error).  It must not synchronise.  -inf is a legal value, NaN raises the reference's error.  Replaces the
 * closed-form target: emx_run, emx_halfstep, emx_eval_log_prob and the all-gather / log-prob / replay exchanges work over it. */
typedef int (*emx_device_log_prob_fn)(void* user, const double* coords_dev, int64_t n, int32_t ndim, double* log_prob_dev,
                                      void* hip_stream);
int emx_set_target_callback(emx_ctx* ctx, emx_device_log_prob_fn fn, void* user);
/* Fused user targets of a single ensemble (EMX_TARGET_FUSED_ENSEMBLE; emcee_amd.targets.DeviceFused / compile_fused_ensemble):
 * the caller's per-row __device__ log-probability compiled INTO the half-step kernel, so that a half-step is ONE launch --
 * proposal, the caller's function on the row staged in LDS, decision, commit -- where the callback target above takes three and
 * sends the proposal block through memory.  The caller's translation unit includes emcee_amd/csrc/emx_fused_ensemble.hpp and emits
 * a launcher with EMX_FUSED_ENSEMBLE_TARGET(name, Functor, ndim), 1 <= ndim <= 256; the library fills the descriptor below and calls
 * the launcher where it launches its own element-wise half-step, and for every evaluation of rows (the initial log-probs, the
 * log-prob pass of WalkMove / KDEMove).  `args` is the library's internal HalfStepArgs: `abi` (EMX_FUSED_ENSEMBLE_ABI of that
 * header, bumped with any change of the struct or of the launch rules) and `args_bytes` (its sizeof) are checked by the launcher
 * against the values it was compiled with, so a launcher built against another version of the header -- or a launcher of the batch
 * targets, whose descriptors start with the same two fields and carry other constants -- is refused, never run.  grid == 0 is a
 * probe: check abi, args_bytes, ndim and move, launch nothing.  Otherwise `grid` is the most workgroups the launch may use,
 * `threads` and `lds_bytes` the workgroup size and the dynamic LDS the header's rules give for ndim (the launcher refuses others).
 * Returns 0, or non-zero and nothing launched (1: another version of the header, 2: another ndim, 3: a move or launch shape that
 * was not compiled in, 5: args that carry an exchange, a graph descriptor or a device-side slot count, 100 + a hipError_t: the
 * launch failed).  emx_set_target_fused probes once, so a mismatch surfaces at bind time (-8 and "built against another version of
 * emx_fused_ensemble.hpp").  `user_dev`: a device pointer handed to the functor with every row; the caller keeps it alive.
 * Such a context runs one launch per half-step (never the persistent kernels or a step graph) in either rng mode -- or, with a
 * one-workgroup launcher bound and an ensemble that fits (emx_set_target_fused_small below), one launch per chunk of steps;
 * results are bit for bit those of emx_set_target_callback with the same function either way.  One replica only:
 * emx_set_shard / emx_comm_init on such a context, and this call on a sharded one, are refused. */
typedef struct emx_fused_ensemble_launch {
    uint32_t abi;            /* EMX_FUSED_ENSEMBLE_ABI the library was built with */
    uint32_t args_bytes;     /* sizeof(HalfStepArgs) of the library */
    int32_t ndim, move, grid, threads;      /* move: EMX_MOVE_STRETCH / DE / SNOOKER / GAUSS, or 4: evaluate rows */
    uint64_t lds_bytes;
    void* hip_stream;
    const void* args;        /* HalfStepArgs */
    const void* user;        /* user_dev */
} emx_fused_ensemble_launch;
typedef int (*emx_fused_ensemble_fn)(const emx_fused_ensemble_launch*);     /* 0, or non-zero and nothing launched */
int emx_set_target_fused(emx_ctx* ctx, emx_fused_ensemble_fn launcher, const void* user);
/* The same target with blobs: nblobs (1 ... 32) float64 derived quantities a sample, written by the functor's five-argument form
 * (x, ndim, member, user, double* blobs) in the call that returns the log-probability, committed where the log-probability is
 * committed and appended to a blob plane (capacity, N, nblobs) next to the chain.  The caller's translation unit emits the launcher
 * with EMX_FUSED_ENSEMBLE_TARGET_BLOBS(name, Functor, ndim, nblobs).  The descriptor's leading fields are those of
 * emx_fused_ensemble_launch; `abi` is EMX_FUSED_ENSEMBLE_BLOBS_ABI, a constant of its own, so each launcher answers 1 to the other's
 * descriptor.  blobs_cur: the walkers' current blobs (N, nblobs) -- or, for an evaluation of rows, the block's; blobs_row: the
 * plane's row of a stored step, NULL on an unstored one.  Answers as above, and 4: another number of blobs.
 * emx_set_target_fused_blobs probes once (-1 and "another number of blobs" on answer 4); nblobs == 0 is emx_set_target_fused with
 * a launcher of that type.  A sharded context is refused, and so is a change of the blob count while stored steps exist.  Blob
 * values are not validated.  A WalkMove / KDEMove in the schedule of a context with blobs is refused (emx_set_moves, emx_run). */
typedef struct emx_fused_ensemble_blobs_launch {
    uint32_t abi;            /* EMX_FUSED_ENSEMBLE_BLOBS_ABI the library was built with */
    uint32_t args_bytes;     /* sizeof(HalfStepArgs) of the library */
    int32_t ndim, move, grid, threads;
    uint64_t lds_bytes;
    void* hip_stream;
    const void* args;        /* HalfStepArgs */
    const void* user;        /* user_dev */
    int32_t nblobs, reserved;
    double* blobs_cur;
    double* blobs_row;
} emx_fused_ensemble_blobs_launch;
typedef int (*emx_fused_ensemble_blobs_fn)(const emx_fused_ensemble_blobs_launch*);
int emx_set_target_fused_blobs(emx_ctx* ctx, emx_fused_ensemble_blobs_fn launcher, const void* user, int32_t nblobs);
/* The same target for a log-probability that sums over data: log p(x) = base(x) + sum_k term(x; datum k), k < ndata.  The caller's
 * translation unit includes emcee_amd/csrc/emx_fused_ensemble_data.hpp and emits the launcher with
 * EMX_FUSED_ENSEMBLE_DATA_TARGET(name, Model, ndim) around a model with `base` and `term` members; k_halfstep_user_data then gives
 * every row a WAVE for the data sum (one lane calls base, 64 lanes stride over the data, a fixed pairwise tree adds the lane
 * partials -- the header defines the order, so the value depends on nothing but x, the data and ndata) where the launcher above
 * loops in one lane.  The descriptor is one of its own: the fields of emx_fused_ensemble_launch, then `ndata` (0 <= ndata < 2^31, a
 * run-time value: the one given to emx_set_target_fused_data) and `rows`, the slots a workgroup takes at once (4 ... the header's
 * tile for ndim; lds_bytes is the header's fused_ens_lds_of(ndim, rows)).  `abi` is EMX_FUSED_ENSEMBLE_DATA_ABI, a constant of its
 * own, so a data launcher and a data-free launcher answer 1 to each other's descriptor.  grid == 0 is the host-only probe; the
 * answers are emx_fused_ensemble_fn's.  emx_set_target_fused_data probes once and refuses another header version or ndim with
 * emx_set_target_fused's wording, refuses a sharded context, frees blob storage and unbinds a blob and a one-workgroup launcher:
 * such a target has no blobs and always runs one launch a half-step.  The rows a workgroup come from the split's length and the
 * CU count (fused_ens_data_rows_rule of the header) unless the tuning key "fused_data_rows" names them (0: the rule; else 4 ... 256,
 * clamped to the tile); results do not depend on them. */
typedef struct emx_fused_ensemble_data_launch {
    uint32_t abi;            /* EMX_FUSED_ENSEMBLE_DATA_ABI the library was built with */
    uint32_t args_bytes;     /* sizeof(HalfStepArgs) of the library */
    int32_t ndim, move, grid, threads;
    uint64_t lds_bytes;
    void* hip_stream;
    const void* args;        /* HalfStepArgs */
    const void* user;        /* user_dev */
    int64_t ndata;
    int32_t rows, reserved;
} emx_fused_ensemble_data_launch;
typedef int (*emx_fused_ensemble_data_fn)(const emx_fused_ensemble_data_launch*);
int emx_set_target_fused_data(emx_ctx* ctx, emx_fused_ensemble_data_fn launcher, const void* user, int64_t ndata);
/* Small ensembles of a fused user target: whole emx_run calls inside ONE workgroup (k_small_run around the caller's functor:
 * ensemble, plans, log-probs and blobs in LDS), one launch per chunk of up to 4 096 steps where the half-step launcher takes two
 * launches a step, in both rng modes, bit for bit the same chain.  Opt-in: the caller's translation unit also emits
 * EMX_FUSED_ENSEMBLE_SMALL_TARGET(name, Functor, ndim) or ..._SMALL_TARGET_BLOBS(name, Functor, ndim, nblobs) (four more kernels to
 * compile), and the launcher is bound here AFTER emx_set_target_fused[_blobs], which keeps the initial log-probs, every evaluation
 * of rows and the ensembles that do not fit (binding a target unbinds the small launcher; NULL unbinds it).  The descriptor is
 * emx_fused_launch (below, with the batch targets) with `args` the library's SmallRunArgs, `abi` EMX_FUSED_ENSEMBLE_SMALL_ABI of
 * emx_fused_ensemble.hpp -- a constant of its own, so a batch launcher is refused, never run --, grid 1 (0: the probe)
 * and `reserved` 1 when the plans are those of the host's MT19937 twin (exact mode), 0 for Philox plans.  Answers: emx_fused_batch_fn's.
 * The probe checks version, ndim and the context's blob count: -8 / -1 with the wording of the other fused binds.
 * The one-workgroup path CAN be taken when emx_small_fused_check accepts the shape: "small_kernel" on, one replica, StretchMove / DEMove
 * (every complement >= 2) / DESnookerMove, a GaussianMove in Philox mode only (WalkMove / KDEMove keep the half-step path), and
 *   small_lds_bytes(N, ndim) + small_fused_stage_bytes(largest split, ndim) + small_blob_bytes(N, nblobs) <= 150 KB
 * (emx_small_host.hpp).  It IS taken where it also pays (emx_small_fused_pays: one lane a row calls the functor and commits, so the
 * kernel's step time grows with ndim -- measured, profiles/ensemble_fused_small.md: with Philox plans ndim <= 10 and nwalkers x ndim
 * <= 1 024, with the host's MT19937 plans ndim <= 16), or wherever it fits with the tuning key "small_kernel" = 2 (tests,
 * experiments).  Otherwise, for emx_step_begin steps and for an emx_run of a single step, nothing changes. */
struct emx_fused_launch;
typedef int (*emx_fused_small_fn)(const struct emx_fused_launch*);      /* an emx_fused_batch_fn */
int emx_set_target_fused_small(emx_ctx* ctx, emx_fused_small_fn small_launcher);
/* the rule above as a host-only predicate (rng_mode: EMX_RNG_*): 0, or -1 and the reason in msg */
int emx_small_fused_check(int64_t nwalkers, int32_t ndim, int32_t nmoves, const emx_move_desc* moves, int32_t rng_mode, int32_t nblobs,
                          char* msg, int32_t msglen);
/* 1 where the one-workgroup kernel of a fused user target is the faster path at this shape and rng mode (host only), else 0 */
int emx_small_fused_pays(int64_t nwalkers, int32_t ndim, int32_t rng_mode);
/* the one-workgroup kernel of this context, any target: out[0] launches and out[1] the steps run in them since emx_create;
 * out[2], out[3]: 0 */
int emx_small_info(emx_ctx* ctx, int64_t out[4]);
/* the walkers' current blobs (N, nblobs) of such a context: nblobs_out (may be NULL) receives the count, 0 without blobs; out may
 * be NULL to ask for the count alone */
int emx_get_blobs(emx_ctx* ctx, double* out, int32_t* nblobs_out);
int emx_set_blobs(emx_ctx* ctx, const double* in);
/* emx_eval_log_prob, and the rows' blobs (n, nblobs) */
int emx_eval_log_prob_blobs(emx_ctx* ctx, const double* coords, int64_t n, double* lp_out, double* blobs_out);
/* the blobs (N, nblobs) a snapshot slot carries (emx_snapshot_save / _restore copy them with coords and log_prob) */
int emx_snapshot_read_blobs(emx_ctx* ctx, int32_t slot, double* blobs);

/* ---- target: the batched log-prob (ensemble.py:458-553, vectorised) -------------------- */
/* p0/p1: DIAG (mu, ivar); DENSE (mu, icov[D*D], symmetric positive definite: factored once as
 * L L^T, the kernel evaluates -0.5 |L^T (x-mu)|^2 with f64 MFMAs: fused into the half-step kernel up to
 * ndim 112, as a log-prob kernel of its own between propose and commit up to ndim 2048); others NULL.
 * scale: Rosenbrock divisor. */
int emx_set_target(emx_ctx* ctx, int32_t kind, const double* p0, const double* p1, double scale);
/* log-prob of the current state, stored as the state's log_prob (ensemble.py:350-351); a target with blobs fills the state's blobs */
int emx_eval_state_log_prob(emx_ctx* ctx);
/* EnsembleSampler.compute_log_prob(coords) for n host rows (n <= nwalkers per call) */
int emx_eval_log_prob(emx_ctx* ctx, const double* coords, int64_t n, double* out);

/* ---- moves & RNG ------------------------------------------------------------------------ */
/* ensemble.py:115-129: move list + normalised cumulative weights (cdf[nmoves-1] == 1) */
int emx_set_moves(emx_ctx* ctx, int32_t nmoves, const emx_move_desc* moves, const double* cdf);
int emx_set_rng_mode(emx_ctx* ctx, int32_t mode);
/* EMX_MOVE_GAUSS: per-coordinate standard deviations (n == ndim; NULL / 0 restores the isotropic sigma) */
int emx_set_move_scale(emx_ctx* ctx, int32_t move_index, const double* std, int32_t n);
/* current descriptor of a move (the sequential Gaussian cursor lives in it) */
int emx_get_move(emx_ctx* ctx, int32_t move_index, emx_move_desc* out);
/* numpy RandomState.get_state()/set_state() tuple round trip (ensemble.py:216-238) */
int emx_rng_set_mt19937(emx_ctx* ctx, const uint32_t key[624], int32_t pos, int32_t has_gauss, double cached);
int emx_rng_get_mt19937(emx_ctx* ctx, uint32_t key[624], int32_t* pos, int32_t* has_gauss, double* cached);
int emx_rng_set_philox(emx_ctx* ctx, uint64_t seed, uint64_t step);
int emx_rng_get_philox(emx_ctx* ctx, uint64_t* seed, uint64_t* step);

/* ---- the hot loop (ensemble.py:403-424): nsteps stored steps, nsteps*thin_by proposals -- */
int emx_chain_config(emx_ctx* ctx, int64_t capacity_steps); /* Backend.grow (backend.py:164-185) */
int emx_chain_reset(emx_ctx* ctx);                            /* Backend.reset (backend.py:19-35) */
int emx_run(emx_ctx* ctx, int64_t nsteps, int32_t thin_by, int32_t store);
int emx_iteration(emx_ctx* ctx, int64_t* stored_steps, int64_t* proposals);
/* With tuning key "graph" = 1, emx_run replays the native 16-step block (plan kernel + 16 x nsplits
 * half-steps, per-replay state in device memory) as ONE hipGraph launch when it can (Philox, one move,
 * thin_by 1, one rank).  Off by default: measured 5 % slower than back-to-back launches on MI355X unless
 * the host is the bottleneck (a busy or slow host thread); results are bit-identical either way.  captured: bit0 no-store graph, bit1 store graph. */
int emx_graph_state(emx_ctx* ctx, int32_t* disabled, int32_t* captured);
/* Backend.get_value slices (backend.py:42-58): steps start, start+stride, ... < stop.
 * what: 0 chain -> out[(nsel, N, D)], 1 log_prob -> out[(nsel, N)], 2 blobs -> out[(nsel, N, nblobs)] (a context with blobs). */
int emx_chain_read(emx_ctx* ctx, int32_t what, int64_t start, int64_t stop, int64_t stride, double* out);
int emx_accepted_counts(emx_ctx* ctx, double* out /* N, backend.accepted */);

/* ---- split-phase stepping: Move.propose pieces for host log-probs and sharded runs ------ */
/* Begin a step: choose the move (ensemble.py:406), build the split plan (red_blue.py:76-80 and
 * every draw of the step).  move_out/nsplits_out report the choice. */
int emx_step_begin(emx_ctx* ctx, int32_t store_this_step, int32_t* move_out, int32_t* nsplits_out);
/* same, for a move the caller already chose (Move.propose called directly: no choice draw) */
int emx_step_begin_with(emx_ctx* ctx, int32_t store_this_step, int32_t move_index, int32_t* nsplits_out);
/* fused half-step on the device target (red_blue.py:81-104 for one split) */
int emx_halfstep(emx_ctx* ctx, int32_t split);
/* host-target variant: proposals q (ns, D) in ascending-walker order (red_blue.py:90) ... */
int emx_propose(emx_ctx* ctx, int32_t split, double* q_out, double* factors_out /* or NULL */, int64_t* ns_out);
/* ... and Metropolis accept + commit given their log-probs (red_blue.py:96-104) */
int emx_accept(emx_ctx* ctx, int32_t split, const double* new_log_prob);
/* user-defined RedBlueMove.get_proposal: q (ns, D) and factors (ns) come from the caller */
int emx_accept_proposals(emx_ctx* ctx, int32_t split, const double* q, const double* factors,
                         const double* new_log_prob);
int emx_step_end(emx_ctx* ctx);
/* INPUTS mode / tests: set or read back the plan of the step begun (arrays of length N in
 * plan order: split 0's members ascending, then split 1's, ...; off has nsplits+1 entries) */
int emx_plan_set(emx_ctx* ctx, int32_t move_index, const int32_t* off, const int32_t* order, const int32_t* p0,
                 const int32_t* p1, const int32_t* p2, const double* s0, const double* uacc);
int emx_plan_get(emx_ctx* ctx, int32_t* off, int32_t* order, int32_t* p0, int32_t* p1, int32_t* p2, double* s0,
                 double* uacc);
/* INPUTS mode, EMX_MOVE_GAUSS: after emx_plan_set (off = {0, N}, order = walker of each slot, p0 = coordinate
 * that moves or -1, uacc), the (N, D) standard normals rng.randn(N, D) and the step-size factor (1 if unused);
 * the library forms (factor * scale_d) * n on the device (gaussian.py:87) */
int emx_plan_set_noise(emx_ctx* ctx, const double* normals, double factor);

/* ---- walker-sharded multi-GPU (one process per GPU; collectives stay in the host layer) -- */
int emx_set_shard(emx_ctx* ctx, int32_t rank, int32_t world);
/* use caller-owned device buffers (e.g. torch tensors handed to RCCL) for the exchange:
 * sendbuf (rows_per_rank, D+2), gathered (world*rows_per_rank, D+2); records = [row | log_prob | accepted] */
int emx_set_shard_buffers(emx_ctx* ctx, void* sendbuf, void* gathered, int64_t rows_per_rank);
/* raw device pointers for zero-copy wrapping (torch.distributed all-gather buffers):
 * which: 0 coords (N,D), 1 log_prob (N), 2 sendbuf (rows/rank, D+2), 3 gathered (world*rows/rank, D+2),
 *        4 chain (stored, N, D), 5 chain log_prob (stored, N), 6 Gaussian-move displacements (N, D),
 *        8 direct-exchange barrier flags (one uint64 per rank),
 *        16 + r: slot r of the plan ring, one block of 48 N bytes: [order|p0] int32, [s0|uacc] f64, [p1|p2] int32, [logu|fac] f64 */
int emx_device_ptr(emx_ctx* ctx, int32_t which, void** ptr, int64_t* nbytes);
int emx_shard_slots(emx_ctx* ctx, int32_t split, int64_t* t_lo, int64_t* t_hi, int64_t* ns);
/* after the all-gather of `sendbuf`s into `gathered`: write the other ranks' rows into X */
int emx_scatter_gathered(emx_ctx* ctx, int32_t split);

/* ---- pull exchange: walker-block ownership, only the partner rows that are read travel -----
 * The all-gather above replicates every updated row on every rank: (G-1)/G of the ensemble crosses
 * xGMI per step.  A half-step reads ONE partner row per updated walker (stretch.py:32; two / three for
 * DE / snooker), so with rank r owning walkers [N r / G, N (r+1) / G) it is enough to move exactly those
 * rows.  The RNG plan is replicated, hence every rank knows which of its rows the others will read:
 *   emx_pull_prepare(split)  -> records [row index | row] for every peer in the send buffer
 *                               (world blocks of *records_per_peer records of D+1 doubles)
 *   all-to-all, records_per_peer * (D+1) doubles per pair (host layer, or emx_run when emx_comm_init ran)
 *   emx_pull_apply(split)    -> received rows into the local replica, then the half-step over the
 *                               slots whose walker this rank owns
 * Only a rank's own block of X / log_prob / accepted / chain is current until emx_replica_pack ->
 * all-gather (bmax records of D+3 doubles per rank) -> emx_replica_unpack re-synchronises the replicas
 * (emx_run does it before it returns).  Results are bit-identical to the single-rank run. */
#define EMX_EXCHANGE_ALLGATHER 0
#define EMX_EXCHANGE_PULL 1
#define EMX_EXCHANGE_DIRECT 2      /* see "direct exchange" below */
#define EMX_EXCHANGE_LOGPROB 3     /* see "log-prob exchange" below */
#define EMX_EXCHANGE_REPLAY 4      /* see "replay exchange" below */
int emx_set_exchange(emx_ctx* ctx, int32_t kind);          /* before emx_set_shard / emx_comm_init */
/* doubles the send / receive buffers must hold for the moves installed (pull exchange) */
int emx_exchange_layout(emx_ctx* ctx, int64_t* send_doubles, int64_t* recv_doubles);
/* caller-owned exchange buffers (pull exchange), e.g. torch tensors handed to RCCL */
int emx_set_exchange_buffers(emx_ctx* ctx, void* send, int64_t send_doubles, void* recv, int64_t recv_doubles);
int emx_own_walkers(emx_ctx* ctx, int64_t* lo, int64_t* hi);
int emx_pull_prepare(emx_ctx* ctx, int32_t split, int64_t* records_per_peer);
int emx_pull_apply(emx_ctx* ctx, int32_t split);
int emx_replica_pack(emx_ctx* ctx, int64_t* records_per_rank);
int emx_replica_unpack(emx_ctx* ctx);

/* ---- direct exchange: partner rows read in place from the owner's HBM over xGMI ----------------------------------
 * Same walker-block ownership as the pull exchange, but nothing is packed, sent or scattered: every rank maps the other
 * ranks' coordinate arrays (hipIpc handles between processes, plain pointers between contexts of one process) and the
 * half-step kernel loads a partner row from the replica of the rank that owns it (stretch.py:32 reads ONE row per updated
 * walker, de.py:53 two, de_snooker.py:41-46 three) -- the only bytes that cross xGMI are the (G-1)/G of those rows that
 * live on another GPU.  Between half-steps a one-wave device-side barrier (a flag store into every peer's flag array, a
 * spin on the own array; bounded by tuning key "direct_timeout_ms", status bit 3 on expiry) orders the two hazards of
 * red_blue.py:85,104: a partner row must carry its owner's last commit, and nobody may start committing split k+1 while a
 * peer still reads those rows as partners of split k.
 *   emx_set_exchange(EMX_EXCHANGE_DIRECT); emx_set_shard / emx_comm_init; then
 *   multi-process: emx_direct_export -> 128 bytes per rank, all-gathered by the host layer -> emx_direct_import
 *   one process:   emx_direct_attach(coordinate arrays, flag arrays) of all ranks (emx_device_ptr which = 0 / 8)
 *   per step:      emx_step_begin; emx_direct_halfstep(split, barrier) for every split; emx_step_end   (emx_run does it)
 * Only a rank's own block is current until the replica re-synchronisation (emx_replica_pack / all-gather / unpack; emx_run
 * runs it before it returns when emx_comm_init was called).  Results are bit-identical to the single-rank run.  World size
 * <= 8 (one node). */
int emx_direct_export(emx_ctx* ctx, uint8_t handles[128]);
int emx_direct_import(emx_ctx* ctx, const uint8_t* handles /* world * 128 bytes, rank order */);
int emx_direct_attach(emx_ctx* ctx, void* const* peer_coords /* [world] */, void* const* peer_flags /* [world] or NULL */);
/* barrier != 0: device-side barrier with the peers first (needs their flag arrays); 0: the caller orders the ranks itself */
int emx_direct_halfstep(emx_ctx* ctx, int32_t split, int32_t barrier);

/* ---- log-prob exchange: the reference's own parallel model (ensemble.py:486-496: pool.map over the proposals) ------------
 * Proposal, decision and commit are replicated -- every rank holds the whole ensemble and the same plan, so every rank computes
 * the same proposals -- and only the log-probability evaluations are shared out: rank r evaluates the proposals
 * [r * per, (r + 1) * per) of the split, per = ceil(ns / world).  What travels is 8 bytes per walker-update (an in-place
 * all-gather of `per` doubles per rank on the buffer emx_device_ptr(which = 3) returns), never a coordinate; the replicas stay
 * identical, so there is nothing to re-synchronise.  The protocol for targets whose evaluation dominates the step (wide dense
 * Gaussians here); for the cheap closed-form targets of the BASELINE configurations the replicated part is most of the step.
 *   emx_set_exchange(EMX_EXCHANGE_LOGPROB); emx_set_shard / emx_comm_init; per step:
 *   emx_step_begin; for every split: emx_logprob_begin(split, &per) -> all-gather(in place, per doubles per rank)
 *   -> emx_logprob_finish(split); emx_step_end   (emx_run does it when emx_comm_init ran).
 * Results are bit-identical to the single-rank run. */
int emx_logprob_begin(emx_ctx* ctx, int32_t split, int64_t* per_rank);
int emx_logprob_finish(emx_ctx* ctx, int32_t split);

/* ---- replay exchange: the DECISIONS travel (8 bytes per walker-update), every replica recomputes the accepted updates ------
 * Full replicas, slot-range ownership as in the all-gather exchange -- but where that one ships every updated row to every rank
 * ((G-1) * 8 (D+2) bytes per walker-update over xGMI), this one ships what the owner decided: the new log-prob of an accepted
 * proposal, NaN for a rejected one.  A proposal (stretch.py:33, de.py:53-62, de_snooker.py:41-46, gaussian.py:87) is a function
 * of rows every replica holds identically before the half-step and of the replicated plan, so after the all-gather of the
 * decisions every rank replays the accepted updates of the others on its own replica and obtains the owner's bits; the
 * log-probability is evaluated once, by the owner.  Extra HBM work per rank: the accepted fraction of the other ranks' slots
 * (24 D + 8 bytes each, no target evaluation) -- which is what makes it the protocol for BOTH regimes: cheap targets (nothing
 * crosses xGMI but 8 (G-1) bytes per update) and expensive ones (the evaluation is shared out like the log-prob exchange's, and
 * unlike there proposal and commit are shared out too).  Replicas stay identical: stored chains are complete on every rank.
 *   emx_set_exchange(EMX_EXCHANGE_REPLAY); emx_set_shard / emx_comm_init; per step:
 *   emx_step_begin; for every split: emx_replay_begin(split, &rows) -> all-gather of `rows` doubles per rank, send buffer
 *   emx_device_ptr(which = 2) into emx_device_ptr(which = 3) -> emx_replay_finish(split); emx_step_end
 *   (emx_run does it when emx_comm_init ran).  Results are bit-identical to the single-rank run. */
int emx_replay_begin(emx_ctx* ctx, int32_t split, int64_t* rows_per_rank);
int emx_replay_finish(emx_ctx* ctx, int32_t split);
/* The same exchange without a collective library (one node): after emx_direct_export / emx_direct_import (or emx_direct_attach)
 * -- which under this exchange map every rank's RECEIVE buffers (emx_device_ptr which = 3: two of them, used alternately) and
 * barrier flags -- emx_replay_exchange(split) replaces the all-gather: a kernel stores the decisions into every peer's buffer
 * over xGMI (8 bytes per own walker-update and peer) and the one-wave device-side barrier of the direct exchange tells every
 * rank that all of them have landed.  No host round trip, no collective launch latency; emx_run uses it when the peers are
 * mapped.  Between emx_replay_begin and emx_replay_finish. */
int emx_replay_exchange(emx_ctx* ctx, int32_t split);

/* RCCL driven by the library itself (ncclAllGather enqueued on the context stream between the
 * half-step kernels, so that emx_run covers sharded runs with no host round trip per step).
 * librccl is resolved with dlopen (path, $EMX_RCCL_LIB, librccl.so.1): pass PyTorch's copy when
 * torch is loaded so that the process holds ONE RCCL.  Rank 0 creates the id, the host layer
 * broadcasts its 128 bytes, every rank calls emx_comm_init. */
int emx_comm_load(const char* librccl_path /* or NULL */);
int emx_comm_get_unique_id(uint8_t id[128]);
int emx_comm_init(emx_ctx* ctx, int32_t rank, int32_t world, const uint8_t id[128]);
int emx_comm_destroy(emx_ctx* ctx);
/* ranks of the communicator emx_comm_init created, as RCCL itself counts them (ncclCommCount) -- what a bench line may claim
 * as its number of GPUs; 0 when no communicator exists */
int emx_comm_count(emx_ctx* ctx, int32_t* ranks_out);

/* ---- around the hot loop: autocorrelation time and the initial-state check ------------------------------------------ */
/* Integrated autocorrelation time of the device-resident chain, per parameter (autocorr.py:49-123 integrated_time applied to
 * Backend.get_value("chain", discard, thin), backend.py:42-58,130-150): normalised FFT autocorrelation function of every
 * walker's series (batched hipFFT next to the chain), averaged over walkers, Sokal window with step size c.  tau_out[ndim] is
 * in units of the SELECTED samples (the caller multiplies by thin, backend.py:150); window_out[ndim] (or NULL) the windows;
 * *nsamples_out the series length, against which the caller applies the reference's "tol" check (autocorr.py:110-121).
 * libhipfft is resolved with dlopen (emx_fft_load(path), $EMX_HIPFFT_LIB, libhipfft.so): pass PyTorch's copy when torch is
 * in the process. */
int emx_fft_load(const char* libhipfft_path /* or NULL */);
int emx_autocorr(emx_ctx* ctx, int64_t discard, int64_t thin, double c, double* tau_out, int32_t* window_out,
                 int64_t* nsamples_out);
/* walkers_independent(coords) (ensemble.py:653-663): centre, scale by max |.| and by the 2-norm per coordinate, condition
 * number <= 1e8.  The (n, ndim) host matrix goes to `device`; Householder QR there (one reflector per coordinate), then the
 * extreme singular values of the ndim x ndim triangular factor by (inverse) power iteration on the host.  *independent: 0 / 1;
 * *cond_out (or NULL): the condition number (inf for a constant coordinate, non-finite input, n < ndim or a singular factor). */
/* Posterior summaries of the device-resident chain over stored rows start, start + stride, ... < stop and every walker
 * (n = rows x nwalkers samples; *nsamples_out), computed next to the chain -- what emx_summary_batch returns for a member of a
 * batch, by kernels that tile over walkers (csrc/emx_summary_single.hpp): mean_out (W), cov_out (W, W) (ddof = 1, symmetric bit
 * for bit, W <= 256), order_out (nranks, W): the ranks[r]-th smallest (0-based, at most 32 ranks) of every column, exactly;
 * map_coords_out (W) / map_log_prob_out: the stored sample of the largest stored log-prob, the smallest (row, walker) among
 * equals.  plane: 0 coordinates (W = ndim), 2 blobs (W = nblobs; emx_chain_read's numbering).  Outputs may be NULL, which skips
 * the work.  The floating-point sums run in an order fixed by (rows, nwalkers, W); no bit depends on the launch shape or on the
 * tuning key "summary_compact" (1; 0: the selection's passes 2 ... 7 read the chain instead of a compacted list, 2: the list
 * wherever it fits).  Scratch stays on the context.  -1 for bad arguments, -2 for a device failure. */
int emx_summary(emx_ctx* ctx, int32_t plane, int64_t start, int64_t stop, int64_t stride, double* mean_out, double* cov_out,
                int32_t nranks, const int64_t* ranks, double* order_out, double* map_coords_out, double* map_log_prob_out,
                int64_t* nsamples_out);
/* What the order statistics of the context's last emx_summary call read: *selection_reads_out how many times the selected
 * elements were read from the chain (histogram passes, times the dim tiles of each, and the compaction), *listed_out the
 * length of the compacted list (-1: none was made), *list_reads_out how many times that list was read.  Outputs may be NULL. */
int emx_summary_info(emx_ctx* ctx, int64_t* selection_reads_out, int64_t* listed_out, int64_t* list_reads_out);
/* Split-R-hat of the context's device-resident chain over emx_summary's selection of rows, its nwalkers walkers as chains:
 * emx_rhat_batch's kernels (csrc/emx_rhat.hip, the definition is there) run with one member.  within_out, between_out: (W),
 * W = ndim + (log_prob != 0), the last column being the stored log-prob series'; *nchains_out = 2 nwalkers, *length_out =
 * h = nt / 2.  The caller forms rhat = sqrt((h - 1) / h + between / within).  The same fixed summation order, so the same bits
 * as a batch member holding the same chain.  -1 for bad arguments (fewer than 4 selected rows among them), -2 for a device
 * failure.  Scratch stays on the context. */
int emx_rhat(emx_ctx* ctx, int64_t start, int64_t stop, int64_t stride, int32_t log_prob, double* within_out, double* between_out,
             int64_t* nchains_out, int64_t* length_out);
/* Histograms of the device-resident chain over the rows and walkers of emx_summary's selection (plane 0: coordinates, W = ndim;
 * 2: blobs, W = nblobs), counted next to the chain (csrc/emx_hist.hpp).  The bin edges are the caller's and are never recomputed on
 * the device; a value v falls in bin b iff e[b] <= v < e[b + 1], the last bin closed on the right (np.histogram's rule); NaN,
 * +-inf beyond the edges and everything outside are counted nowhere.
 * emx_chain_minmax: per column the smallest and the largest FINITE value (+inf / -inf where there is none) and the number of
 * non-finite ones: lo_out[W], hi_out[W], nonfinite_out[W].  Exact, whatever the order of the reduction.
 * emx_histograms: column d's marginal edges are edges[edge_off[d] ... edge_off[d + 1]) (edge_off[0] = 0; 1 ... 1024 bins, strictly
 * increasing); its counts go to counts_out[edge_off[d] - d ...).  With npairs > 0: the pair edges pedge_off / pedges in the same
 * form (1 ... 128 bins a column), pairs[2 p], pairs[2 p + 1] the two different columns (i, j) of panel p, whose pb_i x pb_j counts
 * (column i the slow axis, a sample counted iff both coordinates fall in a bin) go to pair_counts_out[pair_off[p] ...),
 * pair_off[p + 1] - pair_off[p] = pb_i pb_j, pair_off[0] = 0.  *nsamples_out: rows x nwalkers.  The chain is read once whatever
 * the number of pairs: one pass bins every value and leaves a one-byte bin code per value in a dim-major plane, from which the
 * panels are counted; the selection goes in chunks of rows (tuning "hist_chunk_rows") so that this plane stays near 256 MB.
 * Every count is a sum of integers: no count depends on the launch shape, the chunking or the order of the atomics.  Scratch stays
 * on the context.  -1 for bad arguments, -2 for a device failure. */
int emx_chain_minmax(emx_ctx* ctx, int32_t plane, int64_t start, int64_t stop, int64_t stride, double* lo_out, double* hi_out,
                     int64_t* nonfinite_out);
int emx_histograms(emx_ctx* ctx, int32_t plane, int64_t start, int64_t stop, int64_t stride, const int64_t* edge_off,
                   const double* edges, int64_t* counts_out, const int64_t* pedge_off, const double* pedges, int64_t npairs,
                   const int32_t* pairs, const int64_t* pair_off, int64_t* pair_counts_out, int64_t* nsamples_out);
int emx_walkers_independent(int32_t device, const double* coords, int64_t n, int32_t ndim, int32_t* independent,
                            double* cond_out);
/* The same check on the state a context holds (a run continued from the State the previous run returned: the reference re-checks
 * every sample() call, ensemble.py:316-323) -- the ensemble is read where it is, nothing crosses PCIe.  A non-finite coordinate
 * shows as a non-finite entry of the factor (verdict 0). */
int emx_walkers_independent_resident(emx_ctx* ctx, int32_t* independent, double* cond_out);

/* ---- measurement ------------------------------------------------------------------------ */
int emx_timer_start(emx_ctx* ctx);                 /* hipEventRecord on the context stream */
int emx_timer_stop(emx_ctx* ctx, float* ms);       /* record + synchronize + elapsed       */
/* per-launch hipEvent timing of the half-step kernel: enable, run, then read the durations */
int emx_profile_enable(emx_ctx* ctx, int32_t max_launches);
int emx_profile_read(emx_ctx* ctx, float* ms_out, int32_t* n_inout);

/* exact (MT19937) mode: microseconds per produced step of the host plan pipeline's stages while it is alive -- out[0] wall
 * clock, [1] generator (twist + temper), [2] tokenizer (the serial walk of the stream: rejection tests), [3] finishers (summed
 * over the threads), [4] tokenizer waiting for words, [5] tokenizer waiting for a free staging buffer (i.e. for the consumer) */
int emx_pipeline_stats(emx_ctx* ctx, double out[6], int64_t* steps_produced, int32_t* finisher_threads);
/* how the host pipeline handed its stretch steps over so far (EMX_RNG_MT19937; moves/stretch.py:30-32, moves/red_blue.py:100 -- the
 * fixed-length draws of a step): raw_steps -- the draws as the generator words they are, in the plan's columns, finished on the
 * device (k_plan_raw; tuning "mt_device_finish"); of those, regen_steps -- not even the words: `order` and the generator's STATE at
 * every eighth block of the draws' region of the stream, from which the device makes the words again (k_plan_regen, round 6:
 * ensembles of "mt_regen_min_walkers" = 16 384 and more whose half is a power of two; 0: never).  Same plans bit for bit. */
int emx_pipeline_handovers(emx_ctx* ctx, int64_t* raw_steps, int64_t* regen_steps);

/* Exact (MT19937) mode with the plans made ON THE DEVICE (csrc/emx_mtdev.hpp): one StretchMove, one replica, ensembles of
 * 147 456 walkers or more (round 5; 131 072 before) -- where the serial host stages of "same seed => same chain as the reference" (ensemble.py:166-167,406,
 * moves/red_blue.py:76-80,100, moves/stretch.py:30-32) cost more than the kernels do.  MT19937 segments by jump-ahead, the rejection
 * tests of random.shuffle / randint and the Fisher-Yates swaps all run in kernels; no host thread touches a draw.  Tuning key
 * "mt_device": 0 = always the host pipeline, 1 (default) = from "mt_device_min_walkers" (147 456) on, 2 = from 8 192 walkers on
 * (measured, MI355X, 64-dim dense Gaussian: 65 536 walkers 94 us/step against the host pipeline's 69; 262 144 x 32: 192 against 316;
 * 1 048 576: 602 against 1 347 -- profiles/r04/mtdev_sizes.txt).
 *   out[0] 1 when the current configuration takes this producer, [1] 1 while one is alive, [2] steps taken from producers so far,
 *   [3] generation rounds, [4] stream segments (of 128 MT blocks), [5] batches of 16 steps produced, [6] tokenizer windows,
 *   [7] microseconds spent computing the jump polynomials (once per process)  -- [3..7] of the live or the last producer */
int emx_mtdev_info(emx_ctx* ctx, int64_t out[8]);
/* tests: raw pieces of the live producer after a synchronise.  what = 0: `n` tempered stream words from absolute position `arg`
 * (uint32 out); 1: the accepted Fisher-Yates targets J[i], i < nwalkers, of producer step `arg` (uint32 out, entry 0 unused);
 * 2: that step's positions -- nsplits * 3 (z words, randint words, accept words) then the position after the step (uint64 out) */
int emx_mtdev_debug(emx_ctx* ctx, int32_t what, int64_t arg, void* out, int64_t n);
/* the device tokenizer's work so far: out = windows decided | fixed-point rounds | 64-word groups of the one-wave tail | its ballot
 * rounds | then 10 ns ticks: waiting for stream windows | deciding the wide windows | the tail | the whole tokenizer kernels
 * (red_blue.py:80's masked rejection is the only serial part of a step: this is what it cost) */
int emx_mtdev_tok_stats(emx_ctx* ctx, int64_t out[8]);
/* host only: the MT19937 state key `k * stride_words` words after the block FOLLOWING `key` (k >= 1), by the jump polynomial
 * t^(k stride) mod phi applied to the 33-block window after `key` -- the host statement of what k_mt_jump computes */
int emx_host_mt_jump(const uint32_t key[624], uint64_t stride_words, int32_t k, uint32_t out_key[624]);

/* Persistent half-steps.  emx_run takes the headline shape -- stretch-move steps (red_blue.py:55-106 with stretch.py:27-34) and
 * DE-move steps (de.py:40-64) of two splits, snooker steps (de_snooker.py:31-46) of four, the
 * fused dense Gaussian target at an even ndim up to 64, Philox plans, one replica, nwalkers a multiple of 32 from 512 (tuning
 * "persist_min_walkers") to 256 x the CU count, i.e. one 16-walker tile per wave of a co-resident grid of about one workgroup
 * per CU -- up to 32 half-steps per kernel launch (in a mixture: the consecutive steps of one move -- the steps of a DEMove and a
 * DESnookerMove share launches, k_persist_mix, tuning "persist_mix" = 0: never; a launch goes on into the next batch of sixteen
 * steps of Philox plans, "persist_span" = 0: it ends with its batch; steps with another number of
 * splits take the per-half-step launches): a device-wide barrier stands where the kernel
 * boundaries were, and the next half-step's plan entries and own rows are loaded while this one computes.  Same draws, same
 * arithmetic, same bits as the launch-per-half-step path.  Tuning "persist" = 0 turns it off; "persist_timeout_ms" bounds a
 * barrier wait (default 2000: a grid that cannot become co-resident -- another process holding the device's CUs -- raises
 * status bit 3 instead of hanging).  With emx_profile_enable the events bracket whole launches.
 * A context whose only move is the Gaussian Metropolis move (gaussian.py:76-101 / mh.py:57-77; same target, RNG and replica
 * conditions, nwalkers a multiple of 16) runs up to 16 steps per launch with every walker in registers and no barrier at all
 * (k_persist_gauss).
 *   out[0] 1 when the current configuration qualifies, out[1] persistent launches so far, out[2] half-steps they ran,
 *   out[3] reserved (0) */
int emx_persist_info(emx_ctx* ctx, int64_t out[4]);
/* how many of those launches took the one-XCD form: ensembles of up to 8 192 walkers (stretch move, two splits) run an eight times
 * larger grid of which every eighth workgroup works -- all on one XCD, whose L2 keeps the walker state coherent with plain accesses and
 * a barrier of that XCD's own instead of agent-scope accesses and the device-wide barrier (tuning "persist_local" = 0: never;
 * "persist_local_max_walkers").  The element-wise targets (EMX_TARGET_ISO_GAUSS / _DIAG_GAUSS / _ROSENBROCK / _BOX, rows of 4 or 8 lanes:
 * ndim <= 64 even, <= 32 odd) have this form only (csrc/emx_pvalu.hip; tuning "persist_valu" = 0: never); same bits (red_blue.py:85,104: a half-step still sees every update of the one before).
 * EMX_RNG_MT19937 (the reference's own stream; ensemble.py:166-167) takes the one-XCD forms too -- and the device-wide forms of both
 * kernels up to 32 768 walkers ("persist_exact_max_walkers") -- when the context has ONE move: the
 * host pipeline's plans of up to sixteen steps ("persist_exact_steps") are fetched from their pinned staging buffers by one kernel
 * per launch (k_plan_fetch; its workgroups leave the XCD a one-XCD launch lives on alone, tuning "fetch_avoid" = 0: they do not; beside a
 * device-wide launch it runs as "fetch_blocks" = 64 workgroups, 0: one per 256 entries)
 * -- tuning "persist_exact" = 0: the per-half-step launches with an upload per step.  Move mixtures too
 * (round 5: the next step's move is read off the pipeline's plan before it is taken; "persist_exact_mix" = 0: one move only).  A
 * launch of this mode that cannot become resident is redone like a Philox one (round 5): the pipeline keeps the generator state
 * behind each of its last 64 steps and is taken back to the one in front of the launch.  Status bit 3 stays -- the run is void,
 * as for a barrier that timed out in the middle of a launch -- when that is not possible: more than 60 steps of launches have
 * been enqueued since the launch that gave up and are still unsettled, another pipeline has been started since, or a step begun
 * with emx_step_begin is open when the failure is noticed. */
int emx_persist_local_launches(emx_ctx* ctx, int64_t* n);
/* ... and how many took the CARRY form (tuning "persist_carry"): device-wide launches of stretch steps (two splits, even ndim <= 64, no
 * rows stored) over Philox plans whose split 0 is listed in the slot order emx_plan_arrange defines, so that a wave finds the walkers
 * it updated in the second half of a step in the same slots of the next step's first half and keeps their rows in registers */
int emx_persist_carry_launches(emx_ctx* ctx, int64_t* n);
/* host only: the lean stretch plan of `step` (two splits, even `nwalkers`) as the plan kernels write it for k_persist's CARRY form --
 * order, p0, s0, uacc: (nwalkers) entries, split 0 then split 1; keep_mask: one word per 16 slots of split 0, bit s & 15.  has_prev != 0:
 * split 0 is arranged after step - 1: slot s lists the walker of that step's split-1 slot s where it belongs to this step's split 0
 * (keep bit set), the other slots in ascending order list the walkers of this step's split 0 that were in split 0 before, in ascending
 * position.  has_prev == 0: position order, empty masks.  Split 1 is always in position order.  Every entry is the walker's own:
 * a listing order changes no draw.  -> 0, or -1 on a bad argument (odd or < 2 walkers, has_prev at step 0, a null pointer) */
int emx_plan_arrange(uint64_t seed, uint64_t step, int32_t has_prev, int64_t nwalkers, double a, int32_t* order, int32_t* p0, double* s0,
                     double* uacc, int32_t* keep_mask);
/* ... and how many of the CARRY launches found the partner-stable rows of their step boundaries prefetched (tuning "persist_partner_prefetch") */
int emx_persist_pprefetch_launches(emx_ctx* ctx, int64_t* n);
/* host only: the partner-stable masks of the plan emx_plan_arrange(seed, step, 1, ...) gives, as the plan kernels write them behind its
 * keep masks: one word per 16 slots of split 0, bit s & 15 set when slot s's partner p0[s] was in split 0 of step - 1 -- a row nobody
 * writes during that step's second half.  -> 0, or -1 on a bad argument (odd or < 2 walkers, step 0, a null pointer) */
int emx_plan_partner_stable(uint64_t seed, uint64_t step, int64_t nwalkers, double a, int32_t* stable_mask);
/* host only: the grid the persistent kernel takes for `nwalkers` walkers updated in `nsplits` half-steps on a device of `num_cu`
 * CUs -- waves per workgroup (8 / 4 / 2 / 1; 0: no persistent grid, the per-half-step launches run) and workgroups */
int emx_host_persist_shape(int64_t nwalkers, int32_t nsplits, int32_t num_cu, int32_t* waves_per_group, int32_t* groups);

/* ---- host-only helpers (no GPU needed; used by the CPU test-suite) ---------------------- */
typedef struct emx_mt emx_mt;
emx_mt* emx_mt_create(const uint32_t key[624], int32_t pos, int32_t has_gauss, double cached);
void emx_mt_destroy(emx_mt* m);
void emx_mt_get_state(const emx_mt* m, uint32_t key[624], int32_t* pos, int32_t* has_gauss, double* cached);
void emx_mt_random_sample(emx_mt* m, int64_t n, double* out);
void emx_mt_randint(emx_mt* m, uint64_t bound, int64_t n, int64_t* out);
void emx_mt_randn(emx_mt* m, int64_t n, double* out);
void emx_mt_shuffle_labels(emx_mt* m, int64_t n, int32_t nsplits, int32_t* labels);
int32_t emx_mt_choice_cdf(emx_mt* m, const double* cdf, int32_t n);
/* one step's exact plan on the host (the producer emx_run uses in MT19937 mode) */
int emx_host_plan_mt(emx_mt* m, int64_t nwalkers, int32_t ndim, const emx_move_desc* mv, int32_t* off, int32_t* order,
                     int32_t* p0, int32_t* p1, int32_t* p2, double* s0, double* uacc);
/* The same plans for `nsteps` consecutive steps (move choice included, ensemble.py:406) made by the threaded pipeline emx_run
 * uses in MT19937 mode (csrc/emx_mtpipe.hpp: generator / tokenizer / `nworkers` finisher threads, `nsinks` staging buffers used
 * round-robin).  Output arrays hold nsteps * nwalkers entries (step-major; any may be NULL), moves_out nsteps.  Advances `m`
 * exactly like nsteps calls of emx_mt_choice_cdf + emx_host_plan_mt.  Returns the number of finisher threads used (> 0) or a
 * negative code; *seconds_out: wall time of the whole production. */
int emx_host_plan_mt_stream(emx_mt* m, int64_t nwalkers, int32_t ndim, int32_t nmoves, const emx_move_desc* moves,
                            const double* cdf, int64_t nsteps, int32_t nworkers, int32_t nsinks, int32_t* moves_out,
                            int32_t* order, int32_t* p0, int32_t* p1, int32_t* p2, double* s0, double* uacc,
                            double* seconds_out);
/* the draws of ONE RedBlueMove.get_proposal(s, c, random) call for `split` of a given partition */
int emx_host_split_draws(emx_mt* m, int64_t nwalkers, const emx_move_desc* mv, const int32_t* off,
                         const int32_t* order, int32_t split, int32_t* p0, int32_t* p1, int32_t* p2, double* s0);
/* one step's native plan on the host (the function the kernels evaluate in flight) */
int emx_host_plan_philox(uint64_t seed, uint64_t step, int64_t nwalkers, const emx_move_desc* mv, int32_t* off,
                         int32_t* order, int32_t* p0, int32_t* p1, int32_t* p2, double* s0, double* uacc);
int32_t emx_host_move_choice_philox(uint64_t seed, uint64_t step, const double* cdf, int32_t n);
/* EMX_MOVE_WALK / EMX_MOVE_KDE in native mode: the draws of every slot of `split` (slot order of emx_host_plan_philox).
 * helpers: walk s >= 2 -> (ns, s) helper walkers in draw order, KDE -> (ns) kernel centres, walk s == 0 -> unused (may be NULL);
 * normals: walk s >= 2 -> (ns, s), walk s == 0 and KDE -> (ns, ndim).  Returns ns, or -1 for bad arguments. */
int64_t emx_host_walk_kde_draws(uint64_t seed, uint64_t step, int64_t nwalkers, int32_t ndim, const emx_move_desc* mv, int32_t split,
                                int32_t* helpers, double* normals);
/* pull exchange: records per (source, destination) pair of one half-step (what emx_pull_prepare returns) */
int64_t emx_host_pull_capacity(int64_t nwalkers, int32_t world, int32_t nsplits, int32_t partners_per_walker);

/* ---- batches of independent small ensembles (emcee_amd.EnsembleBatch; csrc/emx_batch.hip) ----
 * B ensembles of one shape (nwalkers, ndim), each with its own state, Philox seed, target parameters, chain and status, run by
 * ONE launch of the one-workgroup kernel k_small_run per chunk of up to 4 096 steps: workgroup b runs member b exactly as an
 * emx_ctx in Philox mode runs that ensemble (same bits).  Shapes: small_kernel's rules per member (nwalkers <= 4 096, ndim <= 256,
 * the LDS bound, the dense contraction bound, <= 8 stretch / DE / snooker / Gaussian moves, DE with >= 2 walkers a complement);
 * fused device targets, the caller's batched log-prob (emx_set_batch_target_callback below) or the caller's device function compiled
 * into the kernel (emx_set_batch_target_fused below); not EMX_TARGET_HOST.  Arrays are
 * member-major: coordinates
 * (B, nwalkers, ndim), log-probs and accept counts (B, nwalkers), the chain (B, capacity, nwalkers, ndim).
 * Tuning keys (emx_batch_set_tuning; neither changes a bit, plans do not depend on the state):
 *   "batch_threads"      0 (auto)  threads of a member's workgroup (a multiple of 64, <= 1 024)
 *   "batch_plan_steps"   0 (auto)  steps whose plans one pass keeps in LDS (<= 64)
 *   auto: up to one member a CU, the single-ensemble shape (small_threads / small_batch); more members than CUs, one
 *   half-step's lanes and one plan entry a thread, so that several members share a CU.
 *   "batch_acf_series"   0 (auto)  emx_autocorr_batch: at most this many (member, walker, dim) series per FFT chunk (auto: the
 *                                  scratch within ~3 GB); a chunk may begin and end inside a member
 *   "batch_summary_members" 0 (auto) emx_summary_batch: at most this many members per pass (auto: the scratch within ~512 MB);
 *                                  every member is reduced on its own in an order fixed by its shape, so no bit depends on it
 *   "batch_rhat_members" 0 (auto)  emx_rhat_batch: at most this many members per pass (auto: the scratch within ~512 MB); every
 *                                  sum runs in an order fixed by the shape and the pooling, so no bit depends on it
 *   "batch_hist_members" 0 (auto)  emx_histograms_batch: at most this many members per chunk (auto: the chunk's one-byte bin-code
 *                                  plane, edges and counters within ~256 MB); every count is a sum of integers, so none depends on it
 *   "batch_hist_rows"    0 (auto)  emx_histograms_batch: selected rows of a member per chunk of the code plane (auto: all of them,
 *                                  unless ONE member's code plane exceeds ~256 MB); no count depends on it */
typedef struct emx_batch emx_batch;
/* host only (no device touched): 0 when the kernel takes the shape, else -1 and the reason in msg */
int emx_batch_check(int64_t nwalkers, int32_t ndim, int32_t target, int32_t nmoves, const emx_move_desc* moves, char* msg,
                    int32_t msglen);
int emx_batch_create(int32_t device, int32_t nbatch, int64_t nwalkers, int32_t ndim, emx_batch** out);
int emx_batch_destroy(emx_batch* b);
const char* emx_batch_last_error(emx_batch* b);
int emx_batch_set_tuning(emx_batch* b, const char* key, int64_t value);
/* per_member 0: one target for every member (p0 / p1 as emx_set_target, scales[0]); 1: B of them, member-major
 * (p0 (B, ndim); p1 (B, ndim) ivar or (B, ndim, ndim) icov; scales (B) Rosenbrock scales, 0 or NULL: 20) */
int emx_batch_set_target(emx_batch* b, int32_t kind, const double* p0, const double* p1, const double* scales, int32_t per_member);
/* The caller's own batched log-prob over every member at once (EMX_TARGET_DEVICE_CALLBACK of a batch; emcee_amd.targets.BatchCallable /
 * BatchKernel): the rules of emx_device_log_prob_fn -- called on the host thread that drives the run, it must ENQUEUE work on
 * `hip_stream` that reads coords_dev (nbatch, rows, ndim) and writes log_prob_dev (nbatch, rows), return 0 (non-zero aborts the run
 * with an error) and never synchronise; -inf is legal, NaN raises the reference's error naming the member.  Each row must be
 * computed independently of the others and of the block's shape.  A proposal step is S_max calls (S_max, S_min: the largest and
 * smallest nsplits of the schedule, 1 for a GaussianMove), each on rows = ceil(nwalkers / S_min): at phase k, rows [0, n) of
 * member b are its split k's proposals in the order the single-ensemble callback receives them (n that split's size), the
 * other rows padding -- copies of the member's current walkers, whose results are ignored (NaN included).  The initial
 * log-probs (emx_batch_eval_state_log_prob) are one call on the state itself, rows = nwalkers.  Per run of n proposal steps:
 * n S_max + 1 launches of the library's k_batch_cb (one workgroup a member: commit the previous phase, propose the next) and n S_max
 * calls, whatever B.  A GaussianMove runs only as the one move of such a schedule.  Replaces the fused target; "batch_threads"
 * applies (auto: one phase's rows in one pass), "batch_plan_steps" does not. */
typedef int (*emx_batch_log_prob_fn)(void* user, const double* coords_dev, int32_t nbatch, int64_t rows, int32_t ndim,
                                     double* log_prob_dev, void* hip_stream);
int emx_set_batch_target_callback(emx_batch* b, emx_batch_log_prob_fn fn, void* user);
/* Fused user targets (EMX_TARGET_FUSED_USER; emcee_amd.targets.BatchFused / compile_fused): the caller's per-row __device__
 * log-probability compiled INTO k_small_run, so that the batch runs as it does for a built-in target -- one launch per chunk of up
 * to 4 096 steps, no callback, no proposal block in global memory.  The caller's translation unit includes
 * emcee_amd/csrc/emx_fused_target.hpp and emits a launcher with EMX_FUSED_BATCH_TARGET(name, Functor, ndim); the library fills the
 * descriptor below and calls the launcher where it launches its own instantiations.  `args` is the library's internal SmallRunArgs:
 * `abi` (EMX_FUSED_ABI of that header, bumped with any change of the struct or of the kernel's LDS layout) and `args_bytes`
 * (its sizeof) are checked by the launcher against the values it was compiled with, so a launcher built against another version
 * of the header is refused, never run.  grid == 0 is a probe: check abi, args_bytes and ndim, launch nothing.  Returns 0, or
 * non-zero and nothing launched (1: another version of the header, 2: another ndim, 3: the move selector was not compiled in,
 * 4: another number of blobs, 100 + a hipError_t: the launch failed).  emx_set_batch_target_fused probes once, so a mismatch surfaces at bind time (-8 and
 * "built against another version of emx_fused_target.hpp").  `user_dev`: a device pointer handed to the functor with every row
 * (per-member data, indexed by the functor's `member`); the caller keeps it alive.  The one-workgroup rules apply with the
 * staging area's LDS on top (emx_batch_check with EMX_TARGET_FUSED_USER); "batch_threads" and "batch_plan_steps" apply and
 * change no bit.  Not a target of tempered batches (emx_pt_set_tempering refuses it: this launcher carries k_small_run; the
 * tempered kernel has its own launcher type, emx_pt_set_target_fused below). */
typedef struct emx_fused_launch {
    uint32_t abi;            /* EMX_FUSED_ABI the library was built with */
    uint32_t args_bytes;     /* sizeof(SmallRunArgs) of the library */
    int32_t ndim, movesel, grid, threads;      /* movesel: EMX_MOVE_STRETCH (the schedule is one StretchMove) or 7 (any schedule) */
    uint64_t lds_bytes;      /* dynamic LDS of a workgroup (> 48 KB: the launcher raises the function's limit) */
    void* hip_stream;
    const void* args;        /* SmallRunArgs */
    const void* user;        /* user_dev */
    int32_t nblobs;          /* blobs a sample of the handle's target (0: none); the launcher answers 4 when it was compiled for another count */
    int32_t reserved;        /* batches: 0.  emx_set_target_fused_small: 1 when args carries the host's plans (exact MT19937 mode) */
} emx_fused_launch;
typedef int (*emx_fused_batch_fn)(const emx_fused_launch*);     /* 0, or non-zero and nothing launched */
int emx_set_batch_target_fused(emx_batch* b, emx_fused_batch_fn fn, int32_t ndim_compiled, const void* user_dev);
/* ---- blobs of a batch: derived quantities recorded with every sample (the reference's log_prob_fn returning (lp, blobs...);
 * emcee_amd.EnsembleBatch.get_blobs) ----
 * A batch target may produce nblobs (1 ... 32) doubles with every log-probability, by the same call.  The handle keeps each
 * walker's current blobs (B, nwalkers, nblobs) and a blob plane (B, capacity, nwalkers, nblobs) next to the chain.  A proposal's
 * blobs replace the walker's exactly when its log-probability does (moves/move.py:29-45): a rejected proposal, and a row rejected
 * without reaching the target (a non-finite coordinate, a -inf factor), keep the previous ones.  Values are not validated (NaN is
 * legal).  emx_batch_eval_state_log_prob fills the blobs of the state, emx_batch_chain_read reads the plane (what 4) and
 * emx_summary_batch_plane summarises it.  Coordinates, log-probs and accept counts are bit for bit those of the same function
 * without blobs.  The built-in targets have none.  Set before the first stored step.  A tempered handle carries them too (a
 * callback handle takes emx_set_batch_target_callback_blobs once it is tempered; emx_pt_set_tempering refuses a callback handle
 * that already has blobs): see "blobs of a tempered handle" below.
 *
 * emx_set_batch_target_fused_blobs: emx_set_batch_target_fused for a launcher emitted by EMX_FUSED_BATCH_TARGET_BLOBS(name,
 * Functor, ndim, nblobs) -- the functor's five-argument form (..., double* blobs).  The walkers' blobs live in LDS behind the
 * staging area (nwalkers nblobs doubles on top of emx_batch_check's bound: emx_check_batch_blobs).  The probe hands the count to
 * the launcher, which answers 4 when it was compiled for another one (-1 and "another number of blobs" at bind time);
 * nblobs 0 is emx_set_batch_target_fused.
 *
 * emx_set_batch_target_callback_blobs: emx_set_batch_target_callback for a function that also writes blobs_dev, a (nbatch, rows,
 * nblobs) block, row for row with log_prob_dev (padding rows' blobs are ignored like their log-probs).
 *
 * (emx_check_batch_blobs and emx_get_blobs_batch are named like emx_summary_batch: the emx_batch_ prefix is the handle's closed
 * set of entry points.) */
int emx_set_batch_target_fused_blobs(emx_batch* b, emx_fused_batch_fn fn, int32_t ndim_compiled, const void* user_dev, int32_t nblobs);
typedef int (*emx_batch_log_prob_blobs_fn)(void* user, const double* coords_dev, int32_t nbatch, int64_t rows, int32_t ndim,
                                           double* log_prob_dev, int32_t nblobs, double* blobs_dev, void* hip_stream);
int emx_set_batch_target_callback_blobs(emx_batch* b, emx_batch_log_prob_blobs_fn fn, void* user, int32_t nblobs);
/* Fused user targets of a batch whose log-probability SUMS OVER PER-MEMBER DATA (emcee_amd.targets.BatchFused(..., ndata=) /
 * compile_fused(..., data=True)): base(theta) + sum_k term(theta; datum k), k in [0, ndata[member]).  The caller's translation unit
 * includes emcee_amd/csrc/emx_fused_target_data.hpp and emits the launcher with EMX_FUSED_BATCH_DATA_TARGET(name, Model, ndim)
 * around a model with `base` and `term` members; k_small_run then gives every staged row a WAVE for the data sum -- and commits
 * it with all 64 lanes -- where the plain functor loops over the member's data in one lane.  The value of a row is defined in that
 * header (the lane-strided partial sums and the pairwise tree; emcee_amd.targets.fused_data_sum on the host) and depends on
 * neither the launch shape nor the size of the batch.  The descriptor is one of its own: the fields of emx_fused_launch, then
 * `ndata`, the library's member-indexed DEVICE array of the counts.  `abi` is EMX_FUSED_BATCH_DATA_ABI, a constant of its own, so
 * a data launcher handed emx_fused_launch and an EMX_FUSED_BATCH_TARGET launcher handed this one answer 1; the other answers are
 * emx_fused_batch_fn's (4: nblobs is not 0).  emx_set_batch_target_fused_data copies `ndata_host` (nbatch values, each in
 * [0, 2^31)) to the device, probes once and refuses another header version or ndim, a count out of range and a tempered handle
 * with emx_set_batch_target_fused's codes; it frees blob storage.  When members share CUs the workgroup is cut to a wave a row of
 * the largest split (not to its G lanes a row); "batch_threads" and "batch_plan_steps" apply and change no bit. */
typedef struct emx_fused_batch_data_launch {
    uint32_t abi;            /* EMX_FUSED_BATCH_DATA_ABI the library was built with */
    uint32_t args_bytes;     /* sizeof(SmallRunArgs) of the library */
    int32_t ndim, movesel, grid, threads;
    uint64_t lds_bytes;
    void* hip_stream;
    const void* args;        /* SmallRunArgs */
    const void* user;        /* user_dev */
    int32_t nblobs;          /* 0 */
    int32_t reserved;        /* 0 */
    const int64_t* ndata;    /* device: the data of every member, `grid` values */
} emx_fused_batch_data_launch;
typedef int (*emx_fused_batch_data_fn)(const emx_fused_batch_data_launch*);     /* 0, or non-zero and nothing launched */
int emx_set_batch_target_fused_data(emx_batch* b, emx_fused_batch_data_fn fn, int32_t ndim_compiled, const void* user_dev,
                                    const int64_t* ndata_host);
/* emx_batch_check for a target with nblobs blobs a sample (host only): 0, or -1 and the reason in msg */
int emx_check_batch_blobs(int64_t nwalkers, int32_t ndim, int32_t target, int32_t nmoves, const emx_move_desc* moves, int32_t nblobs,
                          char* msg, int32_t msglen);
/* the current state's blobs -> out (B, nwalkers, nblobs); -1 when the target has none; *nblobs_out (may be NULL): the count */
int emx_get_blobs_batch(emx_batch* b, double* out, int32_t* nblobs_out);
/* the move schedule (as emx_set_moves); a sequential GaussianMove only as the one move */
int emx_batch_set_moves(emx_batch* b, int32_t nmoves, const emx_move_desc* moves, const double* cdf);
int emx_batch_set_move_scale(emx_batch* b, int32_t move, const double* scale, int32_t n);
int emx_batch_get_move(emx_batch* b, int32_t move, emx_move_desc* out);
/* seeds[B]: member b draws exactly as an emx_ctx with emx_rng_set_philox(seeds[b], step) */
int emx_batch_set_philox(emx_batch* b, const uint64_t* seeds, uint64_t step);
int emx_batch_get_philox(emx_batch* b, uint64_t* seeds, uint64_t* step);
int emx_batch_set_state(emx_batch* b, const double* coords, const double* log_prob);     /* log_prob may be NULL */
int emx_batch_get_state(emx_batch* b, double* coords, double* log_prob);                 /* either may be NULL */
/* every member's log-probs of its coordinates in one launch, with emx_eval_state_log_prob's arithmetic (a batched callback: one
 * call and one NaN-check launch); a target with blobs fills the state's blobs by the same call */
int emx_batch_eval_state_log_prob(emx_batch* b);
/* capacity: stored steps a member can hold; growing keeps what is stored */
int emx_batch_chain_config(emx_batch* b, int64_t capacity);
int emx_batch_run(emx_batch* b, int64_t nsteps, int32_t thin_by, int32_t store);
int emx_batch_iteration(emx_batch* b, int64_t* stored, int64_t* proposals);
/* rows start, start + stride, ... < stop of members [member_lo, member_hi): what 0 -> (members, rows, nwalkers, ndim), 1 -> log-probs;
 * tempered handles also 2 -> log-likelihoods (members, rows, nwalkers) and 3 -> betas (members, rows); a target with blobs also
 * 4 -> the blob plane (members, rows, nwalkers, nblobs) */
int emx_batch_chain_read(emx_batch* b, int32_t what, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop,
                         int64_t stride, double* out);
/* Integrated autocorrelation time of members [member_lo, member_hi) per parameter (autocorr.py:20-123 on
 * backend.get_value("chain", discard, thin)), computed next to the chain as emx_autocorr does for one ensemble: tau_out
 * (members, ndim) in units of the selected samples, window_out (members, ndim) the Sokal windows (may be NULL), *nsamples_out
 * the series length nt, against which the caller applies the reference's "tol" rule.  Sokal's window runs on the device too:
 * only the (members, ndim) results cross to the host.  hipFFT plans and scratch stay on the handle between calls (new plans
 * when 2 next_pow_two(nt) changes); libhipfft as emx_autocorr (emx_fft_load), -5 when it cannot be loaded. */
int emx_autocorr_batch(emx_batch* b, int32_t member_lo, int32_t member_hi, int64_t discard, int64_t thin, double c,
                       double* tau_out, int32_t* window_out, int64_t* nsamples_out);
/* Posterior summaries of members [member_lo, member_hi) over rows start, start + stride, ... < stop of each
 * (emx_batch_chain_read's selection) and every walker, n = rows * nwalkers samples a member, computed next to the chain
 * (csrc/emx_batch_summary.hip): only O(members ndim^2) numbers cross to the host.  Any output may be NULL.
 *   mean_out (members, ndim); cov_out (members, ndim, ndim) the ddof = 1 covariance, exactly symmetric (NaN for n = 1);
 *   ranks (nranks <= 32, each in [0, n)): order_out (members, nranks, ndim) holds the ranks[r]-th smallest stored value of every
 *   parameter (0-based; exactly a stored value; of -0.0 and +0.0, which sort apart here and compare equal, either);
 *   map_coords_out (members, ndim), map_log_prob_out (members): the sample of the largest stored log-prob, the first in
 *   (row, walker) order (-inf is a value like any other); *nsamples_out = n.
 * Sums run in an order fixed by (rows, nwalkers, ndim) alone and the selection counts integers: the results do not depend on
 * the member range or on "batch_summary_members".  Scratch stays on the handle.  -1 for bad arguments, -2 for a device failure.
 * (Named like emx_autocorr_batch: the emx_batch_ prefix is the handle's own closed set of entry points, which
 * tests/test_batch_cpu.py pins.) */
int emx_summary_batch(emx_batch* b, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop, int64_t stride,
                      double* mean_out, double* cov_out, int32_t nranks, const int64_t* ranks, double* order_out,
                      double* map_coords_out, double* map_log_prob_out, int64_t* nsamples_out);
/* emx_summary_batch over one plane of the stored samples: plane 0 the coordinates (emx_summary_batch itself), plane 4 the blobs
 * (emx_batch_chain_read's `what`), the same (rows, nwalkers, width) layout with width nblobs in ndim's place: mean_out (members,
 * nblobs), cov_out (members, nblobs, nblobs), order_out (members, nranks, nblobs), map_coords_out (members, nblobs) the blobs
 * of the sample of the largest stored log-prob.  The same kernels and the same fixed summation order.  -1 for plane 4 of a
 * handle without blobs. */
int emx_summary_batch_plane(emx_batch* b, int32_t plane, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop,
                            int64_t stride, double* mean_out, double* cov_out, int32_t nranks, const int64_t* ranks,
                            double* order_out, double* map_coords_out, double* map_log_prob_out, int64_t* nsamples_out);
/* Histograms of members [member_lo, member_hi) of the batch over emx_summary_batch's selection of rows (plane 0: coordinates,
 * W = ndim; 4: blobs, W = nblobs -- emx_batch_chain_read's numbering), counted next to the member-major chain
 * (csrc/emx_batch_hist.hpp): what emx_chain_minmax / emx_histograms return for one ensemble, for every member at once.  One launch
 * grid covers every member of a chunk, so the number of launches does not grow with the number of members.  The rule is
 * emx_histograms': v falls in bin b iff e[b] <= v < e[b + 1], the last bin closed on the right; NaN, +-inf beyond the edges and
 * everything outside are counted nowhere.
 * emx_chain_minmax_batch: per (member, column) the smallest and the largest FINITE value (+inf / -inf where there is none) and
 * the number of non-finite ones: lo_out, hi_out, nonfinite_out, each (members, W).  Exact, whatever the order of the reduction.
 * emx_histograms_batch: the offsets edge_off / pedge_off (W + 1 entries, as emx_histograms': 1 ... 1024 marginal and 1 ... 128
 * pair bins a column), the pairs and pair_off are common to all members; the edge VALUES are per member: member m of the range
 * reads edges + m edge_member_stride (pedges + m pedge_member_stride), strictly increasing; stride 0: one set shared by all
 * members, else at least edge_off[W] (pedge_off[W]).  counts_out (members, edge_off[W] - W): member m's column d at
 * [m][edge_off[d] - d ...); pair_counts_out (members, pair_off[npairs]): member m's panel p, pb_i x pb_j counts with column i the
 * slow axis, at [m][pair_off[p] ...).  *nsamples_out: rows x nwalkers, of every member.  Each member's chain is read once whatever
 * the number of pairs (a one-byte bin code per value in a dim-major plane per member, from which the panels are counted); members
 * go in chunks (tuning "batch_hist_members"), and the rows of a member whose code plane alone exceeds the budget too
 * ("batch_hist_rows").  Every count is a sum of integers: no count depends on the launch shape, the chunking, the member range or
 * the order of the atomics.  Tempered handles: members are nbatch x ntemps.  Scratch stays on the handle.  -1 for bad arguments
 * (plane 4 of a handle without blobs, an empty selection, a member range outside the batch, edges that do not increase), -2 for
 * a device failure.  (Named like emx_summary_batch: the emx_batch_ prefix is the handle's own closed set.)
 * emx_histograms_batch_info: *launches_out the kernel launches of the handle's last emx_histograms_batch call. */
int emx_chain_minmax_batch(emx_batch* b, int32_t plane, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop,
                           int64_t stride, double* lo_out, double* hi_out, int64_t* nonfinite_out);
int emx_histograms_batch(emx_batch* b, int32_t plane, int32_t member_lo, int32_t member_hi, int64_t start, int64_t stop,
                         int64_t stride, const int64_t* edge_off, const double* edges, int64_t edge_member_stride,
                         int64_t* counts_out, const int64_t* pedge_off, const double* pedges, int64_t pedge_member_stride,
                         int64_t npairs, const int32_t* pairs, const int64_t* pair_off, int64_t* pair_counts_out,
                         int64_t* nsamples_out);
int emx_histograms_batch_info(emx_batch* b, int64_t* launches_out);
/* Split-R-hat (Gelman-Rubin, BDA3 section 11.4) of members [member_lo, member_hi) over emx_summary_batch's selection of rows,
 * computed next to the member-major chain (csrc/emx_rhat.hip, which states the definition): with nt selected rows and
 * h = nt / 2 (integer), every series (one walker's values of one parameter) is split into its first h and its last h selected
 * samples (the middle one is dropped when nt is odd): the "chains", each with its mean mu_c and ddof = 1 variance s_c^2.  A
 * group of C chains gives  within = mean_c s_c^2  and  between = var_c(mu_c, ddof = 1);  the caller forms
 * rhat = sqrt((h - 1) / h + between / within).
 *   pool 0: every member is its own group (C = 2 nwalkers), groups = members;
 *   pool P > 0: the members with equal (m - member_lo) mod P are pooled into P groups (C = 2 nwalkers members / P); the number
 *   of members must be a multiple of P.  A batch of replicates passes 1, a tempered handle its ntemps (one group a rung).
 * within_out, between_out: (groups, W), W = ndim + (log_prob != 0); with log_prob the last column holds the same statistic of
 * the stored log-prob series.  *nchains_out = C, *length_out = h (either may be NULL).  A constant group gives 0 and 0, a
 * non-finite sample NaN in its group and column.  -1 for bad arguments (nt < 4 among them), -2 for a device failure.  Scratch
 * stays on the handle.  No floating-point atomics; every sum runs in an order fixed by (nt, nwalkers,
 * ndim, pool): slices of a half in order, then the two halves of a walker, walkers in order, members in order.  No bit depends
 * on the member range (pool 0), on "batch_rhat_members" (0: auto, at most this many members per pass) or on the launch shape.
 * (Named like emx_summary_batch: the emx_batch_ prefix is the handle's own closed set.) */
int emx_rhat_batch(emx_batch* b, int32_t member_lo, int32_t member_hi, int32_t pool, int64_t start, int64_t stop, int64_t stride,
                   int32_t log_prob, double* within_out, double* between_out, int64_t* nchains_out, int64_t* length_out);
/* host twin of the selection (no device): the ranks[r]-th smallest of x[0], x[stride], ..., n values, with the same key
 * transform and digit search as the kernels.  0, or -1 for bad arguments (n < 1, stride < 1, nranks outside [0, 32], a rank
 * outside [0, n)). */
int emx_host_order_stats(const double* x, int64_t n, int64_t stride, int32_t nranks, const int64_t* ranks, double* out);
int emx_batch_accepted_counts(emx_batch* b, double* out);           /* (B, nwalkers) */
/* bits[B]: each member's status (emx_status's bits), read and cleared */
int emx_batch_status(emx_batch* b, uint32_t* bits);
/* the last launch's shape and the launches so far */
int emx_batch_launch_info(emx_batch* b, int32_t* threads, int32_t* plan_steps, int64_t* launches);

/* ---- parallel tempering on a batch handle (emcee_amd.PTSampler; csrc/emx_pt.hip) ----
 * The members of a batched-callback handle grouped in runs of ntemps: member m = g ntemps + t is rung t (beta_t) of group g, so a
 * batched callback sees its nbatch = groups x ntemps members in (object, rung) order.  Each rung samples the tempered
 *   lp = beta L + P    (two IEEE operations, no contraction; lp = P at beta 0, so that 0 x -inf never occurs; lp = -inf where P is)
 * with L the callback's untempered log-likelihood and P the prior: none (0, improper), the box [box_lo, box_hi] evaluated by the
 * library (0 inside, bounds included, -inf outside), or the caller's prior callback, called on the same block before L.  Where P
 * is -inf the row's L is ignored (NaN included) and kept as -inf.  The commit is k_batch_cb's Metropolis rule on the tempered lp;
 * lp, L and P are kept per walker.  A NaN L where P > -inf (or a NaN lp) raises ST_NAN_LOGP in the member's status.
 *
 * Swap pass, after every swap_every-th proposal step (Philox step s with (s + 1) % swap_every == 0; 0: never), ptemcee's order:
 * pairs i = ntemps - 1 ... 1, walker k of rung i against walker pi_i(k) of rung i - 1, accepted when
 *   (beta_{i-1} - beta_i) (L_i[k] - L_{i-1}[pi_i(k)]) > log u_{i,k}          (IEEE: -inf - -inf is NaN, and NaN is rejected)
 * An accepted swap exchanges x, L and P and recomputes lp at both destinations; each pair sees the result of the one before.
 * Draws (emx_host_pt_swap_draws is their host twin): keyed by the group's rung-0 Philox seed and the step just taken, pi_i is
 * a keyed bijection of [0, nwalkers) (the split permutation's construction under the tag 'SWPM', counter 2 (i - 1)), u_{i,k} is u53
 * of the Philox words (step lo, step hi, 'SWAP', (i - 1) nwalkers + k), log u the plan logarithm (host and device bits agree).
 * A step with a swap pass is S_max + 2 launches (the phases, a commit-only launch, k_pt_swap), else S_max; S_max calls of the
 * likelihood a step (and S_max of a prior callback).  Stored rows hold the state after the step's swap pass (ptemcee's rule):
 * coordinates, tempered lp (what 1), L (emx_batch_chain_read what 2) and each member's beta (what 3, one value a row).
 * Accept counts stay per member; swap attempts and accepts are counted per (group, pair i - 1). */
/* ntemps must divide the batch; betas (ntemps) non-increasing (PTSampler asks strictly decreasing), betas[0] == 1, betas[ntemps-1] >= 0; box_lo / box_hi (ndim)
 * or both NULL.  Before anything is stored. */
int emx_pt_set_tempering(emx_batch* b, int32_t ntemps, const double* betas, const double* box_lo, const double* box_hi);
/* the caller's batched log-prior (the emx_batch_log_prob_fn contract), in place of a box; NULL removes it */
int emx_set_batch_prior_callback(emx_batch* b, emx_batch_log_prob_fn fn, void* user);
int emx_pt_set_swap_every(emx_batch* b, int64_t n);                 /* default 1 */
/* one swap pass on the current state with the draws of the last step taken (step - 1); writes no chain row */
int emx_pt_swap(emx_batch* b);
/* attempts / accepts (groups, ntemps - 1) */
int emx_pt_swap_counts(emx_batch* b, uint64_t* attempts, uint64_t* accepts);
/* out (B): the mean of each member's L chain over rows start, start + stride, ... < stop and every walker, on the device */
int emx_pt_mean_loglike(emx_batch* b, int64_t start, int64_t stop, int64_t stride, double* out);
/* The per-block sums behind PTSampler.get_evidence (csrc/emx_pt_evidence.hip, which states the definition) of objects
 * [g_lo, g_hi) over the stored rows start, start + stride, ... < stop (nt of them): with K = nblocks and bl = nt / K, the last K bl
 * selected rows are cut into K consecutive blocks of n = bl nwalkers samples a rung.  sum_L (objects, T, K): the sum of L over
 * block k of rung t.  amax / sexp (objects, T - 1, K): for pair j of rungs j and j + 1, with d = b[j] - b[j + 1] and a = d L over
 * the samples of rung j + 1, M = max a and S = sum exp(a - M) (L = -inf: no weight; a block of nothing else: M = -inf, S = 0; a NaN
 * sample: S NaN).  betas (objects, T): the stored ladder of the first used row; ladder_changed (objects): 1 where some used row's
 * ladder differs from it in any bit.  *block_rows = bl (may be NULL).  The caller merges the blocks (the stepping-stone and the
 * thermodynamic-integration evidence and their Monte-Carlo errors).  The L plane is read once; no floating-point atomics; every
 * sum and every (M, S) merge runs in an order fixed by (nt, nblocks, nwalkers, stride): no bit depends on the object range or the
 * launch shape.  -1 for bad arguments (an untempered handle, no stored chain, rows outside the stored ones, nblocks outside
 * [1, nt]), -2 for a device failure. */
int emx_pt_evidence(emx_batch* b, int64_t g_lo, int64_t g_hi, int64_t start, int64_t stop, int64_t stride, int32_t nblocks,
                    double* sum_L, double* amax, double* sexp, double* betas, int32_t* ladder_changed, int64_t* block_rows);
/* the tempered state: coords (B, nwalkers, ndim), L and P (B, nwalkers); set computes lp with the formula above and each member's
 * current beta */
int emx_pt_set_state(emx_batch* b, const double* coords, const double* loglike, const double* logprior);
int emx_pt_get_state(emx_batch* b, double* loglike, double* logprior);
/* ---- blobs of a tempered handle (emcee_amd.PTSampler.get_blobs) ----
 * A likelihood with nblobs = K (emx_set_batch_target_callback_blobs AFTER emx_pt_set_tempering, in place of the callback the handle
 * was tempered with; or emx_pt_set_target_fused_blobs, which like emx_pt_set_target_fused comes before it) produces K doubles with
 * every untempered L; the prior produces none.  A walker's blobs are replaced exactly when its proposal is accepted by the tempered
 * commit.  An accepted swap exchanges them together with x, L and P: a blob belongs to the point, not to the rung (a blob that
 * records `member` names the rung where the point was last evaluated).  Where P is -inf the row's L is ignored and kept as -inf; its
 * blobs are likewise ignored and stored as NaN (the fused form never calls the likelihood there, the callback path calls it and
 * discards the result); such a row can only be an initial-state walker.  Stored rows are the blobs after the step's swap pass; the
 * ladder update does not touch them.  Coordinates, lp, L, P, accept and swap counts, ladders and the Philox step are bit for bit
 * those of the same function without blobs.  The plane is emx_batch_chain_read's what 4 and plane 4 of emx_summary_batch_plane,
 * emx_histograms_batch and emx_chain_minmax_batch, as on an untempered handle (L stays what 2); emx_get_blobs_batch reads the
 * current state's.
 * emx_pt_get_blobs: the current state's blobs -> out (B, nwalkers, nblobs), next to emx_pt_get_state; -1 for an untempered handle
 * or one without blobs.  emx_pt_set_state keeps its signature and sets the blobs of a handle that has them to NaN: it bypasses the
 * likelihood, so there is nothing they could hold. */
int emx_pt_get_blobs(emx_batch* b, double* out);
/* the swap draws of every pair after Philox step `step` under `seed`: perm_out / logu_out (ntemps - 1, nwalkers), row i - 1 for
 * pair i: pi_i(k) and log u_{i,k}.  0, or -1 for bad arguments. */
int emx_host_pt_swap_draws(uint64_t seed, uint64_t step, int64_t nwalkers, int32_t ntemps, int32_t* perm_out, double* logu_out);
/* The adaptive ladder (Vousden, Farr & Mandel 2016; ptemcee's adaptive=True).  When on, every swap pass ends, in k_pt_swap, with
 * an update of each group's ladder from that pass's accepted counts acc[i - 1] of pair i, after the handle's t-th earlier update:
 *   r[j] = acc[j] / nwalkers,  kappa = (lag / (t + lag)) / time,  dS[j] = kappa (r[j] - r[j + 1]),
 *   dT[j] = (1 / b[j + 1] - 1 / b[j]) exp(dS[j]),  c_j = dT[0] + ... + dT[j],  b'[j + 1] = 1 / (c_j + 1 / b[0])   (j = 0 ... T - 3)
 * in that order, in IEEE + - * / (exp too is made of them: host and device bits agree); rungs 0 and T - 1 stay, and with
 * ntemps <= 2 nothing moves but t still advances.  lp of the moved rungs is recomputed as beta' L + P (as everywhere else; ptemcee
 * adds L dbeta instead), and the new betas are stored as computed (ptemcee adds the difference).  Then the stored rows are
 * written: emx_batch_chain_read what 3 gives each stored row's beta, (B, rows).  ntemps <= 256 while adapting.
 * lag > 0 and time > 0, finite (ptemcee: 10000, 100); on 1 checks that every ladder has betas[0 ... ntemps - 2] > 0.  It may change
 * between runs; t is kept. */
int emx_pt_set_adaptation(emx_batch* b, int32_t on, double lag, double time);
/* betas (groups, ntemps): every group's current ladder; updates: the update counter t (either may be NULL) */
int emx_pt_get_ladder(emx_batch* b, double* betas, int64_t* updates);
/* set every group's ladder (each row checked as emx_pt_set_tempering checks its betas, and betas[0 ... ntemps - 2] > 0 while
 * adapting) and, unless NULL, the counter t; lp is recomputed on the device.  Allowed after rows have been stored. */
int emx_pt_set_ladder(emx_batch* b, const double* betas, const int64_t* updates);
/* the host twin of one group's update: out (ntemps) from betas (ntemps) and accepts (ntemps - 1) of a pass over nwalkers walkers
 * after t earlier updates.  0, or -1 for bad arguments. */
int emx_host_pt_adapt_ladder(const double* betas, const int64_t* accepts, int32_t ntemps, int64_t nwalkers, double lag, double time,
                             int64_t t, double* out);
/* Fused tempered targets (EMX_TARGET_FUSED_PT; emcee_amd.targets.PTFused / compile_fused_pt): the caller's per-row __device__
 * log-likelihood and, optionally, log-prior compiled INTO the tempered one-workgroup kernel k_pt_run.  One workgroup owns one object:
 * all its ntemps rungs live in LDS, every rung's half-step rows run side by side, the swap pass and the ladder update run on LDS
 * between workgroup barriers, and a run is ONE launch per chunk of up to 4 096 steps -- no callback, no proposal block, no k_pt_swap
 * launch.  Bit for bit the tempered callback run of the same functions (while no proposal has a non-finite coordinate: such a row
 * is rejected here without reaching a functor).  The caller's translation unit includes emcee_amd/csrc/emx_pt_fused.hpp and emits a
 * launcher with EMX_FUSED_PT_TARGET(name, LikeFunctor, PriorFunctor, ndim) (emx::NoFusedPrior: no prior functor -- the handle's
 * box, or a flat prior); the functors' `member` is object * ntemps + rung.  The descriptor is emx_fused_launch's with the library's
 * PtRunArgs behind `args` and EMX_FUSED_PT_ABI in `abi`; the launcher's answers are emx_fused_batch_fn's (1: another version of
 * the header, 2: another ndim, 3: the move selector was not compiled in, 100 + a hipError_t), and it writes `has_prior` (grid == 0:
 * the probe, nothing launched).  emx_pt_set_target_fused probes once and makes the launcher the handle's likelihood;
 * emx_pt_set_tempering then accepts the handle (with box_lo / box_hi only when the launcher has no prior functor, and only when
 * emx_pt_fused_check takes the shape).  emx_set_batch_prior_callback does not apply.  "batch_threads" and "batch_plan_steps" apply
 * and change no bit.  Everything that reads the handle's state or chain (emx_pt_get_state, emx_pt_swap, emx_pt_get_ladder,
 * emx_pt_set_ladder, emx_pt_swap_counts, emx_batch_chain_read, ...) works unchanged. */
typedef struct emx_pt_fused_launch {
    uint32_t abi;            /* EMX_FUSED_PT_ABI the library was built with */
    uint32_t args_bytes;     /* sizeof(PtRunArgs) of the library */
    int32_t ndim, movesel, grid, threads;      /* grid: objects (workgroups); movesel as emx_fused_launch's */
    uint64_t lds_bytes;
    void* hip_stream;
    const void* args;        /* PtRunArgs */
    const void* user;        /* user_dev */
    int32_t has_prior;       /* out: 1 when the launcher carries a prior functor */
    int32_t nblobs;          /* blobs a sample of the handle's likelihood (0: none); the launcher answers 4 when it was compiled for another count */
} emx_pt_fused_launch;
typedef int (*emx_pt_fused_fn)(emx_pt_fused_launch*);     /* 0, or non-zero and nothing launched */
int emx_pt_set_target_fused(emx_batch* b, emx_pt_fused_fn fn, int32_t ndim_compiled, const void* user_dev);
/* The same for a launcher emitted by EMX_FUSED_PT_TARGET_BLOBS(name, LikeFunctor, PriorFunctor, ndim, nblobs) around the likelihood's
 * five-argument form (..., double* blobs): nblobs (1 ... 32) doubles a sample, kept in LDS with the walkers (ntemps nwalkers nblobs
 * doubles) and the staging rows (ntemps rows nblobs), behind everything a blob-free object holds: emx_pt_fused_check_blobs.  The
 * probe hands the count to the launcher in the descriptor's `nblobs`, which answers 4 when it was compiled for another one (-1 and
 * "another number of blobs" at bind time).  nblobs 0 is emx_pt_set_target_fused.  The DATA form carries no blobs. */
int emx_pt_set_target_fused_blobs(emx_batch* b, emx_pt_fused_fn fn, int32_t ndim_compiled, const void* user_dev, int32_t nblobs);
/* ... whose log-likelihood SUMS OVER AN OBJECT'S DATA (emcee_amd.targets.PTFused(..., ndata=) / compile_fused_pt(..., data=True)):
 * log L(x) = base(x) + sum_k term(x; datum k).  The caller's translation unit includes emcee_amd/csrc/emx_pt_fused_data.hpp and emits
 * the launcher with EMX_FUSED_PT_DATA_TARGET(name, Model, PriorFunctor, ndim) around a model with base(x, ndim, member, user) and
 * term(x, ndim, member, k, user) members (emx_set_batch_target_fused_data's contract; member = object * ntemps + rung); the prior is
 * emx_pt_set_target_fused's.  k_pt_run's second pass and the initial state then give every row a WAVE: lane 0 evaluates the prior and
 * base, 64 lanes stride over the member's data, a fixed pairwise tree adds the lane partials, lane 0 takes the tempered decision and
 * the wave commits the row.  The value of a row is defined by emx_fused_target_data.hpp ("THE VALUE";
 * emcee_amd.targets.fused_data_sum on the host) and depends on no launch shape; a row outside the prior does not reach the model.
 * The launcher type and the descriptor are emx_pt_set_target_fused's with EMX_FUSED_PT_DATA_ABI in `abi` (a value of its own: a plain
 * launcher handed to this setter, and a data launcher handed to emx_pt_set_target_fused, are refused with -8) and the same answers.
 * `ndata_host` holds one count a member of the handle (nbatch values of emx_batch_create: object-major, every rung of an object
 * its object's count), each in [0, 2^31) -- else -1 and a message naming the member -- and is copied to the device.  Comes before
 * emx_pt_set_tempering; emx_pt_fused_check is unchanged (the data form needs no LDS of its own).  The default launch shape is a wave
 * a row of one half-step of all rungs (at most 512 threads); "batch_threads" and "batch_plan_steps" apply and change no bit. */
int emx_pt_set_target_fused_data(emx_batch* b, emx_pt_fused_fn fn, int32_t ndim_compiled, const void* user_dev,
                                 const int64_t* ndata_host);
/* host only (no device touched): 0 when one workgroup's LDS holds an object of ntemps rungs of (nwalkers, ndim) under this
 * schedule with at least one plan step, else -1 and the reason (with the bytes needed) in msg */
int emx_pt_fused_check(int32_t ntemps, int64_t nwalkers, int32_t ndim, int32_t nmoves, const emx_move_desc* moves, char* msg,
                       int32_t msglen);
/* emx_pt_fused_check for a likelihood with nblobs blobs a sample (nblobs 0: emx_pt_fused_check itself, the same answers and the
 * same text).  A shape that fits only without the blobs is refused with a message that names LDS and the "<nblobs> blobs". */
int emx_pt_fused_check_blobs(int32_t ntemps, int64_t nwalkers, int32_t ndim, int32_t nmoves, const emx_move_desc* moves, int32_t nblobs,
                             char* msg, int32_t msglen);

#ifdef __cplusplus
}
#endif
#endif /* EMX_H */
