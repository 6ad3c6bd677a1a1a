// Private glue between the translation units of libemx (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/emx.h"

struct EnsSummary;     // emx_summary's scratch (emx_batch_summary.hip), kept on the context between calls
struct RhatScratch;    // emx_rhat's / emx_rhat_batch's scratch (emx_rhat.hip), kept on the context / the batch handle between calls
void emx_internal_rhat_release(RhatScratch* s);      // implemented in emx_rhat.hip: frees it (emx_destroy, emx_batch_destroy)
struct PtEvidenceScratch;     // emx_pt_evidence's scratch (emx_pt_evidence.hip), kept on the batch handle between calls
void emx_internal_pt_evidence_release(PtEvidenceScratch* s);      // implemented in emx_pt_evidence.hip: frees it (emx_batch_destroy)
struct EmxChainView {
    double* chain;       // (stored, N, D) device-resident chain, or nullptr
    double* chain_lp;    // (stored, N)
    int64_t N;
    int32_t D;
    int64_t stored;
    hipStream_t stream;
    int device;
    double* chain_blobs; // (stored, N, nblobs) next to the chain, or nullptr
    int32_t nblobs;
    int64_t cap;         // rows the three planes have room for
    int64_t summary_compact;     // tuning "summary_compact"
    EnsSummary** summary;        // the context's slot (nullptr until the first call)
    int64_t hist_chunk_rows;     // tuning "hist_chunk_rows" (0: auto)
    RhatScratch** rhat;          // the context's slot (nullptr until the first call)
};

// implemented in emx.hip
int emx_internal_chain_view(emx_ctx* c, EmxChainView* v);
int emx_internal_state_view(emx_ctx* c, const double** X, int64_t* N, int32_t* D, int* device);      // settles and synchronises the context first
int emx_internal_fail(emx_ctx* c, int code, const char* msg);      // records the message for emx_last_error, returns code
int emx_internal_settle(emx_ctx* c);      // everything the context was asked to run is known to be done (or is done again): before a chain is read
// implemented in emx_batch_summary.hip: frees the scratch (emx_destroy)
void emx_internal_ens_summary_release(EnsSummary* s);

// ---- hipFFT, resolved at run time (PyTorch bundles its own copy; the process should hold one).  Implemented in emx_aux.hip;
// emx_autocorr and emx_autocorr_batch (emx_batch_acf.hip) share the one dlopen.
struct FftApi {
    void* h = nullptr;
    int (*PlanMany)(void**, int, int*, int*, int, int, int*, int, int, int, int) = nullptr;
    int (*SetStream)(void*, hipStream_t) = nullptr;
    int (*ExecD2Z)(void*, double*, void*) = nullptr;
    int (*ExecZ2D)(void*, void*, double*) = nullptr;
    int (*Destroy)(void*) = nullptr;
};
extern FftApi g_fft;
constexpr int FFT_D2Z = 0x6a, FFT_Z2D = 0x6c;
int fft_load(const char* path, std::string& err);      // 0, or -5 with the reason in err

// ---- the batch handle seen from emx_batch_acf.hip, emx_batch_summary.hip, emx_rhat.hip and emx_pt_evidence.hip (the handle itself lives in emx_batch.hip)
struct BatchAcf;     // emx_autocorr_batch's hipFFT plans and scratch, kept on the handle between calls
struct BatchSummary;     // emx_summary_batch's scratch (emx_batch_summary.hip), kept on the handle between calls
struct EmxBatchView {
    const double* chain;     // (B, cap, N, D) member-major, or nullptr
    const double* chain_lp;  // (B, cap, N)
    int32_t B, D;
    int64_t N, cap, stored;
    int64_t acf_series;      // tuning "batch_acf_series" (0: auto)
    hipStream_t stream;
    int device;
    BatchAcf** acf;          // the handle's slot (nullptr until the first call)
    int64_t summary_members; // tuning "batch_summary_members" (0: auto)
    BatchSummary** summary;  // the handle's slot (nullptr until the first call)
    const double* chain_blobs;   // (B, cap, N, nblobs) member-major, or nullptr
    int32_t nblobs;
    int64_t hist_members;    // tuning "batch_hist_members" (0: auto)
    int64_t hist_rows;       // tuning "batch_hist_rows" (0: auto)
    int64_t rhat_members;    // tuning "batch_rhat_members" (0: auto)
    RhatScratch** rhat;      // the handle's slot (nullptr until the first call)
    // a tempered handle (emx_pt_evidence.hip): rungs an object (0: untempered), the L plane (B, cap, N) and the beta plane (B, cap)
    int32_t pt_T;
    const double* chain_L;
    const double* chain_beta;
    PtEvidenceScratch** pt_evidence;     // the handle's slot (nullptr until the first call)
};
// implemented in emx_batch.hip
int emx_internal_batch_view(emx_batch* b, EmxBatchView* v);
int emx_internal_batch_fail(emx_batch* b, int code, const char* msg);      // records the message for emx_batch_last_error, returns code
// implemented in emx_batch_acf.hip: destroys the plans and frees the scratch (emx_batch_destroy)
void emx_internal_batch_acf_release(BatchAcf* a);
// implemented in emx_batch_summary.hip: frees the scratch (emx_batch_destroy)
void emx_internal_batch_summary_release(BatchSummary* s);
