// A USER's models for an EnsembleBatch, each defined ONCE as a __device__ inline function and wrapped twice:
//   * as a batched callback (a kernel + an emx_batch_log_prob_fn, the form of user_batch_logprob.hip; targets.BatchKernel), and
//   * as a functor compiled into the batch kernel (EMX_FUSED_BATCH_TARGET of emx_fused_target.hpp; targets.BatchFused).
// Test material (tests/test_gpu_batch_fused.py, tests/test_batch_fused_cpu.py compile it with hipcc -ffp-contract=off and
// -DUSER_NDIM=<ndim>); not part of the product.  The fused run must equal the callback run of the same function bit for bit.
//
// Model (a): member b's diagonal Gaussian -0.5 sum_d ivar[b, d] (x_d - mu[b, d])^2, accumulated over d in ascending order with a
// separate multiply and add (user_batch_logprob.hip's arithmetic).
// Model (b): a polynomial fit to K = 20 points a member, y_k ~ N(sum_{j < ndim - 1} x_j t_k^j, yerr_k^2 + exp(x_{ndim-1})) -- a
// straight line with a log-variance parameter at ndim 3 -- with a box prior: -inf unless every |x_d| <= 2.5.  It calls the
// device's exp and log and reads 60 values a member through `user`.
// Model (n): model (a), but NaN for member `nan_member` wherever x_0 > nan_above (USER_WITH_NAN; the single-StretchMove kernel only).
#include <emx_fused_target.hpp>

#include <stdint.h>

#ifndef USER_NDIM
#error "compile with -DUSER_NDIM=<ndim>"
#endif

#define USER_K 20

struct user_dev {             // device-resident; what the functors' `user` points at
    const double* mu;         // (nbatch, ndim)
    const double* ivar;       // (nbatch, ndim)
    const double* data;       // (nbatch, 3, USER_K): t, y, yerr
    int nan_member;           // -1: none
    double nan_above;
};

struct user_model {           // host side
    user_dev host;            // the device struct's image (device pointers)
    user_dev* dev;
    int nbatch, ndim;
};

__device__ inline double model_a(const double* x, int ndim, int member, const void* user) {
    const user_dev* u = (const user_dev*)user;
    const double* mu = u->mu + (long long)member * ndim;
    const double* ivar = u->ivar + (long long)member * ndim;
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) {
        const double r = x[d] - mu[d];
        acc = acc + ivar[d] * r * r;
    }
    return -0.5 * acc;
}

__device__ inline double model_b(const double* x, int ndim, int member, const void* user) {
    const user_dev* u = (const user_dev*)user;
    for (int d = 0; d < ndim; ++d)
        if (!(x[d] >= -2.5 && x[d] <= 2.5)) return -__builtin_inf();
    const double* t = u->data + (long long)member * 3 * USER_K;
    const double *y = t + USER_K, *yerr = y + USER_K;
    const double s2 = exp(x[ndim - 1]);
    double acc = 0.0;
    for (int k = 0; k < USER_K; ++k) {
        double m = 0.0;
        for (int j = ndim - 2; j >= 0; --j) m = m * t[k] + x[j];      // Horner
        const double var = yerr[k] * yerr[k] + s2;
        const double r = y[k] - m;
        acc = acc + (r * r / var + log(var));
    }
    return -0.5 * acc;
}

__device__ inline double model_n(const double* x, int ndim, int member, const void* user) {
    const user_dev* u = (const user_dev*)user;
    if (member == u->nan_member && x[0] > u->nan_above) return __builtin_nan("");
    return model_a(x, ndim, member, user);
}

// ---- the batched-callback form: one thread per (member, row) of the (nbatch, rows, ndim) block ----
template <int MODEL>
__global__ __launch_bounds__(256) void k_user_block(const double* __restrict__ q, int nbatch, long long rows, int D, const user_dev* u,
                                                    double* __restrict__ out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (long long)nbatch * rows) return;
    const int b = (int)(k / rows);
    const double* x = q + k * D;
    out[k] = MODEL == 0 ? model_a(x, D, b, u) : MODEL == 1 ? model_b(x, D, b, u) : model_n(x, D, b, u);
}

template <int MODEL>
static int user_block(void* user, const double* coords_dev, int32_t nbatch, int64_t rows, int32_t ndim, double* log_prob_dev, void* hip_stream) {
    user_model* m = (user_model*)user;
    if (ndim != m->ndim || nbatch != m->nbatch) return 1;
    const long long n = (long long)nbatch * rows;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_user_block<MODEL>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, coords_dev, (int)nbatch,
                       (long long)rows, (int)ndim, (const user_dev*)m->dev, log_prob_dev);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// ---- the fused form ----
struct ModelA {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return model_a(x, ndim, member, user); }
};
struct ModelB {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return model_b(x, ndim, member, user); }
};
struct ModelN {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return model_n(x, ndim, member, user); }
};

EMX_FUSED_BATCH_TARGET(user_fused_a, ModelA, USER_NDIM)
EMX_FUSED_BATCH_TARGET(user_fused_b, ModelB, USER_NDIM)
#ifdef USER_WITH_NAN
EMX_FUSED_BATCH_TARGET_MOVES(user_fused_n, ModelN, USER_NDIM, EMX_FUSED_MOVES_STRETCH)
#endif

extern "C" {

// emx_batch_log_prob_fn of the three models: enqueue on `hip_stream`, never synchronise
__attribute__((visibility("default"))) int user_block_a(void* user, const double* q, int32_t nbatch, int64_t rows, int32_t ndim, double* out, void* st) {
    return user_block<0>(user, q, nbatch, rows, ndim, out, st);
}
__attribute__((visibility("default"))) int user_block_b(void* user, const double* q, int32_t nbatch, int64_t rows, int32_t ndim, double* out, void* st) {
    return user_block<1>(user, q, nbatch, rows, ndim, out, st);
}
__attribute__((visibility("default"))) int user_block_n(void* user, const double* q, int32_t nbatch, int64_t rows, int32_t ndim, double* out, void* st) {
    return user_block<2>(user, q, nbatch, rows, ndim, out, st);
}

// mu, ivar (nbatch, ndim) and data (nbatch, 3, USER_K) from the host -> the model (user of the callbacks); NULL on failure
__attribute__((visibility("default"))) void* user_setup(const double* mu, const double* ivar, const double* data, int nbatch, int ndim,
                                                         int nan_member, double nan_above) {
    if (nbatch < 1 || ndim != USER_NDIM) return nullptr;
    user_model* m = new user_model();
    m->nbatch = nbatch;
    m->ndim = ndim;
    const size_t pb = (size_t)nbatch * ndim * 8, db = (size_t)nbatch * 3 * USER_K * 8;
    double *dmu = nullptr, *div = nullptr, *dd = nullptr;
    if (hipMalloc((void**)&dmu, pb) != hipSuccess || hipMalloc((void**)&div, pb) != hipSuccess || hipMalloc((void**)&dd, db) != hipSuccess ||
        hipMalloc((void**)&m->dev, sizeof(user_dev)) != hipSuccess)
        return nullptr;
    m->host.mu = dmu;
    m->host.ivar = div;
    m->host.data = dd;
    m->host.nan_member = nan_member;
    m->host.nan_above = nan_above;
    if (hipMemcpy(dmu, mu, pb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(div, ivar, pb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dd, data, db, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->dev, &m->host, sizeof(user_dev), hipMemcpyHostToDevice) != hipSuccess)
        return nullptr;
    return m;
}

// the device pointer the fused functors take as `user`
__attribute__((visibility("default"))) void* user_device_pointer(void* user) { return ((user_model*)user)->dev; }

__attribute__((visibility("default"))) void user_teardown(void* user) {
    user_model* m = (user_model*)user;
    (void)hipFree((void*)m->host.mu);
    (void)hipFree((void*)m->host.ivar);
    (void)hipFree((void*)m->host.data);
    (void)hipFree(m->dev);
    delete m;
}

}  // extern "C"
