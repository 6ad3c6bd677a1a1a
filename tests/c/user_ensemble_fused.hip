// A USER's models for a single EnsembleSampler, each defined ONCE as a __device__ inline function and wrapped twice:
//   * as a device callback (a kernel + an emx_device_log_prob_fn, the form of user_logprob.hip; targets.DeviceKernel), and
//   * as a functor compiled into the half-step kernel (EMX_FUSED_ENSEMBLE_TARGET of emx_fused_ensemble.hpp; targets.DeviceFused).
// Test material (tests/test_gpu_ensemble_fused.py, tests/test_ensemble_fused_cpu.py compile it with hipcc -ffp-contract=off and
// -DUSER_NDIM=<ndim>); not part of the product.  The fused run must equal the callback run of the same function bit for bit.
//
// Model (a): the diagonal Gaussian -0.5 sum_d ivar[d] (x_d - mu[d])^2, accumulated over d in ascending order with a separate
// multiply and add; mu and ivar live behind `user`.
// Model (b): a straight-line fit to K = 20 points, y_k ~ N(x_0 + x_1 t_k, yerr_k^2), the coordinates beyond the second under a
// unit Gaussian, inside a box: -inf unless every |x_d| <= box.
// Model (n): model (a), but NaN wherever x_0 > nan_above.
#include <emx_fused_ensemble.hpp>

#include <stdint.h>

#ifndef USER_NDIM
#error "compile with -DUSER_NDIM=<ndim>"
#endif

#define USER_K 20

struct user_dev {             // device-resident; what the functors' `user` points at
    const double* mu;         // (ndim)
    const double* ivar;       // (ndim)
    const double* data;       // (3, USER_K): t, y, yerr
    double box;
    double nan_above;
};

struct user_model {           // host side
    user_dev host;            // the device struct's image (device pointers)
    user_dev* dev;
    int ndim;
};

__device__ inline double model_a(const double* x, int ndim, const void* user) {
    const user_dev* u = (const user_dev*)user;
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) {
        const double r = x[d] - u->mu[d];
        acc = acc + u->ivar[d] * r * r;
    }
    return -0.5 * acc;
}

__device__ inline double model_b(const double* x, int ndim, const void* user) {
    const user_dev* u = (const user_dev*)user;
    for (int d = 0; d < ndim; ++d)
        if (!(x[d] >= -u->box && x[d] <= u->box)) return -__builtin_inf();
    const double* t = u->data;
    const double *y = t + USER_K, *yerr = y + USER_K;
    const double slope = ndim > 1 ? x[1] : 0.0;
    double acc = 0.0;
    for (int k = 0; k < USER_K; ++k) {
        const double r = (y[k] - (x[0] + slope * t[k])) / yerr[k];
        acc = acc + r * r;
    }
    for (int d = 2; d < ndim; ++d) acc = acc + x[d] * x[d];
    return -0.5 * acc;
}

__device__ inline double model_n(const double* x, int ndim, const void* user) {
    const user_dev* u = (const user_dev*)user;
    if (x[0] > u->nan_above) return __builtin_nan("");
    return model_a(x, ndim, user);
}

// ---- the device-callback form: one thread per row of the (n, ndim) block ----
template <int MODEL>
__global__ __launch_bounds__(256) void k_user_rows(const double* __restrict__ q, long long n, int D, const user_dev* u, double* __restrict__ out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double* x = q + k * D;
    out[k] = MODEL == 0 ? model_a(x, D, u) : MODEL == 1 ? model_b(x, D, u) : model_n(x, D, u);
}

template <int MODEL>
static int user_rows(void* user, const double* coords_dev, int64_t n, int32_t ndim, double* log_prob_dev, void* hip_stream) {
    user_model* m = (user_model*)user;
    if (ndim != m->ndim) return 1;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_user_rows<MODEL>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, coords_dev, (long long)n,
                       (int)ndim, (const user_dev*)m->dev, log_prob_dev);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// ---- the fused form ----
struct ModelA {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const { return model_a(x, ndim, user); }
};
struct ModelB {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const { return model_b(x, ndim, user); }
};
struct ModelN {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const { return model_n(x, ndim, user); }
};

EMX_FUSED_ENSEMBLE_TARGET(user_fused_a, ModelA, USER_NDIM)
#ifndef USER_ONLY_A
EMX_FUSED_ENSEMBLE_TARGET(user_fused_b, ModelB, USER_NDIM)
EMX_FUSED_ENSEMBLE_TARGET(user_fused_n, ModelN, USER_NDIM)
#endif

extern "C" {

// emx_device_log_prob_fn of the three models: enqueue on `hip_stream`, never synchronise
__attribute__((visibility("default"))) int user_rows_a(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<0>(user, q, n, ndim, out, st);
}
__attribute__((visibility("default"))) int user_rows_b(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<1>(user, q, n, ndim, out, st);
}
__attribute__((visibility("default"))) int user_rows_n(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<2>(user, q, n, ndim, out, st);
}

// mu, ivar (ndim) and data (3, USER_K) from the host -> the model (user of the callbacks); NULL on failure
__attribute__((visibility("default"))) void* user_setup(const double* mu, const double* ivar, const double* data, int ndim, double box,
                                                         double nan_above) {
    if (ndim != USER_NDIM) return nullptr;
    user_model* m = new user_model();
    m->ndim = ndim;
    const size_t pb = (size_t)ndim * 8, db = (size_t)3 * USER_K * 8;
    double *dmu = nullptr, *div = nullptr, *dd = nullptr;
    if (hipMalloc((void**)&dmu, pb) != hipSuccess || hipMalloc((void**)&div, pb) != hipSuccess || hipMalloc((void**)&dd, db) != hipSuccess ||
        hipMalloc((void**)&m->dev, sizeof(user_dev)) != hipSuccess)
        return nullptr;
    m->host.mu = dmu;
    m->host.ivar = div;
    m->host.data = dd;
    m->host.box = box;
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
