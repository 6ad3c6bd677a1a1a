// A USER's models for a SMALL EnsembleSampler -- one that fits one workgroup's LDS --, each defined ONCE as a __device__ inline
// function and wrapped three ways:
//   * as a device callback (a kernel + an emx_device_log_prob_fn; targets.DeviceKernel),
//   * as a functor compiled into the half-step kernel (EMX_FUSED_ENSEMBLE_TARGET[_BLOBS]; targets.DeviceFused), and
//   * the same functor compiled into the one-workgroup kernel (EMX_FUSED_ENSEMBLE_SMALL_TARGET[_BLOBS]; DeviceFused's small_fn).
// Test material (tests/test_gpu_ensemble_fused_small.py, tests/test_ensemble_fused_small_cpu.py compile it with hipcc
// -ffp-contract=off and -DUSER_NDIM=<ndim>); not part of the product.  All three runs must agree bit for bit.
//
// Model (a): the diagonal Gaussian -0.5 sum_d ivar[d] (x_d - mu[d])^2, accumulated over d in ascending order with a separate
// multiply and add; mu and ivar live behind `user`.
// -DUSER_EXTRA adds model (b): model (a) inside a box, -inf unless every |x_d| <= box, and model (n): model (a), but NaN wherever
// x_0 > nan_above.
// -DUSER_NBLOBS=<K> adds model (a) in the functor's five-argument form, every blob one rounding away from the row:
//     b[0] = x[0]      b[1] = x[ndim-1] + x[0]      b[2] = lp      b[k] = x[k % ndim] * (k + 1)   for k >= 3
#include <emx_fused_ensemble.hpp>

#include <stdint.h>

#ifndef USER_NDIM
#error "compile with -DUSER_NDIM=<ndim>"
#endif

struct user_dev {             // device-resident; what the functors' `user` points at
    const double* mu;         // (ndim)
    const double* ivar;       // (ndim)
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
    return model_a(x, ndim, user);
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

// ---- the fused forms ----
struct ModelA {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const { return model_a(x, ndim, user); }
#ifdef USER_NBLOBS
    __device__ double operator()(const double* x, int ndim, int, const void* user, double* b) const {
        const double lp = model_a(x, ndim, user);
        b[0] = x[0];
        if (USER_NBLOBS > 1) b[1] = x[ndim - 1] + x[0];
        if (USER_NBLOBS > 2) b[2] = lp;
#pragma unroll
        for (int k = 3; k < USER_NBLOBS; ++k) b[k] = x[k % ndim] * (double)(k + 1);
        return lp;
    }
#endif
};

EMX_FUSED_ENSEMBLE_TARGET(user_fused_a, ModelA, USER_NDIM)
EMX_FUSED_ENSEMBLE_SMALL_TARGET(user_small_a, ModelA, USER_NDIM)
#ifdef USER_NBLOBS
EMX_FUSED_ENSEMBLE_TARGET_BLOBS(user_fused_blobs, ModelA, USER_NDIM, USER_NBLOBS)
EMX_FUSED_ENSEMBLE_SMALL_TARGET_BLOBS(user_small_blobs, ModelA, USER_NDIM, USER_NBLOBS)
#endif
#ifdef USER_EXTRA
struct ModelB {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const { return model_b(x, ndim, user); }
};
struct ModelN {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const { return model_n(x, ndim, user); }
};
EMX_FUSED_ENSEMBLE_TARGET(user_fused_b, ModelB, USER_NDIM)
EMX_FUSED_ENSEMBLE_SMALL_TARGET(user_small_b, ModelB, USER_NDIM)
EMX_FUSED_ENSEMBLE_TARGET(user_fused_n, ModelN, USER_NDIM)
EMX_FUSED_ENSEMBLE_SMALL_TARGET(user_small_n, ModelN, USER_NDIM)
#endif

extern "C" {

// emx_device_log_prob_fn of the models: enqueue on `hip_stream`, never synchronise
__attribute__((visibility("default"))) int user_rows_a(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<0>(user, q, n, ndim, out, st);
}
#ifdef USER_EXTRA
__attribute__((visibility("default"))) int user_rows_b(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<1>(user, q, n, ndim, out, st);
}
__attribute__((visibility("default"))) int user_rows_n(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<2>(user, q, n, ndim, out, st);
}
#endif

// mu, ivar (ndim) from the host -> the model (user of the callbacks); NULL on failure
__attribute__((visibility("default"))) void* user_setup(const double* mu, const double* ivar, int ndim, double box, double nan_above) {
    if (ndim != USER_NDIM) return nullptr;
    user_model* m = new user_model();
    m->ndim = ndim;
    const size_t pb = (size_t)ndim * 8;
    double *dmu = nullptr, *div = nullptr;
    if (hipMalloc((void**)&dmu, pb) != hipSuccess || hipMalloc((void**)&div, pb) != hipSuccess ||
        hipMalloc((void**)&m->dev, sizeof(user_dev)) != hipSuccess)
        return nullptr;
    m->host.mu = dmu;
    m->host.ivar = div;
    m->host.box = box;
    m->host.nan_above = nan_above;
    if (hipMemcpy(dmu, mu, pb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(div, ivar, pb, hipMemcpyHostToDevice) != hipSuccess ||
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
    (void)hipFree(m->dev);
    delete m;
}

}  // extern "C"
