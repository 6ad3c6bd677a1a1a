// A USER's likelihoods that sum over data, for a single EnsembleSampler.  Each model's `base` and `term` are defined ONCE and wrapped
// three ways:
//   * as a data target (EMX_FUSED_ENSEMBLE_DATA_TARGET of emx_fused_ensemble_data.hpp; targets.DeviceFused(..., ndata=)): a wave a row;
//   * as a device callback (a kernel + an emx_device_log_prob_fn; targets.DeviceKernel) with one thread a row that keeps 64 partials
//     in a local array and adds them by the pairwise tree: the order the header defines, written serially;
//   * as a plain functor of the same serial form (EMX_FUSED_ENSEMBLE_TARGET of emx_fused_ensemble.hpp), one lane a row: what a
//     user had before the data target (tools/ensemble_fused_data_bench.py measures against it).
// Test material (tests/test_gpu_ensemble_fused_data.py, tests/test_ensemble_fused_data_cpu.py compile it with hipcc
// -ffp-contract=off and -DUSER_NDIM=<ndim>); not part of the product.  The three must agree bit for bit.
//
// Data: (3, ndata) behind `user`: t, y, sigma.
// Model (a): a straight-line fit, slope x_0 and intercept x_1 (0 at ndim 1): base is a flat prior on the box |x_d| <= box (-inf
//            outside), term is -0.5 ((y_k - x_0 t_k - x_1) / sigma_k)^2.  Only + - * /: NumPy reproduces its bits.
// Model (b): the same with the polynomial sum_d x_d t_k^d (Horner, highest power first) of ndim coefficients.
// Model (c): model (b), but term returns NaN outside the box, where base returns -inf: the terms of such a row are never evaluated.
// Model (d): model (b), but term is NaN wherever x_0 > nan_above (inside the box).
#include <emx_fused_ensemble_data.hpp>

#include <stdint.h>

#ifndef USER_NDIM
#error "compile with -DUSER_NDIM=<ndim>"
#endif

struct user_dev {             // device-resident; what `user` points at
    const double* data;       // (3, ndata): t, y, sigma
    long long ndata;
    double box;
    double nan_above;
};

struct user_model {           // host side
    user_dev host;            // the device struct's image (device pointers)
    user_dev* dev;
    int ndim;
};

__device__ inline bool in_box(const double* x, int ndim, const user_dev* u) {
    for (int d = 0; d < ndim; ++d)
        if (!(x[d] >= -u->box && x[d] <= u->box)) return false;
    return true;
}

template <int MODEL>
struct Model {
    __device__ double base(const double* x, int ndim, const void* user) const {
        return in_box(x, ndim, (const user_dev*)user) ? 0.0 : -__builtin_inf();
    }
    __device__ double term(const double* x, int ndim, long long k, const void* user) const {
        const user_dev* u = (const user_dev*)user;
        const double t = u->data[k], y = u->data[u->ndata + k], s = u->data[2 * u->ndata + k];
        if (MODEL == 2 && !in_box(x, ndim, u)) return __builtin_nan("");
        if (MODEL == 3 && x[0] > u->nan_above) return __builtin_nan("");
        double r;
        if (MODEL == 0) {
            r = y - x[0] * t;
            if (ndim > 1) r = r - x[1];
        } else {
            double mu = x[ndim - 1];
            for (int d = ndim - 2; d >= 0; --d) mu = mu * t + x[d];
            r = y - mu;
        }
        r = r / s;
        return -0.5 * (r * r);
    }
};

// the defined order written serially: partial l adds the terms l, l + 64, ... in ascending k; then adjacent pairs, level by level
template <int MODEL>
__device__ inline double serial_log_prob(const double* x, int ndim, const void* user) {
    const Model<MODEL> m;
    const double b = m.base(x, ndim, user);
    if (b != b || b == -__builtin_inf()) return b;
    const long long ndata = ((const user_dev*)user)->ndata;
    double p[64];
#pragma unroll
    for (int l = 0; l < 64; ++l) p[l] = 0.0;
    for (long long k0 = 0; k0 < ndata; k0 += 64) {
#pragma unroll
        for (int l = 0; l < 64; ++l)
            if (k0 + l < ndata) p[l] = p[l] + m.term(x, ndim, k0 + l, user);
    }
#pragma unroll
    for (int w = 64; w > 1; w /= 2)
#pragma unroll
        for (int l = 0; l < w / 2; ++l) p[l] = p[2 * l] + p[2 * l + 1];
    return b + p[0];
}

// ---- the device-callback form: one thread per row of the (n, ndim) block ----
template <int MODEL>
__global__ __launch_bounds__(64) void k_user_rows(const double* __restrict__ q, long long n, int D, const user_dev* u, double* __restrict__ out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    out[k] = serial_log_prob<MODEL>(q + k * D, D, u);
}

template <int MODEL>
static int user_rows(void* user, const double* coords_dev, int64_t n, int32_t ndim, double* log_prob_dev, void* hip_stream) {
    user_model* m = (user_model*)user;
    if (ndim != m->ndim) return 1;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_user_rows<MODEL>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream, coords_dev, (long long)n,
                       (int)ndim, (const user_dev*)m->dev, log_prob_dev);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// ---- the plain one-lane functor of the same serial form ----
template <int MODEL>
struct Serial {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const { return serial_log_prob<MODEL>(x, ndim, user); }
};

EMX_FUSED_ENSEMBLE_DATA_TARGET(user_data_a, Model<0>, USER_NDIM)
EMX_FUSED_ENSEMBLE_TARGET(user_serial_a, Serial<0>, USER_NDIM)
#ifndef USER_ONLY_A
EMX_FUSED_ENSEMBLE_DATA_TARGET(user_data_b, Model<1>, USER_NDIM)
EMX_FUSED_ENSEMBLE_DATA_TARGET(user_data_c, Model<2>, USER_NDIM)
EMX_FUSED_ENSEMBLE_DATA_TARGET(user_data_d, Model<3>, USER_NDIM)
#endif

extern "C" {

// emx_device_log_prob_fn of the four models: enqueue on `hip_stream`, never synchronise
__attribute__((visibility("default"))) int user_rows_a(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<0>(user, q, n, ndim, out, st);
}
#ifndef USER_ONLY_A
__attribute__((visibility("default"))) int user_rows_b(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<1>(user, q, n, ndim, out, st);
}
__attribute__((visibility("default"))) int user_rows_c(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<2>(user, q, n, ndim, out, st);
}
__attribute__((visibility("default"))) int user_rows_d(void* user, const double* q, int64_t n, int32_t ndim, double* out, void* st) {
    return user_rows<3>(user, q, n, ndim, out, st);
}
#endif

// data (3, ndata) from the host -> the model (user of the callbacks); NULL on failure
__attribute__((visibility("default"))) void* user_setup(const double* data, long long ndata, int ndim, double box, double nan_above) {
    if (ndim != USER_NDIM || ndata < 0) return nullptr;
    user_model* m = new user_model();
    m->ndim = ndim;
    const size_t db = (size_t)3 * (size_t)(ndata > 0 ? ndata : 1) * 8;
    double* dd = nullptr;
    if (hipMalloc((void**)&dd, db) != hipSuccess || hipMalloc((void**)&m->dev, sizeof(user_dev)) != hipSuccess) return nullptr;
    m->host.data = dd;
    m->host.ndata = ndata;
    m->host.box = box;
    m->host.nan_above = nan_above;
    if ((ndata > 0 && hipMemcpy(dd, data, (size_t)3 * ndata * 8, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(m->dev, &m->host, sizeof(user_dev), hipMemcpyHostToDevice) != hipSuccess)
        return nullptr;
    return m;
}

// the device pointer the fused targets take as `user`
__attribute__((visibility("default"))) void* user_device_pointer(void* user) { return ((user_model*)user)->dev; }

__attribute__((visibility("default"))) void user_teardown(void* user) {
    user_model* m = (user_model*)user;
    (void)hipFree((void*)m->host.data);
    (void)hipFree(m->dev);
    delete m;
}

}  // extern "C"
