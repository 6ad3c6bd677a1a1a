// A USER's models for a PTSampler, each defined ONCE as a __device__ inline function and wrapped twice:
//   * as a batched callback (a kernel + an emx_batch_log_prob_fn; targets.BatchKernel, likelihood or prior), and
//   * as a functor compiled into the tempered kernel (EMX_FUSED_PT_TARGET of emx_pt_fused.hpp; targets.PTFused).
// Test material (tests/test_gpu_pt_fused.py, tests/test_pt_fused_cpu.py compile it with hipcc -ffp-contract=off and
// -DUSER_NDIM=<ndim>); not part of the product.  The fused run must equal the callback run of the same functions bit for bit.
//
// Likelihood (a): member m's diagonal Gaussian -0.5 sum_d ivar[m, d] (x_d - mu[m, d])^2, accumulated over d in ascending order.
// Likelihood (m): the two-mode mixture of tools/pt_bench.py, log(0.25 N(x; -4, 0.3^2) + 0.75 N(x; +4, 0.3^2)), the same for every member.
// Likelihood (n): (a), but NaN for member `nan_member` wherever x_0 > nan_above (USER_WITH_NAN; the single-StretchMove kernel only).
// Prior (p): -0.5 * 0.01 * sum x_d^2 inside |x_d| <= bound, -inf outside.
// member = object * ntemps + rung in both wrappings.
#include <emx_pt_fused.hpp>

#include <stdint.h>

#ifndef USER_NDIM
#error "compile with -DUSER_NDIM=<ndim>"
#endif

struct user_dev {             // device-resident; what the functors' `user` points at
    const double* mu;         // (members, ndim)
    const double* ivar;       // (members, ndim)
    int nan_member;           // -1: none
    double nan_above;
    double bound;             // prior (p)'s box
};

struct user_model {           // host side
    user_dev host;            // the device struct's image (device pointers)
    user_dev* dev;
    int members, ndim;
};

__device__ inline double like_a(const double* x, int ndim, int member, const void* user) {
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

__device__ inline double like_m(const double* x, int ndim, int, const void*) {
    const double s2 = 0.3 * 0.3;
    double d1 = 0.0, d2 = 0.0;
    for (int d = 0; d < ndim; ++d) {
        d1 = d1 + (x[d] + 4.0) * (x[d] + 4.0);
        d2 = d2 + (x[d] - 4.0) * (x[d] - 4.0);
    }
    const double a = -1.3862943611198906 - 0.5 * d1 / s2;      // log 0.25
    const double b = -0.2876820724517809 - 0.5 * d2 / s2;      // log 0.75
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    const double norm = -0.5 * (double)ndim * log(2.0 * 3.141592653589793 * s2);
    return hi + log1p(exp(lo - hi)) + norm;
}

__device__ inline double like_n(const double* x, int ndim, int member, const void* user) {
    const user_dev* u = (const user_dev*)user;
    if (member == u->nan_member && x[0] > u->nan_above) return __builtin_nan("");
    return like_a(x, ndim, member, user);
}

__device__ inline double prior_p(const double* x, int ndim, int, const void* user) {
    const user_dev* u = (const user_dev*)user;
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) {
        if (!(x[d] >= -u->bound && x[d] <= u->bound)) return -__builtin_inf();
        acc = acc + x[d] * x[d];
    }
    return -0.005 * acc;
}

// ---- the batched-callback form: one thread per (member, row) of the (members, rows, ndim) block ----
template <int MODEL>
__global__ __launch_bounds__(256) void k_user_block(const double* __restrict__ q, int members, long long rows, int D, const user_dev* u,
                                                    double* __restrict__ out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (long long)members * rows) return;
    const int b = (int)(k / rows);
    const double* x = q + k * D;
    out[k] = MODEL == 0 ? like_a(x, D, b, u) : MODEL == 1 ? like_m(x, D, b, u) : MODEL == 2 ? like_n(x, D, b, u) : prior_p(x, D, b, u);
}

template <int MODEL>
static int user_block(void* user, const double* coords_dev, int32_t members, int64_t rows, int32_t ndim, double* log_prob_dev, void* hip_stream) {
    user_model* m = (user_model*)user;
    if (ndim != m->ndim || members != m->members) return 1;
    const long long n = (long long)members * rows;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_user_block<MODEL>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, coords_dev, (int)members,
                       (long long)rows, (int)ndim, (const user_dev*)m->dev, log_prob_dev);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// ---- the fused form ----
struct LikeA {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return like_a(x, ndim, member, user); }
};
struct LikeM {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return like_m(x, ndim, member, user); }
};
struct LikeN {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return like_n(x, ndim, member, user); }
};
struct PriorP {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return prior_p(x, ndim, member, user); }
};

EMX_FUSED_PT_TARGET(pt_fused_a, LikeA, emx::NoFusedPrior, USER_NDIM)
EMX_FUSED_PT_TARGET(pt_fused_ap, LikeA, PriorP, USER_NDIM)
EMX_FUSED_PT_TARGET(pt_fused_m, LikeM, emx::NoFusedPrior, USER_NDIM)
#ifdef USER_WITH_NAN
EMX_FUSED_PT_TARGET_MOVES(pt_fused_n, LikeN, emx::NoFusedPrior, USER_NDIM, EMX_FUSED_MOVES_STRETCH)
#endif

extern "C" {

// emx_batch_log_prob_fn of the likelihoods and of the prior: enqueue on `hip_stream`, never synchronise
__attribute__((visibility("default"))) int user_block_a(void* user, const double* q, int32_t members, int64_t rows, int32_t ndim, double* out, void* st) {
    return user_block<0>(user, q, members, rows, ndim, out, st);
}
__attribute__((visibility("default"))) int user_block_m(void* user, const double* q, int32_t members, int64_t rows, int32_t ndim, double* out, void* st) {
    return user_block<1>(user, q, members, rows, ndim, out, st);
}
__attribute__((visibility("default"))) int user_block_n(void* user, const double* q, int32_t members, int64_t rows, int32_t ndim, double* out, void* st) {
    return user_block<2>(user, q, members, rows, ndim, out, st);
}
__attribute__((visibility("default"))) int user_block_p(void* user, const double* q, int32_t members, int64_t rows, int32_t ndim, double* out, void* st) {
    return user_block<3>(user, q, members, rows, ndim, out, st);
}

// mu, ivar (members, ndim) from the host -> the model (user of the callbacks); NULL on failure
__attribute__((visibility("default"))) void* user_setup(const double* mu, const double* ivar, int members, int ndim, int nan_member,
                                                         double nan_above, double bound) {
    if (members < 1 || ndim != USER_NDIM) return nullptr;
    user_model* m = new user_model();
    m->members = members;
    m->ndim = ndim;
    const size_t pb = (size_t)members * ndim * 8;
    double *dmu = nullptr, *div = nullptr;
    if (hipMalloc((void**)&dmu, pb) != hipSuccess || hipMalloc((void**)&div, pb) != hipSuccess ||
        hipMalloc((void**)&m->dev, sizeof(user_dev)) != hipSuccess)
        return nullptr;
    m->host.mu = dmu;
    m->host.ivar = div;
    m->host.nan_member = nan_member;
    m->host.nan_above = nan_above;
    m->host.bound = bound;
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
