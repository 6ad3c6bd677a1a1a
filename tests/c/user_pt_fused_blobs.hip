// A USER's likelihood WITH BLOBS for a PTSampler, defined ONCE as a __device__ inline function and wrapped four ways:
//   * as a functor with blobs compiled into the tempered kernel without a prior functor (EMX_FUSED_PT_TARGET_BLOBS; targets.PTFused(nblobs = 4)),
//   * as the same functor with blobs and the prior functor (p),
//   * as the same functor WITHOUT blobs (EMX_FUSED_PT_TARGET), with and without the prior functor: the runs whose coordinates, log-probs,
//     likelihoods, ladders and counts the blob runs must reproduce bit for bit, and
//   * as batched callbacks with and without blobs (a kernel + an emx_batch_log_prob[_blobs]_fn; targets.BatchKernel), and the prior's.
// Test material (tests/test_gpu_pt_blobs.py, tests/test_pt_blobs_cpu.py compile it with hipcc -ffp-contract=off and -DUSER_NDIM=<ndim>);
// not part of the product.
//
// Likelihood: member m's diagonal Gaussian -0.5 sum_d ivar[m, d] (x_d - mu[m, d])^2, accumulated over d in ascending order
// (user_pt_fused.hip's (a)).  Prior (p): -0.5 * 0.01 * sum x_d^2 inside |x_d| <= bound, -inf outside (user_pt_fused.hip's).
// Blobs: {L itself, x[0] + x[1], x[0] * x[1], (double)member} -- single correctly rounded operations on stored numbers, so the tests
// compare them with NumPy's on get_chain() without a tolerance.  member = object * ntemps + rung in every wrapping.
#include <emx_pt_fused.hpp>

#include <stdint.h>

#ifndef USER_NDIM
#error "compile with -DUSER_NDIM=<ndim>"
#endif
#if USER_NDIM < 2
#error "the blobs read x[0] and x[1]"
#endif

#ifndef USER_NBLOBS
#define USER_NBLOBS 4
#endif

struct user_dev {             // device-resident; what the functors' `user` points at
    const double* mu;         // (members, ndim)
    const double* ivar;       // (members, ndim)
    double bound;             // prior (p)'s box
};

struct user_model {           // host side
    user_dev host;            // the device struct's image (device pointers)
    user_dev* dev;
    int members, ndim;
};

__device__ inline double like_g(const double* x, int ndim, int member, const void* user) {
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

__device__ inline double prior_p(const double* x, int ndim, int, const void* user) {
    const user_dev* u = (const user_dev*)user;
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) {
        if (!(x[d] >= -u->bound && x[d] <= u->bound)) return -__builtin_inf();
        acc = acc + x[d] * x[d];
    }
    return -0.005 * acc;
}

__device__ inline void the_blobs(double L, const double* x, int member, double* blobs) {
    blobs[0] = L;
    blobs[1] = x[0] + x[1];
    blobs[2] = x[0] * x[1];
    blobs[3] = (double)member;
}

// ---- the fused forms ----
struct LikeG {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return like_g(x, ndim, member, user); }
};
struct LikeGBlobs {
    __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const {
        const double L = like_g(x, ndim, member, user);
        the_blobs(L, x, member, blobs);
        return L;
    }
};
struct PriorP {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return prior_p(x, ndim, member, user); }
};

EMX_FUSED_PT_TARGET(pt_fused_g, LikeG, emx::NoFusedPrior, USER_NDIM)
EMX_FUSED_PT_TARGET(pt_fused_gp, LikeG, PriorP, USER_NDIM)
EMX_FUSED_PT_TARGET_BLOBS(pt_fused_g_blobs, LikeGBlobs, emx::NoFusedPrior, USER_NDIM, USER_NBLOBS)
EMX_FUSED_PT_TARGET_BLOBS(pt_fused_gp_blobs, LikeGBlobs, PriorP, USER_NDIM, USER_NBLOBS)

// ---- the batched-callback forms: one thread per (member, row) of the (members, rows, ndim) block ----
// MODEL 0: the likelihood (blobs non-null: with its blobs); 1: the prior
template <int MODEL>
__global__ __launch_bounds__(256) void k_user_block(const double* __restrict__ q, int members, long long rows, int D, const user_dev* u,
                                                    double* __restrict__ out, double* __restrict__ blobs) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (long long)members * rows) return;
    const int b = (int)(k / rows);
    const double* x = q + k * D;
    const double v = MODEL == 0 ? like_g(x, D, b, u) : prior_p(x, D, b, u);
    out[k] = v;
    if (MODEL == 0 && blobs) the_blobs(v, x, b, blobs + k * USER_NBLOBS);
}

template <int MODEL>
static int user_block(void* user, const double* coords_dev, int32_t members, int64_t rows, int32_t ndim, double* log_prob_dev, double* blobs_dev,
                      void* hip_stream) {
    user_model* m = (user_model*)user;
    if (ndim != m->ndim || members != m->members) return 1;
    const long long n = (long long)members * rows;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_user_block<MODEL>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, coords_dev, (int)members,
                       (long long)rows, (int)ndim, (const user_dev*)m->dev, log_prob_dev, blobs_dev);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" {

// emx_batch_log_prob_fn of the likelihood and of the prior: enqueue on `hip_stream`, never synchronise
__attribute__((visibility("default"))) int user_block_g(void* user, const double* q, int32_t members, int64_t rows, int32_t ndim, double* out, void* st) {
    return user_block<0>(user, q, members, rows, ndim, out, nullptr, st);
}
__attribute__((visibility("default"))) int user_block_p(void* user, const double* q, int32_t members, int64_t rows, int32_t ndim, double* out, void* st) {
    return user_block<1>(user, q, members, rows, ndim, out, nullptr, st);
}
// emx_batch_log_prob_blobs_fn of the likelihood
__attribute__((visibility("default"))) int user_block_g_blobs(void* user, const double* q, int32_t members, int64_t rows, int32_t ndim, double* out,
                                                              int32_t nblobs, double* blobs, void* st) {
    if (nblobs != USER_NBLOBS || !blobs) return 1;
    return user_block<0>(user, q, members, rows, ndim, out, blobs, st);
}

__attribute__((visibility("default"))) int user_nblobs() { return USER_NBLOBS; }

// mu, ivar (members, ndim) from the host and the prior's bound -> the model (user of the callbacks); NULL on failure
__attribute__((visibility("default"))) void* user_setup(const double* mu, const double* ivar, int members, int ndim, double bound) {
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
