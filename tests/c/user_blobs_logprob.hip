// A USER's models WITH BLOBS for an EnsembleBatch, each defined ONCE as a __device__ inline function and wrapped three times:
//   * as a functor with blobs compiled into the batch kernel (EMX_FUSED_BATCH_TARGET_BLOBS; targets.BatchFused(nblobs = 4)),
//   * as the same functor WITHOUT blobs (EMX_FUSED_BATCH_TARGET): the run whose coordinates, log-probs and accept counts the
//     blob run must reproduce bit for bit, and
//   * as a batched callback with blobs (a kernel + an emx_batch_log_prob_blobs_fn; targets.BatchKernel(nblobs = 4)).
// Test material (tests/test_gpu_batch_blobs.py, tests/test_batch_blobs_cpu.py compile it with hipcc -ffp-contract=off and
// -DUSER_NDIM=<ndim>); not part of the product.
//
// Blobs of every model: {the log-probability itself, x[0] + x[1], x[0] * x[1], (double)member} -- single correctly rounded
// operations on stored coordinates, so the tests compare them with NumPy's on get_chain() without a tolerance.
// Model (g): member b's diagonal Gaussian -0.5 sum_d ivar[b, d] (x_d - mu[b, d])^2 (user_fused_logprob.hip's model (a)).
// Model (x): model (g) inside the box |x_d| <= half for every d, -inf outside; every -inf evaluation is counted in the device
// word `ninf`, so a test can tell that the region was hit.  The blobs are written in the -inf case too ({-inf, ...}): they must
// never reach a walker.
#include <emx_fused_target.hpp>

#include <stdint.h>

#ifndef USER_NDIM
#error "compile with -DUSER_NDIM=<ndim>"
#endif
#if USER_NDIM < 2
#error "the blobs read x[0] and x[1]"
#endif

#define USER_NBLOBS 4

struct user_dev {             // device-resident; what the functors' `user` points at
    const double* mu;         // (nbatch, ndim)
    const double* ivar;       // (nbatch, ndim)
    double half;              // model (x)'s box
    unsigned long long* ninf; // model (x)'s -inf evaluations
};

struct user_model {           // host side
    user_dev host;
    user_dev* dev;
    int nbatch, ndim;
};

__device__ inline double model_g(const double* x, int ndim, int member, const void* user) {
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

__device__ inline double model_x(const double* x, int ndim, int member, const void* user) {
    const user_dev* u = (const user_dev*)user;
    for (int d = 0; d < ndim; ++d)
        if (!(x[d] >= -u->half && x[d] <= u->half)) {
            atomicAdd(u->ninf, 1ull);
            return -__builtin_inf();
        }
    return model_g(x, ndim, member, user);
}

__device__ inline void the_blobs(double lp, const double* x, int member, double* blobs) {
    blobs[0] = lp;
    blobs[1] = x[0] + x[1];
    blobs[2] = x[0] * x[1];
    blobs[3] = (double)member;
}

// ---- the fused forms ----
struct ModelG {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return model_g(x, ndim, member, user); }
};
struct ModelGBlobs {
    __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const {
        const double lp = model_g(x, ndim, member, user);
        the_blobs(lp, x, member, blobs);
        return lp;
    }
};
struct ModelX {
    __device__ double operator()(const double* x, int ndim, int member, const void* user) const { return model_x(x, ndim, member, user); }
};
struct ModelXBlobs {
    __device__ double operator()(const double* x, int ndim, int member, const void* user, double* blobs) const {
        const double lp = model_x(x, ndim, member, user);
        the_blobs(lp, x, member, blobs);
        return lp;
    }
};

EMX_FUSED_BATCH_TARGET(user_fused_g, ModelG, USER_NDIM)
EMX_FUSED_BATCH_TARGET_BLOBS(user_fused_g_blobs, ModelGBlobs, USER_NDIM, USER_NBLOBS)
EMX_FUSED_BATCH_TARGET(user_fused_x, ModelX, USER_NDIM)
EMX_FUSED_BATCH_TARGET_BLOBS(user_fused_x_blobs, ModelXBlobs, USER_NDIM, USER_NBLOBS)

// ---- the batched-callback form with blobs: one thread per (member, row) of the (nbatch, rows, ndim) block ----
template <int MODEL>
__global__ __launch_bounds__(256) void k_user_block_blobs(const double* __restrict__ q, int nbatch, long long rows, int D, const user_dev* u,
                                                          double* __restrict__ out, double* __restrict__ blobs) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (long long)nbatch * rows) return;
    const int b = (int)(k / rows);
    const double* x = q + k * D;
    const double lp = MODEL == 0 ? model_g(x, D, b, u) : model_x(x, D, b, u);
    out[k] = lp;
    the_blobs(lp, x, b, blobs + k * USER_NBLOBS);
}

template <int MODEL>
static int user_block_blobs(void* user, const double* coords_dev, int32_t nbatch, int64_t rows, int32_t ndim, double* log_prob_dev,
                            int32_t nblobs, double* blobs_dev, void* hip_stream) {
    user_model* m = (user_model*)user;
    if (ndim != m->ndim || nbatch != m->nbatch || nblobs != USER_NBLOBS || !blobs_dev) return 1;
    const long long n = (long long)nbatch * rows;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_user_block_blobs<MODEL>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, coords_dev,
                       (int)nbatch, (long long)rows, (int)ndim, (const user_dev*)m->dev, log_prob_dev, blobs_dev);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" {

// emx_batch_log_prob_blobs_fn of the two models: enqueue on `hip_stream`, never synchronise
__attribute__((visibility("default"))) int user_block_g_blobs(void* user, const double* q, int32_t nbatch, int64_t rows, int32_t ndim, double* out,
                                                              int32_t nblobs, double* blobs, void* st) {
    return user_block_blobs<0>(user, q, nbatch, rows, ndim, out, nblobs, blobs, st);
}
__attribute__((visibility("default"))) int user_block_x_blobs(void* user, const double* q, int32_t nbatch, int64_t rows, int32_t ndim, double* out,
                                                              int32_t nblobs, double* blobs, void* st) {
    return user_block_blobs<1>(user, q, nbatch, rows, ndim, out, nblobs, blobs, st);
}

__attribute__((visibility("default"))) int user_nblobs() { return USER_NBLOBS; }

// mu, ivar (nbatch, ndim) from the host and the box half-width -> the model (user of the callbacks); NULL on failure
__attribute__((visibility("default"))) void* user_setup(const double* mu, const double* ivar, int nbatch, int ndim, double half) {
    if (nbatch < 1 || ndim != USER_NDIM) return nullptr;
    user_model* m = new user_model();
    m->nbatch = nbatch;
    m->ndim = ndim;
    const size_t pb = (size_t)nbatch * ndim * 8;
    double *dmu = nullptr, *div = nullptr;
    if (hipMalloc((void**)&dmu, pb) != hipSuccess || hipMalloc((void**)&div, pb) != hipSuccess ||
        hipMalloc((void**)&m->host.ninf, 8) != hipSuccess || hipMalloc((void**)&m->dev, sizeof(user_dev)) != hipSuccess)
        return nullptr;
    m->host.mu = dmu;
    m->host.ivar = div;
    m->host.half = half;
    if (hipMemcpy(dmu, mu, pb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(div, ivar, pb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(m->host.ninf, 0, 8) != hipSuccess || hipMemcpy(m->dev, &m->host, sizeof(user_dev), hipMemcpyHostToDevice) != hipSuccess)
        return nullptr;
    return m;
}

// the device pointer the fused functors take as `user`
__attribute__((visibility("default"))) void* user_device_pointer(void* user) { return ((user_model*)user)->dev; }

// model (x)'s -inf evaluations so far (synchronises the device)
__attribute__((visibility("default"))) long long user_ninf(void* user) {
    unsigned long long n = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&n, ((user_model*)user)->host.ninf, 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (long long)n;
}

__attribute__((visibility("default"))) void user_teardown(void* user) {
    user_model* m = (user_model*)user;
    (void)hipFree((void*)m->host.mu);
    (void)hipFree((void*)m->host.ivar);
    (void)hipFree((void*)m->host.ninf);
    (void)hipFree(m->dev);
    delete m;
}

}  // extern "C"
