// A USER's batched log-probability over every member of an EnsembleBatch, written as a HIP kernel and plugged into libemx
// through emx_set_batch_target_callback (include/emx.h).  Test material (tests/test_gpu_batch_callback.py compiles it with hipcc
// -ffp-contract=off on the GPU box); not part of the product.  Target: member b's diagonal Gaussian
// -0.5 sum_d ivar[b, d] (x_d - mu[b, d])^2, accumulated over d in ascending order with a separate multiply and add -- the order
// of the test's torch callable, so that the two give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

struct user_batch {
    double* mu;       // device, (nbatch, ndim)
    double* ivar;     // device, (nbatch, ndim)
    int nbatch, ndim;
    long long calls;  // host-side statistics for the test
    long long rows;
};

__global__ __launch_bounds__(256) void k_user_diag(const double* __restrict__ q, int nbatch, long long rows, int D,
                                                   const double* __restrict__ mu, const double* __restrict__ ivar,
                                                   double* __restrict__ out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // one thread per (member, row)
    if (k >= (long long)nbatch * rows) return;
    const long long b = k / rows;
    const double* x = q + k * D;
    double acc = 0.0;
    for (int d = 0; d < D; ++d) {
        const double r = x[d] - mu[b * D + d];
        acc = acc + ivar[b * D + d] * r * r;
    }
    out[k] = -0.5 * acc;
}

extern "C" {

void* user_setup(const double* mu_host, const double* ivar_host, int nbatch, int ndim) {
    if (nbatch < 1 || ndim < 1) return nullptr;
    user_batch* u = new user_batch();
    u->nbatch = nbatch;
    u->ndim = ndim;
    u->calls = u->rows = 0;
    const size_t bytes = (size_t)nbatch * ndim * 8;
    if (hipMalloc((void**)&u->mu, bytes) != hipSuccess || hipMalloc((void**)&u->ivar, bytes) != hipSuccess) return nullptr;
    if (hipMemcpy(u->mu, mu_host, bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(u->ivar, ivar_host, bytes, hipMemcpyHostToDevice) != hipSuccess)
        return nullptr;
    return u;
}

void user_stats(void* user, long long* calls, long long* rows) {
    user_batch* u = (user_batch*)user;
    *calls = u->calls;
    *rows = u->rows;
}

void user_teardown(void* user) {
    user_batch* u = (user_batch*)user;
    (void)hipFree(u->mu);
    (void)hipFree(u->ivar);
    delete u;
}

// emx_batch_log_prob_fn: enqueue on `hip_stream`, never synchronise
int user_batch_log_prob(void* user, const double* coords_dev, int32_t nbatch, int64_t rows, int32_t ndim, double* log_prob_dev,
                        void* hip_stream) {
    user_batch* u = (user_batch*)user;
    if (ndim != u->ndim || nbatch != u->nbatch) return 1;
    u->calls += 1;
    u->rows += rows;
    const long long n = (long long)nbatch * rows;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_user_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, coords_dev, (int)nbatch,
                       (long long)rows, (int)ndim, u->mu, u->ivar, log_prob_dev);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
