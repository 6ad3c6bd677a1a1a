// A USER's model with blobs for a single EnsembleSampler: a diagonal Gaussian, defined ONCE as a __device__ inline function and wrapped
//   * in the functor's four-argument form (EMX_FUSED_ENSEMBLE_TARGET: the blob-free run that the blob run must equal bit for bit), and
//   * in its five-argument form (EMX_FUSED_ENSEMBLE_TARGET_BLOBS), which also writes USER_NBLOBS derived quantities a row.
// Test material (tests/test_gpu_ensemble_fused_blobs.py, tests/test_ensemble_fused_blobs_cpu.py compile it with hipcc
// -ffp-contract=off, -DUSER_NDIM=<ndim> and -DUSER_NBLOBS=<K>); not part of the product.
//
// lp = -0.5 sum_d ivar[d] (x_d - mu[d])^2, accumulated over d in ascending order with a separate multiply and add; with a finite
// `box`, -inf unless every |x_d| <= box (the functors named *_box).  Every blob is one rounding away from the row, so that NumPy
// reproduces it exactly:
//     b[0] = x[0]      b[1] = x[ndim-1] + x[0]      b[2] = lp      b[k] = x[k % ndim] * (k + 1)   for k >= 3
#include <emx_fused_ensemble.hpp>

#include <stdint.h>

#if !defined(USER_NDIM) || !defined(USER_NBLOBS)
#error "compile with -DUSER_NDIM=<ndim> -DUSER_NBLOBS=<K>"
#endif

struct user_dev {             // device-resident; what the functors' `user` points at
    const double* mu;         // (ndim)
    const double* ivar;       // (ndim)
    double box;
};

struct user_model {           // host side
    user_dev host;
    user_dev* dev;
};

template <bool BOX>
__device__ inline double model_lp(const double* x, int ndim, const void* user) {
    const user_dev* u = (const user_dev*)user;
    if (BOX)
        for (int d = 0; d < ndim; ++d)
            if (!(x[d] >= -u->box && x[d] <= u->box)) return -__builtin_inf();
    double acc = 0.0;
    for (int d = 0; d < ndim; ++d) {
        const double r = x[d] - u->mu[d];
        acc = acc + u->ivar[d] * r * r;
    }
    return -0.5 * acc;
}

template <bool BOX>
struct Model {
    __device__ double operator()(const double* x, int ndim, int, const void* user) const { return model_lp<BOX>(x, ndim, user); }
    __device__ double operator()(const double* x, int ndim, int, const void* user, double* b) const {
        const double lp = model_lp<BOX>(x, ndim, user);
        b[0] = x[0];
        if (USER_NBLOBS > 1) b[1] = x[ndim - 1] + x[0];
        if (USER_NBLOBS > 2) b[2] = lp;
#pragma unroll
        for (int k = 3; k < USER_NBLOBS; ++k) b[k] = x[k % ndim] * (double)(k + 1);
        return lp;
    }
};

EMX_FUSED_ENSEMBLE_TARGET(user_plain, Model<false>, USER_NDIM)
EMX_FUSED_ENSEMBLE_TARGET(user_plain_box, Model<true>, USER_NDIM)
EMX_FUSED_ENSEMBLE_TARGET_BLOBS(user_blobs, Model<false>, USER_NDIM, USER_NBLOBS)
EMX_FUSED_ENSEMBLE_TARGET_BLOBS(user_blobs_box, Model<true>, USER_NDIM, USER_NBLOBS)

extern "C" {

// mu, ivar (ndim) from the host -> the model; NULL on failure
__attribute__((visibility("default"))) void* user_setup(const double* mu, const double* ivar, int ndim, double box) {
    if (ndim != USER_NDIM) return nullptr;
    user_model* m = new user_model();
    const size_t pb = (size_t)ndim * 8;
    double *dmu = nullptr, *div = nullptr;
    if (hipMalloc((void**)&dmu, pb) != hipSuccess || hipMalloc((void**)&div, pb) != hipSuccess ||
        hipMalloc((void**)&m->dev, sizeof(user_dev)) != hipSuccess)
        return nullptr;
    m->host.mu = dmu;
    m->host.ivar = div;
    m->host.box = box;
    if (hipMemcpy(dmu, mu, pb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(div, ivar, pb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->dev, &m->host, sizeof(user_dev), hipMemcpyHostToDevice) != hipSuccess)
        return nullptr;
    return m;
}

// the device pointer the functors take as `user`
__attribute__((visibility("default"))) void* user_device_pointer(void* user) { return ((user_model*)user)->dev; }

__attribute__((visibility("default"))) int user_nblobs() { return USER_NBLOBS; }

__attribute__((visibility("default"))) void user_teardown(void* user) {
    user_model* m = (user_model*)user;
    (void)hipFree((void*)m->host.mu);
    (void)hipFree((void*)m->host.ivar);
    (void)hipFree(m->dev);
    delete m;
}

}  // extern "C"
