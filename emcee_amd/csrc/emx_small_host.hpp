// Host-side rules of the one-workgroup kernel k_small_run (emx_kernels.hpp), shared by the single-ensemble path (emx.hip:
// run_small, emx_set_target) and the batched one (emx_batch.hip): row layout, plan steps per pass, LDS bytes, threads, and
// the dense Gaussian target's image.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "emx_kernels.hpp"

namespace emx {

struct Shape {
    int G, V, CH;
};

// Row layout for a row of `Dcover` doubles: G lanes x CH chunks x V doubles, chosen to minimise
// the instructions per walker (few lanes per walker -> short cross-lane reductions, many walkers per
// pass) while every chunk of a row is still read as whole 128-byte lines (G*V*8 >= 128 B).
constexpr int shape_g(int cols) {
    return cols <= 4 ? 4 : cols <= 32 ? 8 : cols <= 64 ? 16 : cols <= 128 ? 32 : 64;
}
constexpr int shape_ch(int cols) {
    return cols <= 8 ? 1 : cols <= 16 ? 2 : cols <= 256 ? 4 : cols <= 512 ? 8 : 16;
}

inline Shape pick_shape(int D, int Dcover) {
    Shape s;
    s.V = (D % 2 == 0) ? 2 : 1;
    const int cols = (Dcover + s.V - 1) / s.V;
    s.G = shape_g(cols);
    s.CH = shape_ch(cols);
    return s;
}

// steps whose plans one pass evaluates: as many as give every thread of the workgroup an entry
inline int small_batch(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>(64, 1024 / N)); }

// dense_dp > 0: + the Cholesky image and one 16-row tile per wave; plan_steps 0: small_batch(N)
inline size_t small_lds_bytes(int64_t N, int D, int dense_dp = 0, int waves = 0, int plan_steps = 0) {
    const size_t B = (size_t)(plan_steps > 0 ? plan_steps : small_batch(N));
    size_t b = (size_t)N * ((size_t)D * 8 + 8 + 4 + 1) + B * (size_t)N * (3 * 8 + 4 * 4) + 64;
    if (dense_dp > 0) b += 16 + ((size_t)dense_img_doubles(dense_dp) + dense_dp + (size_t)waves * (16 * (dense_dp + 2) + 16)) * 8;
    return b;
}

// a fused user target's LDS staging area behind the rest (k_small_run<..., USER>): `rows` proposals (the largest split of the
// schedule) at D | 1 doubles a row, a factor each, and the 16-byte alignment
constexpr size_t small_fused_stage_bytes(int64_t rows, int D) { return 16 + (size_t)rows * ((size_t)(D | 1) * 8 + 8); }

// a fused user target's blobs in LDS behind the staging area (k_small_run<..., USER, NBLOBS>): nblobs doubles a walker
constexpr size_t small_blob_bytes(int64_t N, int nblobs) { return (size_t)N * (size_t)nblobs * 8; }

// blobs a sample of a batch target may carry
constexpr int BATCH_MAX_BLOBS = 32;

// widest padded ndim of a dense Gaussian target whose image the fused kernels and k_small_run keep in LDS
constexpr int DENSE_FUSED_MAX_DP = 128;

// the LDS a workgroup of k_small_run may hold (of the 160 KB of a gfx950 CU)
constexpr size_t SMALL_LDS_MAX = 150 * 1024;

// threads of the one workgroup: enough for one half-step's lanes and one plan entry each across the batch; the dense
// variant keeps one LDS tile per wave, so it takes the largest power-of-two wave count that still fits
inline int small_threads(int64_t N, int D, int Dp, int G, int minsplits, bool dense) {
    const int64_t nsmax = (N + minsplits - 1) / minsplits;
    const int64_t want = std::max<int64_t>(dense ? ((nsmax + 15) / 16) * 64 : nsmax * G, (int64_t)small_batch(N) * N);
    int threads = (int)std::min<int64_t>(1024, std::max<int64_t>(64, ((want + 63) / 64) * 64));
    if (dense) {
        int waves = threads / 64;
        while (waves > 1 && small_lds_bytes(N, D, Dp, waves) > SMALL_LDS_MAX) waves = (waves + 1) / 2;
        threads = waves * 64;
    }
    return threads;
}

// -0.5 d^T A d with A = sym(icov) = L L^T  ==  -0.5 |L^T d|^2: the image of a dense Gaussian target of ndim n (padded Dp),
// L in MFMA B-fragment order (zero padded) followed by the mean, Dp * Dp + Dp doubles.  Returns -1, or the row at which the
// Cholesky factorisation failed (icov not symmetric positive definite).
inline int dense_image(int n, const double* mu, const double* icov, std::vector<double>& img) {
    const int Dp = (n + 15) / 16 * 16, KK = Dp / 4;
    std::vector<double> Lm((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double sum = 0.5 * (icov[(size_t)i * n + j] + icov[(size_t)j * n + i]);
            for (int k = 0; k < j; ++k) sum -= Lm[(size_t)i * n + k] * Lm[(size_t)j * n + k];
            if (i == j) {
                if (!(sum > 0.0 && std::isfinite(sum))) return i;
                Lm[(size_t)i * n + i] = std::sqrt(sum);
            } else {
                Lm[(size_t)i * n + j] = sum / Lm[(size_t)j * n + j];
            }
        }
    img.assign((size_t)Dp * Dp + Dp, 0.0);
    for (int nb = 0; nb < Dp / 16; ++nb)
        for (int kk = 0; kk < KK; ++kk)
            for (int l = 0; l < 64; ++l) {
                const int k = 4 * kk + (l >> 4), col = 16 * nb + (l & 15);
                if (k < n && col < n && k >= col) img[((size_t)nb * KK + kk) * 64 + l] = Lm[(size_t)k * n + col];
            }
    for (int d = 0; d < n; ++d) img[(size_t)Dp * Dp + d] = mu[d];
    return -1;
}

// the fused kernels' and k_small_run's form of that image: only the non-zero 16 x 16 blocks (dense_block), then the mean;
// dense_img_doubles(Dp) + Dp doubles
inline std::vector<double> dense_pack(int Dp, const std::vector<double>& img) {
    const int B = Dp / 16, KK = Dp / 4;
    std::vector<double> packed((size_t)dense_img_doubles(Dp) + Dp, 0.0);
    for (int nb = 0; nb < B; ++nb)
        for (int kb = nb; kb < B; ++kb)
            for (int i = 0; i < 4; ++i)
                for (int l = 0; l < 64; ++l)
                    packed[((size_t)dense_block(B, nb, kb) * 4 + i) * 64 + l] = img[((size_t)nb * KK + 4 * kb + i) * 64 + l];
    for (int d = 0; d < Dp; ++d) packed[(size_t)dense_img_doubles(Dp) + d] = img[(size_t)Dp * Dp + d];
    return packed;
}

}  // namespace emx
