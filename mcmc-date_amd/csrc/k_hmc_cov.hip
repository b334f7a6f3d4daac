// k_hmc_cov.hip -- covariance of the positions one warm-up window visited (mcd_hmc_nuts_warmup_dense, gfx950): what the dense metric of
// the device NUTS is tuned from (`HTuneAllMasses`, app/Hamiltonian.hs:62-63).
//
// Two passes, never a sum of x^2 (the rule of k_summary.hip): the mean of every coordinate, then the centred products.  Both sums run
// over the sample index in ascending order in ONE accumulator per entry, no floating-point atomics: the same bits on every call, and
// cov[i][j] and cov[j][i] are the same products in the same order, so the result is exactly symmetric.  Runs once per window.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvn_kernels.h"

namespace mcd {

// mean[k] = sum_s Q[s][k] / n; one thread per coordinate, consecutive threads read consecutive doubles
__global__ __launch_bounds__(64) void k_hmc_cov_mean(const double* __restrict__ Q, int64_t n, int dim, double* __restrict__ mean)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= dim) return;
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += Q[i * dim + k];
    mean[k] = s / (double)n;
}

constexpr int COV_TILE = 16, COV_CHUNK = 32;

// cov[i][j] = sum_s (Q[s][i] - mean[i]) (Q[s][j] - mean[j]) / n; a 16 x 16 tile of entries per workgroup, the centred columns of both index
// ranges staged in LDS 32 samples at a time
__global__ __launch_bounds__(256) void k_hmc_cov_products(const double* __restrict__ Q, int64_t n, int dim, const double* __restrict__ mean,
                                                           double* __restrict__ cov)
{
    __shared__ double a[COV_CHUNK][COV_TILE], c[COV_CHUNK][COV_TILE];
    const int ti = threadIdx.x / COV_TILE, tj = threadIdx.x % COV_TILE;
    const int i0 = blockIdx.y * COV_TILE, j0 = blockIdx.x * COV_TILE;
    double acc = 0.0;
    for (int64_t s0 = 0; s0 < n; s0 += COV_CHUNK) {
        __syncthreads();
        for (int l = threadIdx.x; l < COV_CHUNK * COV_TILE; l += 256) {
            const int r = l / COV_TILE, k = l % COV_TILE;
            const int64_t s = s0 + r;
            const bool in_s = s < n;
            a[r][k] = (in_s && i0 + k < dim) ? Q[s * dim + i0 + k] - mean[i0 + k] : 0.0;
            c[r][k] = (in_s && j0 + k < dim) ? Q[s * dim + j0 + k] - mean[j0 + k] : 0.0;
        }
        __syncthreads();
        const int rows = (int)((n - s0 < COV_CHUNK) ? n - s0 : COV_CHUNK);
        for (int r = 0; r < rows; ++r) acc += a[r][ti] * c[r][tj];
    }
    if (i0 + ti < dim && j0 + tj < dim) cov[(size_t)(i0 + ti) * dim + (j0 + tj)] = acc / (double)n;
}

hipError_t launch_hmc_cov(const double* Q, int64_t n, int dim, double* mean, double* cov, hipStream_t st)
{
    hipLaunchKernelGGL(k_hmc_cov_mean, dim3((unsigned)((dim + 63) / 64)), dim3(64), 0, st, Q, n, dim, mean);
    const unsigned t = (unsigned)((dim + COV_TILE - 1) / COV_TILE);
    hipLaunchKernelGGL(k_hmc_cov_products, dim3(t, t), dim3(256), 0, st, Q, n, dim, mean, cov);
    return hipGetLastError();
}

}  // namespace mcd
