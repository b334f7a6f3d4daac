// metric_device.hpp -- the dense metric of the device leapfrog and NUTS (k_hmc.hip, k_nuts.hip): v = A x for one chain's workgroup.
//
// A is [dim][dim] row-major, dim <= kHmcDenseMaxDim = 512, and the product is taken down the COLUMNS: v_k = sum_j A[j dim + k] x_j, j
// ascending, one accumulator per coordinate.  For the stored inverse mass matrix C (exactly symmetric) that is C x with coalesced loads --
// at a fixed j the 256 threads read consecutive doubles of row j --; for the stored U^-1 (lower triangular) it is U^-T x, what turns
// standard normal draws into momenta with covariance C^-1 = M.  x is staged in LDS (<= 4 KiB) and broadcast; thread t owns the
// coordinates t and t + 256.  The order of the sum is fixed, so a chain's result does not depend on the batch, the launch or the other
// chains.  Workgroups of 256 threads only.
#pragma once
#include <hip/hip_runtime.h>

#include "mvn_kernels.h"

namespace mcd {

constexpr int kMetricOwned = kHmcDenseMaxDim / 256;      // coordinates per thread

// v[c] = (column product above) for the coordinate k = threadIdx.x + 256 c, where x_k = x(k, c).  `lower`: A is lower triangular, the sum
// starts at the first coordinate of the thread's wave (the rows skipped hold zeros for all its coordinates, and adding zeros changes nothing).  Every thread of the workgroup must call it (barriers inside); xs is the
// workgroup's staging array [kHmcDenseMaxDim], free for the next call on return of the NEXT barrier only -- the call begins with one.
template <class X>
__device__ __forceinline__ void metric_apply(const double* __restrict__ A, int dim, bool lower, double* xs, X x, double (&v)[kMetricOwned])
{
    __syncthreads();                                        // the previous product's readers are done with xs
    for (int c = 0; c < kMetricOwned; ++c) {
        const int k = (int)threadIdx.x + 256 * c;
        if (k < dim) xs[k] = x(k, c);
    }
    __syncthreads();
    const int k0 = (int)threadIdx.x, k1 = (int)threadIdx.x + 256;
    const bool own0 = k0 < dim, own1 = k1 < dim;
    double a0 = 0.0, a1 = 0.0;
    const int first = lower ? ((int)threadIdx.x & ~63) : 0;  // wave-uniform: rows above the wave's first coordinate hold zeros for all of them
    const double* row = A + (size_t)first * dim;
#pragma unroll 4
    for (int j = first; j < dim; ++j, row += dim) {
        const double xj = xs[j];
        if (own0) a0 += row[k0] * xj;
        if (own1) a1 += row[k1] * xj;
    }
    v[0] = a0;
    v[1] = a1;
}

}  // namespace mcd
