// leapfrog_device.hpp -- the element-wise part of a leapfrog step (k_hmc.hip has the integrator), as device functions: the kick and the
// collect of one entry, and the kick + drift of one chain by its workgroup of 256 threads.  k_hmc.hip's kernels call them, and so does the
// one-launch form (k_nuts_chain.hip), where n_steps leapfrog steps of a chain are one loop of its workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hmc_device.hpp"
#include "metric_device.hpp"
#include "mvn_kernels.h"

namespace mcd {

// eps_b with the direction of time dir_b (+1 / -1 per chain, null = +1)
__device__ __forceinline__ double hmc_signed_eps(const HmcDev& D, int64_t b) { return D.eps[b] * (D.dir ? D.dir[b] : 1.0); }

// the kick of entry i of chain b with the gradient entry g, which D.grad keeps
__device__ __forceinline__ void hmc_kick_entry(const HmcDev& D, int64_t i, int64_t b, double kick, double g)
{
    D.p[i] = D.p[i] + kick * hmc_signed_eps(D, b) * g;
    D.grad[i] = g;
}

// the position of entry i = (b, k) from the state arrays; coordinate 0 leaves the chain's ln target in D.value
__device__ __forceinline__ void hmc_collect_entry(const HmcDev& D, int64_t i, int64_t b, int k)
{
    D.q[i] = *hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]);
    if (k == 0) D.value[b] = hmc_ln_target(D, b);
}

// entry i = (b, k) of k_hmc_collect: the gradient entry from the gradient kernels' outputs, then the position and the ln target
__device__ __forceinline__ void hmc_grad_collect_entry(const HmcDev& D, int64_t i, int64_t b, int k)
{
    D.grad[i] = hmc_grad_entry(D, b, D.pos_field[k], D.pos_index[k]);
    hmc_collect_entry(D, i, b, k);
}

// entry i = (b, k) of k_hmc_kick_collect: the closing half kick together with the collect
__device__ __forceinline__ void hmc_kick_collect_entry(const HmcDev& D, int64_t i, int64_t b, int k, double kick)
{
    hmc_kick_entry(D, i, b, kick, hmc_grad_entry(D, b, D.pos_field[k], D.pos_index[k]));
    hmc_collect_entry(D, i, b, k);
}

// q += e (C p) for chain b under the dense metric: the chain's momenta D.p are final (a barrier or a launch boundary lies behind)
__device__ __forceinline__ void hmc_drift_dense(const HmcDev& D, int64_t b, double e, double* xs)
{
    const int64_t o = b * D.dim;
    double v[kMetricOwned];
    metric_apply(D.metric, D.dim, false, xs, [&](int k, int) { return D.p[o + k]; }, v);
    for (int c = 0; c < kMetricOwned; ++c) {
        const int k = (int)threadIdx.x + 256 * c;
        if (k >= D.dim) break;
        double* slot = hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]);
        const double q = *slot + e * v[c];
        *slot = q;
        D.q[o + k] = q;
    }
}

// kick and drift of one leapfrog step of chain b by its workgroup: a barrier separates "every gradient entry of the chain has been
// read" (the Jacobian term of a coordinate reads state entries that belong to other coordinates) from "the new position is written
// into the state".  p += kick eps g;  q += eps M^-1 p.
// Dense: M^-1 = D.metric (metric_device.hpp), q += eps (C p), xs its kHmcDenseMaxDim doubles of LDS; the diagonal form keeps its expressions.
template <bool Dense>
__device__ __forceinline__ void hmc_kick_drift_chain(const HmcDev& D, int64_t b, double kick, double* xs)
{
    const int64_t o = b * D.dim;
    const double e = hmc_signed_eps(D, b);
    for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
        const double g = hmc_grad_entry(D, b, D.pos_field[k], D.pos_index[k]);
        D.grad[o + k] = g;
        D.p[o + k] = D.p[o + k] + kick * e * g;
    }
    __syncthreads();
    if constexpr (Dense) {
        hmc_drift_dense(D, b, e, xs);
    } else {
        for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
            double* slot = hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]);
            const double q = *slot + e * D.inv_mass[k] * D.p[o + k];
            *slot = q;
            D.q[o + k] = q;
        }
    }
}

}  // namespace mcd
