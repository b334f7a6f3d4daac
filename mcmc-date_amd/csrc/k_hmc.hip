// k_hmc.hip -- leapfrog integrator of the Hamiltonian proposal on the device (gfx950).  SURVEY.md 8(f) row f3, second part.
//
// Potential: U(q) = -ln [ prior x likelihood x jacobianRootBranch ](state(q))       (`htargetWith`, app/Hamiltonian.hs:72-92)
// Position:  q = the masked, reversed fold of the state record (`toVector`, `getMask`, app/Hamiltonian.hs:33-60):
//            pos_field[i] in {0 birth, 1 death, 2 tH, 3 height, 4 rMu, 5 rVar, 6 rate}, pos_index[i] = node id.
// One leapfrog step (step size eps_b per chain, diagonal inverse masses):
//     p += eps/2 grad(q);   q += eps Minv p;   p += eps/2 grad(q)
// With a dense metric on the handle (D.metric = C = M^-1, mcd_hmc_set_metric) the drift is q += eps (C p), the product of
// metric_device.hpp by one workgroup per chain; the diagonal kernels and their expressions are untouched.
// The gradient comes from the batched kernels (k_prior_grad.hip for the prior, k_tree_grad.hip for the likelihood) plus
// the five-number Jacobian term (hmc_device.hpp: gradient entry, state slot and ln target of the position layout, shared with
// the NUTS kernels and the recorder); this file holds the element-wise part: assemble the gradient in the position layout,
// kick, drift and scatter the new position into the state arrays.  One thread per (chain, coordinate).  What an entry and a chain's workgroup
// do is written once, in leapfrog_device.hpp, for the kernels here and for the one-launch form (k_nuts_chain.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "leapfrog_device.hpp"
#include "mvn_kernels.h"

namespace mcd {

// p += kick * eps_b * dir_b * grad.  `dir` (+1 / -1 per chain, may be null = +1) integrates backwards in time (NUTS-style
// doubling).  The drift is a separate launch (k_hmc_drift): the Jacobian term of one coordinate reads state entries that
// belong to other coordinates, so every gradient entry is read before any position is written.
// use_pos_grad != 0: the gradient is taken from D.grad (position layout, supplied by the caller with the position)
// instead of being assembled from the outputs of the gradient kernels
__global__ __launch_bounds__(256) void k_hmc_kick(HmcDev D, double kick, int use_pos_grad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D.batch * D.dim) return;
    const int64_t b = i / D.dim;
    const int k = (int)(i - b * D.dim);
    hmc_kick_entry(D, i, b, kick, use_pos_grad ? D.grad[i] : hmc_grad_entry(D, b, D.pos_field[k], D.pos_index[k]));
}

// the state arrays receive the position D.q (masked-out entries keep their values)
__global__ __launch_bounds__(256) void k_hmc_scatter(HmcDev D)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D.batch * D.dim) return;
    const int64_t b = i / D.dim;
    const int k = (int)(i - b * D.dim);
    *hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]) = D.q[i];
}

__global__ __launch_bounds__(256) void k_hmc_drift(HmcDev D)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D.batch * D.dim) return;
    const int64_t b = i / D.dim;
    const int k = (int)(i - b * D.dim);
    double* slot = hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]);
    const double q = *slot + hmc_signed_eps(D, b) * D.inv_mass[k] * D.p[i];
    *slot = q;
    D.q[i] = q;
}

// value[b] = ln prior + ln likelihood + ln jacobianRootBranch of the current state; q and grad in the position layout
__global__ __launch_bounds__(256) void k_hmc_collect(HmcDev D)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D.batch * D.dim) return;
    const int64_t b = i / D.dim;
    const int k = (int)(i - b * D.dim);
    hmc_grad_collect_entry(D, i, b, k);
}

// kick and drift of one leapfrog step in ONE launch: a workgroup per chain, so that a barrier separates "every gradient entry of
// the chain has been read" (the Jacobian term of a coordinate reads state entries that belong to other coordinates) from "the
// new position is written into the state".  p += kick eps g;  q += eps M^-1 p.
// Dense: M^-1 = D.metric (metric_device.hpp), q += eps (C p); the diagonal form keeps its expressions.
template <bool Dense>
__global__ __launch_bounds__(256) void k_hmc_kick_drift(HmcDev D, double kick)
{
    __shared__ double xs[Dense ? kHmcDenseMaxDim : 1];
    hmc_kick_drift_chain<Dense>(D, blockIdx.x, kick, xs);
}

// the stand-alone drift (k_hmc_drift) under a dense metric: a workgroup per chain
__global__ __launch_bounds__(256) void k_hmc_drift_dense(HmcDev D)
{
    __shared__ double xs[kHmcDenseMaxDim];
    const int64_t b = blockIdx.x;
    hmc_drift_dense(D, b, hmc_signed_eps(D, b), xs);
}

// the drift under a dense metric in the across-chains form: Y = P C is k_metric_gemm.hip's product over all chains, q += e Y elementwise
__global__ __launch_bounds__(256) void k_hmc_drift_across(HmcDev D, const double* __restrict__ Y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D.batch * D.dim) return;
    const int64_t b = i / D.dim;
    const int k = (int)(i - b * D.dim);
    double* slot = hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]);
    const double q = *slot + hmc_signed_eps(D, b) * Y[i];
    *slot = q;
    D.q[i] = q;
}

// the closing half kick together with k_hmc_collect
__global__ __launch_bounds__(256) void k_hmc_kick_collect(HmcDev D, double kick)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D.batch * D.dim) return;
    const int64_t b = i / D.dim;
    const int k = (int)(i - b * D.dim);
    hmc_kick_collect_entry(D, i, b, k, kick);
}

static unsigned hmc_grid(const HmcDev& D) { return (unsigned)((D.batch * D.dim + 255) / 256); }

hipError_t launch_hmc_kick(const HmcDev& D, double kick, int use_pos_grad, hipStream_t st)
{
    hipLaunchKernelGGL(k_hmc_kick, dim3(hmc_grid(D)), dim3(256), 0, st, D, kick, use_pos_grad);
    return hipGetLastError();
}
hipError_t launch_hmc_scatter(const HmcDev& D, hipStream_t st)
{
    hipLaunchKernelGGL(k_hmc_scatter, dim3(hmc_grid(D)), dim3(256), 0, st, D);
    return hipGetLastError();
}
hipError_t launch_hmc_drift(const HmcDev& D, hipStream_t st)
{
    if (D.metric)
        hipLaunchKernelGGL(k_hmc_drift_dense, dim3((unsigned)D.batch), dim3(256), 0, st, D);
    else
        hipLaunchKernelGGL(k_hmc_drift, dim3(hmc_grid(D)), dim3(256), 0, st, D);
    return hipGetLastError();
}
hipError_t launch_hmc_drift_across(const HmcDev& D, const double* Y, hipStream_t st)
{
    hipLaunchKernelGGL(k_hmc_drift_across, dim3(hmc_grid(D)), dim3(256), 0, st, D, Y);
    return hipGetLastError();
}
hipError_t launch_hmc_kick_drift(const HmcDev& D, double kick, hipStream_t st)
{
    if (D.metric)
        hipLaunchKernelGGL(k_hmc_kick_drift<true>, dim3((unsigned)D.batch), dim3(256), 0, st, D, kick);
    else
        hipLaunchKernelGGL(k_hmc_kick_drift<false>, dim3((unsigned)D.batch), dim3(256), 0, st, D, kick);
    return hipGetLastError();
}
hipError_t launch_hmc_kick_collect(const HmcDev& D, double kick, hipStream_t st)
{
    hipLaunchKernelGGL(k_hmc_kick_collect, dim3(hmc_grid(D)), dim3(256), 0, st, D, kick);
    return hipGetLastError();
}
hipError_t launch_hmc_collect(const HmcDev& D, hipStream_t st)
{
    hipLaunchKernelGGL(k_hmc_collect, dim3(hmc_grid(D)), dim3(256), 0, st, D);
    return hipGetLastError();
}

}  // namespace mcd
