// k_nuts.hip -- the No-U-Turn sampler's tree building on the device, for B chains in lock step (gfx950).
// the reference's Hamiltonian proposal is `nuts` of the package `mcmc` (`nutsWith`,
// app/Hamiltonian.hs:95-105; dschrempf/mcmc 542c43f6, not vendored), restated from the algorithm it implements: Hoffman &
// Gelman, "The No-U-Turn Sampler", JMLR 15 (2014), Algorithm 3 -- slice variable, doubling in a random direction, U-turn
// and divergence stops, a uniform draw from the admissible leaves of the new sub tree, the biased progressive choice between
// the sub tree's candidate and the current proposal.
//
// The recursion of Algorithm 3 is unrolled into a per-chain state machine (doubling j, direction v, leaf index i inside the
// sub tree of 2^j leaves): every leapfrog step of every chain is one round of
//     [ k_nuts_step: finish the step, book the new leaf, load the edge to extend next, half kick + drift ]
//     [ k_prior_grad ] [ k_tree_grad ]                          (gradient of ln prior / ln likelihood at the new position)
// so a chain's tree needs no host decision.  The U-turn test of every aligned sub tree of 2^k leaves (what the recursion checks
// when two halves are joined) uses a stack of the sub trees' first leaves, one level per k; the candidate inside the new
// sub tree is chosen by reservoir sampling over its admissible leaves (the same uniform law as the recursion's pairwise
// choices, with other random numbers).  Chains that have finished wait for the others; the host only polls a counter.
//
// Random numbers: Philox4x32-10 as in the Metropolis-Hastings driver (mh_device.hpp), counter = (draw, chain, transition):
// draws 0x4000 + k / 2 -> momenta (Box-Muller pair), 1 -> slice, 0x10 + 2 j -> direction of doubling j, 0x11 + 2 j -> its
// merge, 0x100000 + leaf number -> reservoir.  tests/test_gpu_nuts.py holds the CPU twin that follows the same streams.
//
// One workgroup (256 threads) per chain; coordinates strided over the threads; dot products by workgroup reductions.
//
// The metric: diagonal inverse masses D.inv_mass, or -- template <Dense>, chosen by the launchers when D.metric is set
// (mcd_hmc_set_metric) -- a full inverse mass matrix C = U U^T: momenta p = U^-T z from the same normal draws z, kinetic energy
// 1/2 p^T C p, drift q += eps (C p), U-turn (q+ - q-)^T C r >= 0 at both ends from ONE product w = C (q+ - q-).  The products are
// metric_device.hpp's.  The dense metric's other form (mcd_hmc_set_metric_form: the products of all chains as one matrix product, any
// dim) is k_nuts_across.hip.
//
// The state machine itself is written once, in nuts_device.hpp, for the kernels of both files: the random streams, the start of a
// transition (nuts_tree_init, nuts_start), the booking of a leaf (nuts_book_leaf: slice test, divergence flag, reservoir, acceptance
// statistic) and the decision (nuts_decide: merge, U-turn of the whole tree as a callable, depth stop, write-back).  This file holds what
// belongs to the per-chain form: momenta, kinetic energy and U-turn products by the chain's own workgroup, the half kick + drift of the
// next leaf, and the loop over the stack levels, which opens and closes them in one pass -- as device functions in nuts_chain_device.hpp,
// which the one-launch transition (k_nuts_chain.hip) calls too; the kernels here are one call each.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mvn_kernels.h"
#include "nuts_chain_device.hpp"

namespace mcd {

// Start of a transition: momenta, slice variable, the tree = the current point, first doubling, first leaf on its way.
// Needs D.q, D.grad, D.value of the current state (mcd_hmc_set_state / the previous transition).
template <bool Dense>
__global__ __launch_bounds__(256) void k_nuts_begin(HmcDev D, NutsDev N, uint64_t seed, int64_t chain0, uint64_t transition)
{
    __shared__ double red[4];
    __shared__ double xs[Dense ? kHmcDenseMaxDim : 1];
    nuts_begin_chain<Dense>(D, N, blockIdx.x, seed, chain0, transition, red, xs);
}

// One round: the gradient kernels have run at the position the drift reached.  Finish the leapfrog step (second half kick),
// book the leaf, decide, and send the next leaf on its way -- or mark the chain done (nuts_book_leaf, nuts_decide: nuts_device.hpp).
template <bool Dense>
__global__ __launch_bounds__(256) void k_nuts_step(HmcDev D, NutsDev N, uint64_t seed, int64_t chain0, uint64_t transition, int max_depth,
                                                   int* __restrict__ active)
{
    __shared__ double red[4];
    __shared__ double xs[Dense ? kHmcDenseMaxDim : 1];
    const int64_t b = blockIdx.x;
    if (N.done[b]) return;                                          // workgroup-uniform
    nuts_step_chain<Dense>(D, N, b, seed, chain0, transition, max_depth, active, red, xs);
}

// End of a transition: the proposal becomes the chain's state (position, gradient and ln target with it)
__global__ __launch_bounds__(256) void k_nuts_end(HmcDev D, NutsDev N) { nuts_end_chain(D, N, blockIdx.x); }

hipError_t launch_nuts_begin(const HmcDev& D, const NutsDev& N, uint64_t seed, int64_t chain0, uint64_t transition, hipStream_t st)
{
    if (D.metric)
        hipLaunchKernelGGL(k_nuts_begin<true>, dim3((unsigned)D.batch), dim3(256), 0, st, D, N, seed, chain0, transition);
    else
        hipLaunchKernelGGL(k_nuts_begin<false>, dim3((unsigned)D.batch), dim3(256), 0, st, D, N, seed, chain0, transition);
    return hipGetLastError();
}
hipError_t launch_nuts_step(const HmcDev& D, const NutsDev& N, uint64_t seed, int64_t chain0, uint64_t transition, int max_depth, int* active,
                            hipStream_t st)
{
    if (D.metric)
        hipLaunchKernelGGL(k_nuts_step<true>, dim3((unsigned)D.batch), dim3(256), 0, st, D, N, seed, chain0, transition, max_depth, active);
    else
        hipLaunchKernelGGL(k_nuts_step<false>, dim3((unsigned)D.batch), dim3(256), 0, st, D, N, seed, chain0, transition, max_depth, active);
    return hipGetLastError();
}
hipError_t launch_nuts_end(const HmcDev& D, const NutsDev& N, hipStream_t st)
{
    hipLaunchKernelGGL(k_nuts_end, dim3((unsigned)D.batch), dim3(256), 0, st, D, N);
    return hipGetLastError();
}

}  // namespace mcd
