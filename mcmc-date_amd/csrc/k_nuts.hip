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
// next leaf, and the loop over the stack levels, which opens and closes them in one pass.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "metric_device.hpp"
#include "mh_device.hpp"
#include "mvn_kernels.h"
#include "nuts_device.hpp"

namespace mcd {

// (q_minus, r_minus, q_plus, r_plus) do not turn back on each other: (q+ - q-) . M^-1 r >= 0 at both ends (Algorithm 3)
template <bool Dense>
__device__ __forceinline__ bool nuts_no_u_turn(const HmcDev& D, const double* qm, const double* rm, const double* qp, const double* rp, double* red,
                                               double* xs)
{
    double a = 0.0, c = 0.0;
    if constexpr (Dense) {
        double w[kMetricOwned];
        metric_apply(D.metric, D.dim, false, xs, [&](int k, int) { return qp[k] - qm[k]; }, w);
        for (int i = 0; i < kMetricOwned; ++i) {
            const int k = (int)threadIdx.x + 256 * i;
            if (k >= D.dim) break;
            a += w[i] * rm[k];
            c += w[i] * rp[k];
        }
    } else {
        for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
            const double d = qp[k] - qm[k];
            a += d * (rm[k] * D.inv_mass[k]);
            c += d * (rp[k] * D.inv_mass[k]);
        }
    }
    a = nuts_block_sum(a, red);
    c = nuts_block_sum(c, red);
    return a >= 0.0 && c >= 0.0;
}

// the edge that is extended next goes to D.q / D.p / D.grad; half kick, drift, new position into the state arrays
template <bool Dense>
__device__ __forceinline__ void nuts_launch_leaf(const HmcDev& D, const NutsDev& N, int64_t b, int v, double* xs)
{
    const int64_t o = b * D.dim;
    const double* eq = (v < 0 ? N.qm : N.qp) + o;
    const double* ep = (v < 0 ? N.pm : N.pp) + o;
    const double* eg = (v < 0 ? N.gm : N.gp) + o;
    const double e = D.eps[b] * (double)v;
    if constexpr (Dense) {
        double cp[kMetricOwned];
        metric_apply(D.metric, D.dim, false, xs, [&](int k, int) { return ep[k] + 0.5 * e * eg[k]; }, cp);
        for (int i = 0; i < kMetricOwned; ++i) {
            const int k = (int)threadIdx.x + 256 * i;
            if (k >= D.dim) break;
            const double g = eg[k];
            const double p = ep[k] + 0.5 * e * g;                   // p += eps / 2 grad
            const double q = eq[k] + e * cp[i];                     // q += eps (C p)
            D.p[o + k] = p;
            D.q[o + k] = q;
            D.grad[o + k] = g;
            *hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]) = q;
        }
    } else {
        for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
            const double g = eg[k];
            const double p = ep[k] + 0.5 * e * g;                       // p += eps / 2 grad
            const double q = eq[k] + e * D.inv_mass[k] * p;             // q += eps M^-1 p
            D.p[o + k] = p;
            D.q[o + k] = q;
            D.grad[o + k] = g;
            *hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]) = q;
        }
    }
    if (threadIdx.x == 0) const_cast<double*>(D.dir)[b] = (double)v;
}

// Start of a transition: momenta, slice variable, the tree = the current point, first doubling, first leaf on its way.
// Needs D.q, D.grad, D.value of the current state (mcd_hmc_set_state / the previous transition).
template <bool Dense>
__global__ __launch_bounds__(256) void k_nuts_begin(HmcDev D, NutsDev N, uint64_t seed, int64_t chain0, uint64_t transition)
{
    __shared__ double red[4];
    __shared__ double xs[Dense ? kHmcDenseMaxDim : 1];
    const int64_t b = blockIdx.x;
    const int64_t o = b * D.dim;
    const Rng g = mh_rng(seed, chain0 + b, transition);
    double kin = 0.0;
    if constexpr (Dense) {
        double p[kMetricOwned], cp[kMetricOwned];
        metric_apply(D.metric_uinv, D.dim, true, xs, [&](int k, int) { return nuts_normal(g, k); }, p);   // p = U^-T z ~ N(0, C^-1) = N(0, M)
        metric_apply(D.metric, D.dim, false, xs, [&](int, int i) { return p[i]; }, cp);
        for (int i = 0; i < kMetricOwned; ++i) {
            const int k = (int)threadIdx.x + 256 * i;
            if (k >= D.dim) break;
            kin += p[i] * cp[i];
            nuts_tree_init(D, N, o + k, p[i]);
        }
    } else {
        for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
            const double z = nuts_normal(g, k);
            const double p = z / sqrt(D.inv_mass[k]);                   // p ~ N(0, M)
            kin += p * p * D.inv_mass[k];
            nuts_tree_init(D, N, o + k, p);
        }
    }
    kin = 0.5 * nuts_block_sum(kin, red);
    const int v = nuts_start(D, N, b, g, kin);
    __syncthreads();
    nuts_launch_leaf<Dense>(D, N, b, v, xs);
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
    const int64_t o = b * D.dim;
    const Rng rng = mh_rng(seed, chain0 + b, transition);
    const int v = N.v[b], j = N.j[b], i = N.i[b];
    const double e = D.eps[b] * (double)v;
    double* eq = (v < 0 ? N.qm : N.qp) + o;
    double* ep = (v < 0 ? N.pm : N.pp) + o;
    double* eg = (v < 0 ? N.gm : N.gp) + o;
    // ---- the new leaf: gradient from the kernels' outputs, second half kick, ln target; it becomes the tree's edge
    double kin = 0.0;
    for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
        const double g = hmc_grad_entry(D, b, D.pos_field[k], D.pos_index[k]);
        const double p = D.p[o + k] + 0.5 * e * g;
        if constexpr (!Dense) kin += p * p * D.inv_mass[k];
        eq[k] = D.q[o + k];
        ep[k] = p;
        eg[k] = g;
    }
    if constexpr (Dense) {                                          // 1/2 p^T C p; every thread reads back the entries it has just written
        double cp[kMetricOwned];
        metric_apply(D.metric, D.dim, false, xs, [&](int k, int) { return ep[k]; }, cp);
        for (int i = 0; i < kMetricOwned; ++i) {
            const int k = (int)threadIdx.x + 256 * i;
            if (k >= D.dim) break;
            kin += ep[k] * cp[i];
        }
    }
    kin = 0.5 * nuts_block_sum(kin, red);
    NutsLeaf L = nuts_book_leaf(D, N, b, rng, hmc_ln_target(D, b), kin, eq, eg);
    // ---- aligned sub trees: leaf i opens those of 2^k leaves with i % 2^k == 0 and closes those with (i + 1) % 2^k == 0
    for (int k = 1; k <= j; ++k) {
        const int size = 1 << k;
        double* lq = N.sq + ((int64_t)b * N.max_depth + (k - 1)) * D.dim;
        double* lr = N.sp + ((int64_t)b * N.max_depth + (k - 1)) * D.dim;
        if ((i & (size - 1)) == 0) {
            for (int c = threadIdx.x; c < D.dim; c += blockDim.x) {
                lq[c] = eq[c];
                lr[c] = ep[c];
            }
        } else if (((i + 1) & (size - 1)) == 0 && L.s1) {
            __syncthreads();
            // in time order: going forwards the first leaf is the minus end, going backwards the plus end
            const bool ok = v > 0 ? nuts_no_u_turn<Dense>(D, lq, lr, eq, ep, red, xs) : nuts_no_u_turn<Dense>(D, eq, ep, lq, lr, red, xs);
            L.s1 = L.s1 && ok;
        }
    }
    __syncthreads();
    const int vn = nuts_decide(D, N, b, rng, max_depth, v, j, i, L,
                               [&] { return nuts_no_u_turn<Dense>(D, N.qm + o, N.pm + o, N.qp + o, N.pp + o, red, xs); }, active, nullptr);
    if (vn) nuts_launch_leaf<Dense>(D, N, b, vn, xs);
}

// End of a transition: the proposal becomes the chain's state (position, gradient and ln target with it)
__global__ __launch_bounds__(256) void k_nuts_end(HmcDev D, NutsDev N)
{
    const int64_t b = blockIdx.x;
    const int64_t o = b * D.dim;
    for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
        const double q = N.qn[o + k];
        D.q[o + k] = q;
        D.grad[o + k] = N.gn[o + k];
        *hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]) = q;
    }
    if (threadIdx.x == 0) D.value[b] = N.lpn[b];
}

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
