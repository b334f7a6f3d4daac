// nuts_chain_device.hpp -- the per-chain form of the NUTS tree building (k_nuts.hip has the algorithm and the random streams): what a
// chain's workgroup of 256 threads does at the start of a transition, after every leaf and at the end, as device functions.  k_nuts.hip's
// kernels are one call each; the one-launch transition (k_nuts_chain.hip) calls them in a loop with the gradients in between.  red: 4
// doubles of LDS, xs: kHmcDenseMaxDim doubles of LDS under a dense metric (else unused).
#pragma once
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
__device__ __forceinline__ void nuts_begin_chain(const HmcDev& D, const NutsDev& N, int64_t b, uint64_t seed, int64_t chain0, uint64_t transition,
                                                 double* red, double* xs)
{
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
// Returns the direction of the next leaf, 0 for a chain that is done.
template <bool Dense>
__device__ __forceinline__ int nuts_step_chain(const HmcDev& D, const NutsDev& N, int64_t b, uint64_t seed, int64_t chain0, uint64_t transition,
                                               int max_depth, int* active, double* red, double* xs)
{
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
    return vn;
}

// End of a transition: the proposal becomes the chain's state (position, gradient and ln target with it)
__device__ __forceinline__ void nuts_end_chain(const HmcDev& D, const NutsDev& N, int64_t b)
{
    const int64_t o = b * D.dim;
    for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
        const double q = N.qn[o + k];
        D.q[o + k] = q;
        D.grad[o + k] = N.gn[o + k];
        *hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]) = q;
    }
    if (threadIdx.x == 0) D.value[b] = N.lpn[b];
}

}  // namespace mcd
