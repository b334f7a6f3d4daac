// nuts_device.hpp -- the NUTS state machine (Hoffman & Gelman's Algorithm 3 unrolled per chain, k_nuts.hip's header), written once for the
// kernels of both metric forms: k_nuts.hip (a workgroup per chain does everything) and k_nuts_across.hip (the dense metric's products taken
// out into k_metric_gemm.hip).  Here: the workgroup sum, the random streams, the start of a transition (nuts_tree_init, nuts_start), the
// booking of a new leaf (nuts_book_leaf) and the decision that follows it (nuts_decide).  What stays in the kernels is where the momenta,
// the kinetic energy and the U-turn products come from, and the loop over the stack levels a leaf opens and closes.  Every function is
// called by a whole workgroup (256 threads) of chain b under workgroup-uniform conditions: they hold barriers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hmc_device.hpp"
#include "mh_device.hpp"
#include "mvn_kernels.h"

namespace mcd {

constexpr double NUTS_DELTA_MAX = 1000.0;

__device__ __forceinline__ double nuts_block_sum(double v, double* red)
{
    v = mh_wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// the standard normal draw of coordinate k: a Box-Muller pair per draw 0x4000 + k / 2, cos for the even coordinate, sin for the odd one
__device__ __forceinline__ double nuts_normal(const Rng& g, int k)
{
    double ua, ub;
    philox_block(g, 0x4000u + (uint32_t)(k >> 1), ua, ub);
    const double rad = sqrt(-2.0 * log(ua)), ang = 6.28318530717958647692 * ub;
    return (k & 1) ? rad * sin(ang) : rad * cos(ang);
}

__device__ __forceinline__ int nuts_direction(const Rng& g, int j)
{
    double ua, ub;
    philox_block(g, 0x10u + 2u * (uint32_t)j, ua, ub);
    return ua < 0.5 ? -1 : 1;
}

// Start of a transition, entry `at` = (chain, coordinate): the tree is the current point with the momentum p
__device__ __forceinline__ void nuts_tree_init(const HmcDev& D, const NutsDev& N, int64_t at, double p)
{
    const double q = D.q[at], gr = D.grad[at];
    N.qm[at] = q;
    N.qp[at] = q;
    N.pm[at] = p;
    N.pp[at] = p;
    N.gm[at] = gr;
    N.gp[at] = gr;
    N.qn[at] = q;
    N.gn[at] = gr;
}

// Start of a transition, chain b with the kinetic energy `kin` of its momenta: joint0, the slice variable (draw 1), the chain's fields.
// Returns the direction of doubling 0.
__device__ __forceinline__ int nuts_start(const HmcDev& D, const NutsDev& N, int64_t b, const Rng& g, double kin)
{
    const double joint0 = D.value[b] - kin;
    double us, ub2;
    philox_block(g, 1u, us, ub2);
    const int v = nuts_direction(g, 0);
    if (threadIdx.x == 0) {
        N.joint0[b] = joint0;
        N.log_u[b] = joint0 + log(us);
        N.lpn[b] = D.value[b];
        N.alpha[b] = 0.0;
        N.n_alpha[b] = 0;
        N.n[b] = 1;
        N.n1[b] = 0;
        N.s1[b] = 1;
        N.j[b] = 0;
        N.v[b] = v;
        N.i[b] = 0;
        N.leaf[b] = 0;
        N.depth[b] = 0;
        N.done[b] = 0;
        N.diverged[b] = 0;
    }
    return v;
}

// what the booking of a leaf leaves for the decision: admissible leaves of the sub tree, the leaf's number, "the sub tree goes on"
struct NutsLeaf {
    int n1, leaf;
    bool s1;
};

// The new leaf (position eq, gradient eg, ln target lp, kinetic energy kin) is booked: slice test, divergence flag, the uniform draw
// among the admissible leaves of the sub tree (reservoir, draw 0x100000 + leaf), the acceptance statistic.
__device__ __forceinline__ NutsLeaf nuts_book_leaf(const HmcDev& D, const NutsDev& N, int64_t b, const Rng& g, double lp, double kin, const double* eq,
                                                   const double* eg)
{
    const int64_t o = b * D.dim;
    double joint = lp - kin;
    if (!isfinite(joint)) joint = -INFINITY;                        // left the support / diverged: not admissible
    const double log_u = N.log_u[b];
    const bool nl = log_u <= joint;
    const bool sl = log_u < NUTS_DELTA_MAX + joint;
    const int n1 = N.n1[b] + (nl ? 1 : 0);
    const bool s1 = N.s1[b] != 0 && sl;
    if (!sl && threadIdx.x == 0) N.diverged[b] = 1;                 // what the sample recorder reports (k_hmc_record.hip)
    const int leaf = N.leaf[b];
    if (nl) {                                                       // reservoir over the admissible leaves of the sub tree
        double ua, ub;
        philox_block(g, 0x100000u + (uint32_t)leaf, ua, ub);
        if (ua * (double)n1 < 1.0) {
            for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
                N.qc[o + k] = eq[k];
                N.gc[o + k] = eg[k];
            }
            if (threadIdx.x == 0) N.lpc[b] = lp;
        }
    }
    if (threadIdx.x == 0) {
        const double d = joint - N.joint0[b];
        N.alpha[b] += fmin(1.0, exp(fmin(0.0, d)));
        N.n_alpha[b] += 1;
    }
    return {n1, leaf, s1};
}

// The decision after leaf i of doubling j in direction v, once the sub trees the leaf closes have been tested (L.s1; a barrier lies behind):
// abandon the sub tree, or -- it is complete -- the biased progressive choice (draw 0x11 + 2 j) and `no_u_turn()` of the whole tree, called
// under exactly these conditions, then the depth stop; the chain's fields are written back.  A chain that goes on counts itself in `active`
// and, where `list` is not null, lists itself there (at most batch entries: one per chain).  Returns the direction of the next leaf, 0 for
// a chain that is done.
template <class NoUTurn>
__device__ __forceinline__ int nuts_decide(const HmcDev& D, const NutsDev& N, int64_t b, const Rng& g, int max_depth, int v, int j, int i, NutsLeaf L,
                                           NoUTurn no_u_turn, int* active, int* list)
{
    __shared__ int flag;
    const int64_t o = b * D.dim;
    int done = 0, jn = j, vn = v, in_ = i + 1, n = N.n[b], n1 = L.n1;
    if (!L.s1) {
        done = 1;                                                   // the sub tree is abandoned, the proposal stays
        jn = j + 1;
    } else if (in_ == (1 << j)) {                                   // sub tree complete
        double ua, ub;
        philox_block(g, 0x11u + 2u * (uint32_t)j, ua, ub);
        if (n1 > 0 && ua * (double)n < (double)n1) {
            for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
                N.qn[o + k] = N.qc[o + k];
                N.gn[o + k] = N.gc[o + k];
            }
            if (threadIdx.x == 0) N.lpn[b] = N.lpc[b];
        }
        n += n1;
        __syncthreads();
        const bool s = no_u_turn();
        jn = j + 1;
        if (!s || jn >= max_depth) {
            done = 1;
        } else {
            vn = nuts_direction(g, jn);
            in_ = 0;
            n1 = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        N.n[b] = n;
        N.n1[b] = n1;
        N.s1[b] = L.s1 ? 1 : 0;
        N.j[b] = jn;
        N.v[b] = vn;
        N.i[b] = in_;
        N.leaf[b] = L.leaf + 1;
        N.done[b] = done;
        N.depth[b] = jn;
        if (!done) {
            const int at = atomicAdd(active, 1);
            if (list) list[at] = (int)b;
        }
        flag = done;
    }
    __syncthreads();
    return flag ? 0 : vn;
}

}  // namespace mcd
