// k_nuts_across.hip -- the device NUTS (k_nuts.hip) under a dense metric in the across-chains form (mcd_hmc_set_metric_form): k_nuts_begin
// and k_nuts_step split at the products with C and U^-1, which leave the chain's workgroup and become rows of k_metric_gemm.hip's one
// product over the lock-step chains.  Random streams, start of a transition, booking of a leaf and the decision are the functions of
// nuts_device.hpp that k_nuts.hip calls too (nuts_normal, nuts_tree_init, nuts_start, nuts_book_leaf, nuts_decide); here is only where a
// product's numbers come from, and the stack levels opened in k_nutsx_leaf and closed in k_nutsx_book.  One transition (hmc_capi.cpp):
//
//     k_nutsx_draw           Z = the normal draws 0x4000 + k / 2                           (one thread per chain and coordinate)
//     gemm (lower)           P = Z U^-1 rows, i.e. p = U^-T z
//     gemm                   CP = P C
//     k_nutsx_begin          kin = 1/2 p . Cp, joint0, slice, the tree = the current point; the first edge's half-kicked momentum -> D.p
//     gemm                   Y = D.p C
//     k_nutsx_drift          q = edge + eps v Y -> D.q and the state arrays
//   per round, after the gradient kernels:
//     k_nutsx_leaf      (a)  second half kick, the leaf becomes the edge, opens its stack levels, writes the round's right-hand sides
//     gemm              (b)  all of them at once: nuts_rhs_plan(j, i).count x (chains still building) rows
//     k_nutsx_book      (c)  kinetic energy, joint, booking, reservoir, U-turn dots and the decision; next edge's half-kicked momentum
//     gemm              (d)  Y = D.p C
//     k_nutsx_drift     (e)
//
// Chains that have finished leave the products: k_nutsx_book appends every chain that goes on to an index list (in whatever order the
// workgroups arrive: a row of a product depends on that row only, not on its place), the host reads their number with the counter it
// polls anyway, and the products (d), (b) of the next round multiply the listed chains' rows only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mh_device.hpp"
#include "mvn_kernels.h"
#include "nuts_device.hpp"
#include "nuts_rhs_plan.hpp"

namespace mcd {

static_assert(kNutsRhsMaxSlots == 13, "one slot for the leaf, one per stack level below the top, one for the whole tree");

__global__ __launch_bounds__(256) void k_nutsx_draw(HmcDev D, double* __restrict__ Z, uint64_t seed, int64_t chain0, uint64_t transition)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D.batch * D.dim) return;
    const int64_t b = i / D.dim;
    const int k = (int)(i - b * D.dim);
    Z[i] = nuts_normal(mh_rng(seed, chain0 + b, transition), k);
}

// the edge that is extended next: its half-kicked momentum goes to D.p (the right-hand side of the drift's product), its gradient to D.grad
__device__ __forceinline__ void nutsx_next_edge(const HmcDev& D, const NutsDev& N, int64_t b, int v)
{
    const int64_t o = b * D.dim;
    const double* ep = (v < 0 ? N.pm : N.pp) + o;
    const double* eg = (v < 0 ? N.gm : N.gp) + o;
    const double e = D.eps[b] * (double)v;
    for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
        const double g = eg[k];
        D.p[o + k] = ep[k] + 0.5 * e * g;                           // p += eps / 2 grad
        D.grad[o + k] = g;
    }
    if (threadIdx.x == 0) const_cast<double*>(D.dir)[b] = (double)v;
}

// Start of a transition after the momenta: P = U^-T z and CP = C p of every chain are there.  A workgroup per chain.
__global__ __launch_bounds__(256) void k_nutsx_begin(HmcDev D, NutsDev N, const double* __restrict__ P, const double* __restrict__ CP, uint64_t seed,
                                                     int64_t chain0, uint64_t transition)
{
    __shared__ double red[4];
    const int64_t b = blockIdx.x;
    const int64_t o = b * D.dim;
    double kin = 0.0;
    for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
        const double p = P[o + k];
        kin += p * CP[o + k];
        nuts_tree_init(D, N, o + k, p);
    }
    kin = 0.5 * nuts_block_sum(kin, red);
    const int v = nuts_start(D, N, b, mh_rng(seed, chain0 + b, transition), kin);
    __syncthreads();
    nutsx_next_edge(D, N, b, v);
}

// q = edge + eps v (C p), Y = the product of the half-kicked momenta; new position into D.q and the state arrays.  Chains that have
// finished keep their state.  One thread per (chain, coordinate).
__global__ __launch_bounds__(256) void k_nutsx_drift(HmcDev D, NutsDev N, const double* __restrict__ Y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D.batch * D.dim) return;
    const int64_t b = i / D.dim;
    if (N.done[b]) return;
    const int k = (int)(i - b * D.dim);
    const int v = N.v[b];
    const double e = D.eps[b] * (double)v;
    const double q = (v < 0 ? N.qm : N.qp)[i] + e * Y[i];            // q += eps (C p)
    D.q[i] = q;
    *hmc_state_slot(D, b, D.pos_field[k], D.pos_index[k]) = q;
}

// (a) of a round: the gradient kernels have run at the position the drift reached.  Second half kick; the leaf becomes the tree's edge and
// the first leaf of the stack levels it opens; the round's right-hand sides go to X (nuts_rhs_plan.hpp).  Everything is elementwise in the
// coordinate: one thread per (chain, coordinate).
__global__ __launch_bounds__(256) void k_nutsx_leaf(HmcDev D, NutsDev N, double* __restrict__ X)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= D.batch * D.dim) return;
    const int64_t b = t / D.dim;
    if (N.done[b]) return;
    const int k = (int)(t - b * D.dim);
    const int64_t B = D.batch;
    const int v = N.v[b], j = N.j[b], i = N.i[b];
    const double e = D.eps[b] * (double)v;
    const double g = hmc_grad_entry(D, b, D.pos_field[k], D.pos_index[k]);
    const double p = D.p[t] + 0.5 * e * g;
    const double q = D.q[t];
    (v < 0 ? N.qm : N.qp)[t] = q;
    (v < 0 ? N.pm : N.pp)[t] = p;
    (v < 0 ? N.gm : N.gp)[t] = g;
    const NutsRhsPlan plan = nuts_rhs_plan(j, i);
    X[t] = p;                                                        // slot 0: the leaf's momentum
    for (int lvl = 1; lvl <= j; ++lvl) {
        const int size = 1 << lvl;
        const int64_t at = ((int64_t)b * N.max_depth + (lvl - 1)) * D.dim + k;
        if ((i & (size - 1)) == 0) {
            N.sq[at] = q;
            N.sp[at] = p;
        } else if (lvl <= plan.closes) {
            // q+ - q- in time order: going forwards the first leaf is the minus end, going backwards the plus end
            const double lq = N.sq[at];
            X[((int64_t)lvl * B + b) * D.dim + k] = v > 0 ? q - lq : lq - q;
        }
    }
    if (plan.whole) X[((int64_t)(plan.closes + 1) * B + b) * D.dim + k] = v > 0 ? q - N.qm[t] : N.qp[t] - q;
}

// w . rm >= 0 and w . rp >= 0, w = C (q+ - q-) from the round's product
__device__ __forceinline__ bool nutsx_no_u_turn(int dim, const double* w, const double* rm, const double* rp, double* red)
{
    double a = 0.0, c = 0.0;
    for (int k = threadIdx.x; k < dim; k += blockDim.x) {
        a += w[k] * rm[k];
        c += w[k] * rp[k];
    }
    a = nuts_block_sum(a, red);
    c = nuts_block_sum(c, red);
    return a >= 0.0 && c >= 0.0;
}

// (c) of a round: Y holds the products of the right-hand sides k_nutsx_leaf wrote.  Book the leaf, decide, and prepare the next leaf -- or
// mark the chain done.  A workgroup per chain; k_nuts_step's round (nuts_book_leaf, nuts_decide: nuts_device.hpp) with the products read from Y.
__global__ __launch_bounds__(256) void k_nutsx_book(HmcDev D, NutsDev N, const double* __restrict__ Y, uint64_t seed, int64_t chain0, uint64_t transition,
                                                    int max_depth, int* __restrict__ active, int* __restrict__ list)
{
    __shared__ double red[4];
    const int64_t b = blockIdx.x;
    if (N.done[b]) return;                                          // workgroup-uniform
    const int64_t o = b * D.dim, B = D.batch;
    const Rng rng = mh_rng(seed, chain0 + b, transition);
    const int v = N.v[b], j = N.j[b], i = N.i[b];
    const double* eq = (v < 0 ? N.qm : N.qp) + o;
    const double* ep = (v < 0 ? N.pm : N.pp) + o;
    const double* eg = (v < 0 ? N.gm : N.gp) + o;
    const NutsRhsPlan plan = nuts_rhs_plan(j, i);
    double kin = 0.0;                                               // 1/2 p^T C p
    for (int k = threadIdx.x; k < D.dim; k += blockDim.x) kin += ep[k] * Y[o + k];
    kin = 0.5 * nuts_block_sum(kin, red);
    NutsLeaf L = nuts_book_leaf(D, N, b, rng, hmc_ln_target(D, b), kin, eq, eg);
    // ---- the aligned sub trees the leaf closes, smallest first
    for (int lvl = 1; lvl <= plan.closes; ++lvl) {
        if (!L.s1) break;
        const double* lr = N.sp + ((int64_t)b * N.max_depth + (lvl - 1)) * D.dim;
        const double* w = Y + ((int64_t)lvl * B + b) * D.dim;
        const bool ok = v > 0 ? nutsx_no_u_turn(D.dim, w, lr, ep, red) : nutsx_no_u_turn(D.dim, w, ep, lr, red);
        L.s1 = L.s1 && ok;
    }
    __syncthreads();
    const int vn = nuts_decide(D, N, b, rng, max_depth, v, j, i, L,
                               [&] { return nutsx_no_u_turn(D.dim, Y + ((int64_t)(plan.closes + 1) * B + b) * D.dim, N.pm + o, N.pp + o, red); }, active, list);
    if (vn) nutsx_next_edge(D, N, b, vn);
}

static unsigned nutsx_grid(const HmcDev& D) { return (unsigned)((D.batch * D.dim + 255) / 256); }

hipError_t launch_nutsx_draw(const HmcDev& D, double* Z, uint64_t seed, int64_t chain0, uint64_t transition, hipStream_t st)
{
    hipLaunchKernelGGL(k_nutsx_draw, dim3(nutsx_grid(D)), dim3(256), 0, st, D, Z, seed, chain0, transition);
    return hipGetLastError();
}
hipError_t launch_nutsx_begin(const HmcDev& D, const NutsDev& N, const double* P, const double* CP, uint64_t seed, int64_t chain0, uint64_t transition,
                              hipStream_t st)
{
    hipLaunchKernelGGL(k_nutsx_begin, dim3((unsigned)D.batch), dim3(256), 0, st, D, N, P, CP, seed, chain0, transition);
    return hipGetLastError();
}
hipError_t launch_nutsx_drift(const HmcDev& D, const NutsDev& N, const double* Y, hipStream_t st)
{
    hipLaunchKernelGGL(k_nutsx_drift, dim3(nutsx_grid(D)), dim3(256), 0, st, D, N, Y);
    return hipGetLastError();
}
hipError_t launch_nutsx_leaf(const HmcDev& D, const NutsDev& N, double* X, hipStream_t st)
{
    hipLaunchKernelGGL(k_nutsx_leaf, dim3(nutsx_grid(D)), dim3(256), 0, st, D, N, X);
    return hipGetLastError();
}
hipError_t launch_nutsx_book(const HmcDev& D, const NutsDev& N, const double* Y, uint64_t seed, int64_t chain0, uint64_t transition, int max_depth,
                             int* active, int* list, hipStream_t st)
{
    hipLaunchKernelGGL(k_nutsx_book, dim3((unsigned)D.batch), dim3(256), 0, st, D, N, Y, seed, chain0, transition, max_depth, active, list);
    return hipGetLastError();
}

}  // namespace mcd
