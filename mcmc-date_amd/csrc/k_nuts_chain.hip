// k_nuts_chain.hip -- a whole NUTS transition, or n_steps leapfrog steps, of every chain in ONE launch (gfx950), for the trees whose
// likelihood is one 64-row block (MvnDev.R == 1: N <= 64, at most 66 nodes).  mcd_hmc_set_transition_form(MCD_HMC_TRANSITION_ONE_LAUNCH).
//
// The rounds form (hmc_capi.cpp: nuts_build) runs a leapfrog step of a tree as three launches -- k_prior_grad, k_tree_grad, k_nuts_step --
// with a counter cleared, copied back and waited for by the host around them.  Here one workgroup of 256 threads owns one chain from the
// momenta to the evaluation at the accepted point: the round loop is a counted loop of at most 2^max_depth iterations inside the kernel,
// left when the chain is done.  No workgroup reads what another one writes during the launch, so there is no flag, no poll and no
// fence beyond the workgroup's barriers: every array that passes from one phase to the next is re-read by the compute unit that stored it,
// behind a __syncthreads().
//
// The same bits as the rounds form with the substitution sweep as its likelihood gradient (what launch_tree_grad takes at R = 1 below 2048
// chains unless a form is forced), because no body exists twice and no sum depends on the launch geometry:
//   * begin / step / end of the tree building: nuts_chain_device.hpp, what k_nuts.hip's kernels call (256 threads per chain there too);
//   * the gradient of ln prior: prior_grad_device.hpp, what k_prior_grad calls; its closing sums are wave 0's, in lane order, for any
//     number of waves -- here waves 0 .. 2;
//   * the gradient of ln likelihood: wave 3 meanwhile, the steps of k_tree_grad<1, .., ..>'s compute wave -- load_tree<1, 1>, ONE
//     fwd_apply (R = 1: the factor is one chunk of 32 column pairs), finish_ll, the row scaling, ONE bwd_apply, tree_grad_tail
//     (mvn_device.hpp).  Ring, loader waves and prefetch depth of that kernel move bytes, not arithmetic: here the two factors (32 KiB
//     each, the layout they have in memory IS the chunk's layout in a ring slot) are staged into LDS once per launch;
//   * kick + drift, closing kick and collect: leapfrog_device.hpp, what k_hmc.hip's kernels call.
// The two roles meet at the workgroup barriers: prior_grad_chain holds kPriorGradBarriers of them, the likelihood wave arrives at as
// many of its own.
//
// LDS: 64 KiB of factors + (7 n_nodes + 2) doubles of the prior + n_nodes_pad doubles of the chain rule, dynamic and above 64 KiB
// (lds_optin.hpp); 4 KiB of xs under a dense metric and the small statics beside them: two workgroups share a compute unit.
#include "mvn_device.hpp"

#include "lds_optin.hpp"
#include "leapfrog_device.hpp"
#include "nuts_chain_device.hpp"
#include "prior_grad_device.hpp"

namespace mcd {

constexpr int kChainFactorD2 = 32 * 64;                      // a factor of R = 1: 32 column pairs x 64 lanes

// what the launch's dynamic LDS holds
struct ChainLds {
    d2 *ft, *ut;               // the forward and the backward factor, as a ring slot holds their one chunk
    double* sh;                // prior_grad_chain's 7 n_nodes + 2 doubles
    double* e;                 // tree_grad_tail's n_nodes_pad doubles
};
static size_t chain_lds_bytes(int n_nodes, int n_nodes_pad)
{
    return sizeof(d2) * 2 * kChainFactorD2 + sizeof(double) * (size_t)(7 * n_nodes + 2 + n_nodes_pad);
}

// the carve-up, and both factors from memory into their slots; every thread of the workgroup calls it, a barrier closes it
__device__ __forceinline__ ChainLds chain_lds_stage(d2* lds, const MvnDev& M, const PriorDev& P, bool factors)
{
    ChainLds L;
    L.ft = lds;
    L.ut = lds + kChainFactorD2;
    L.sh = reinterpret_cast<double*>(lds + 2 * kChainFactorD2);
    L.e = L.sh + 7 * P.n_nodes + 2;
    if (factors) {
        const d2* ft = reinterpret_cast<const d2*>(M.Ft);
        const d2* ut = reinterpret_cast<const d2*>(M.Ut);
        for (int i = threadIdx.x; i < kChainFactorD2; i += 256) {
            L.ft[i] = ft[i];
            L.ut[i] = ut[i];
        }
    }
    __syncthreads();
    return L;
}

// ln prior, ln likelihood and their gradients at chain b's state, into the arrays the gradient kernels write (D.lp, D.gp_*, D.ll, D.gl_*).
// Every thread of the workgroup calls it; it begins and ends with a barrier: the state the caller wrote is read, the outputs may be read.
__device__ __forceinline__ void chain_gradients(const HmcDev& D, const MvnDev& M, const TreeDev& T, const PriorDev& P, int64_t b, const ChainLds& L)
{
    const int64_t B = D.batch;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* tH = D.sc + 2 * B;
    double* rMu = D.sc + 3 * B;
    __syncthreads();
    if (wave < 3) {
        prior_grad_chain(P, D.sc, D.sc + B, tH, D.H, rMu, D.sc + 4 * B, D.R, D.ld, b, D.lp, D.gp_sc, D.gp_sc + B, D.gp_sc + 2 * B, D.gp_H,
                         D.gp_sc + 3 * B, D.gp_sc + 4 * B, D.gp_R, L.sh, tid, 192);
    } else {
        double d[1][1], dist[1][1];
        load_tree<1, 1>(d, dist, M, T, D.H, D.R, D.ld, tH, rMu, b, B, lane);
        fwd_apply<1, 1, 0, 0, 0>(d, L.ft, nullptr, lane);
        finish_ll<1, 1>(d, M, b, B, D.ll, lane);
        d[0][0] *= M.invdiag[lane];
        bwd_apply<1, 1, 0, 0>(d, L.ut, lane);
        tree_grad_tail<1>(d, dist, T, D.H, D.R, D.ld, tH, rMu, b, L.e, lane, D.gl_H, D.gl_R, D.gl_tH, D.gl_rMu);
        for (int i = 0; i < kPriorGradBarriers; ++i) __syncthreads();   // the barriers waves 0 .. 2 hold inside prior_grad_chain
    }
    __syncthreads();
}

// One transition of chain blockIdx.x: k_nuts_begin, then per round [ k_prior_grad | k_tree_grad ] and k_nuts_step, then k_nuts_end, the
// gradients at the accepted point and k_hmc_collect (hmc_capi.cpp: nuts_transition has the same sequence as launches).  active: the
// counter nuts_decide counts the chains that go on in; nobody reads it here.
template <bool Dense>
__global__ __launch_bounds__(256) void k_nuts_chain(HmcDev D, NutsDev N, MvnDev M, TreeDev T, PriorDev P, uint64_t seed, int64_t chain0,
                                                    uint64_t transition, int max_depth, int* active)
{
    extern __shared__ d2 chain_lds[];
    __shared__ double red[4];
    __shared__ double xs[Dense ? kHmcDenseMaxDim : 1];
    const int64_t b = blockIdx.x;
    const int64_t o = b * D.dim;
    const ChainLds L = chain_lds_stage(chain_lds, M, P, true);
    nuts_begin_chain<Dense>(D, N, b, seed, chain0, transition, red, xs);
    const int max_rounds = 1 << max_depth;                  // 2^max_depth - 1 leaves at most (max_depth <= 12: the host checks)
    for (int r = 0; r < max_rounds; ++r) {
        chain_gradients(D, M, T, P, b, L);
        if (!nuts_step_chain<Dense>(D, N, b, seed, chain0, transition, max_depth, active, red, xs)) break;   // workgroup-uniform
    }
    __syncthreads();
    nuts_end_chain(D, N, b);
    chain_gradients(D, M, T, P, b, L);
    for (int k = threadIdx.x; k < D.dim; k += blockDim.x) hmc_grad_collect_entry(D, o + k, b, k);
}

// n_steps leapfrog steps of chain blockIdx.x (mcd_hmc_leapfrog has the sequence): kick + drift with the kick 1/2 for step 0 and 1
// afterwards, then the gradients, n_steps times; the closing half kick with the collect.  n_steps == 0: the collect alone.
template <bool Dense>
__global__ __launch_bounds__(256) void k_leapfrog_chain(HmcDev D, MvnDev M, TreeDev T, PriorDev P, int n_steps)
{
    extern __shared__ d2 chain_lds[];
    __shared__ double xs[Dense ? kHmcDenseMaxDim : 1];
    const int64_t b = blockIdx.x;
    const int64_t o = b * D.dim;
    const ChainLds L = chain_lds_stage(chain_lds, M, P, n_steps > 0);
    for (int s = 0; s < n_steps; ++s) {
        hmc_kick_drift_chain<Dense>(D, b, (s == 0) ? 0.5 : 1.0, xs);
        chain_gradients(D, M, T, P, b, L);
    }
    for (int k = threadIdx.x; k < D.dim; k += blockDim.x) {
        if (n_steps > 0)
            hmc_kick_collect_entry(D, o + k, b, k, 0.5);
        else
            hmc_grad_collect_entry(D, o + k, b, k);
    }
}

template <auto Kernel, class... Args>
static hipError_t launch_chain(const HmcDev& D, const TreeDev& T, const PriorDev& P, hipStream_t st, Args... args)
{
    const size_t bytes = chain_lds_bytes(P.n_nodes, T.n_nodes_pad);
    if (hipError_t e = allow_dynamic_lds<Kernel>((int)chain_lds_bytes(kNutsChainMaxNodes, kNutsChainMaxNodes + 64))) return e;
    hipLaunchKernelGGL(Kernel, dim3((unsigned)D.batch), dim3(256), bytes, st, args...);
    return hipGetLastError();
}

bool nuts_chain_available(const MvnDev& M, const TreeDev& T, const PriorDev& P)
{
    return M.R == 1 && M.ncols == 64 && P.n_nodes == T.n_nodes && T.n_nodes <= kNutsChainMaxNodes && T.n_nodes_pad <= kNutsChainMaxNodes + 64;
}

hipError_t launch_nuts_chain(const HmcDev& D, const NutsDev& N, const MvnDev& M, const TreeDev& T, const PriorDev& P, uint64_t seed, int64_t chain0,
                             uint64_t transition, int max_depth, int* active, hipStream_t st)
{
    if (!nuts_chain_available(M, T, P) || max_depth < 1 || max_depth > 12) return hipErrorInvalidValue;
    if (D.metric) return launch_chain<k_nuts_chain<true>>(D, T, P, st, D, N, M, T, P, seed, chain0, transition, max_depth, active);
    return launch_chain<k_nuts_chain<false>>(D, T, P, st, D, N, M, T, P, seed, chain0, transition, max_depth, active);
}

hipError_t launch_leapfrog_chain(const HmcDev& D, const MvnDev& M, const TreeDev& T, const PriorDev& P, int n_steps, hipStream_t st)
{
    if (!nuts_chain_available(M, T, P) || n_steps < 0) return hipErrorInvalidValue;
    if (D.metric) return launch_chain<k_leapfrog_chain<true>>(D, T, P, st, D, M, T, P, n_steps);
    return launch_chain<k_leapfrog_chain<false>>(D, T, P, st, D, M, T, P, n_steps);
}

}  // namespace mcd
