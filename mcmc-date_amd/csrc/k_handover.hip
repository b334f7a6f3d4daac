// k_handover.hip -- the chains of one driver handle become those of another ON THE DEVICE (gfx950): mcd_hmc_take_state, mcd_mh_take_state and
// the Hamiltonian proposal attached to an mcd_mh_t (`maybeHamiltonianProposal`, app/Definitions.hs:272-278; mh_capi.cpp, hmc_capi.cpp).
//
//   k_handover    dst := src in one launch.  Workgroups [0, batch): one chain's two rows, lanes over the node index -- a wave loads and
//                 stores 512 contiguous bytes per 64 nodes, whatever the two handles' leading dimensions are; only the first n_nodes
//                 entries of a row are read or written.  The workgroups behind them: the scalars [5][batch], which lie alike in both
//                 handles, 256 consecutive doubles per workgroup.
//   k_ham_stats   the diagnostics of the transition a NutsDev holds, added into per-chain sums: one thread per chain.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "handover_device.hpp"

namespace mcd {

__global__ __launch_bounds__(256) void k_handover(ChainArrays dst, ChainArrays src, int64_t batch, int n_nodes)
{
    const int64_t blk = blockIdx.x;
    const int tid = threadIdx.x;
    if (blk < batch) {
        const double* __restrict__ sH = src.H + blk * src.ld;
        const double* __restrict__ sR = src.R + blk * src.ld;
        double* __restrict__ dH = dst.H + blk * dst.ld;
        double* __restrict__ dR = dst.R + blk * dst.ld;
        for (int w = tid; w < n_nodes; w += 256) {
            dH[w] = sH[w];
            dR[w] = sR[w];
        }
        return;
    }
    const int64_t i = (blk - batch) * 256 + tid;
    if (i < 5 * batch) dst.sc[i] = src.sc[i];
}

hipError_t launch_handover(const ChainArrays& dst, const ChainArrays& src, int64_t batch, int n_nodes, hipStream_t st)
{
    if (batch < 1 || n_nodes < 1 || dst.ld < n_nodes || src.ld < n_nodes) return hipErrorInvalidValue;
    const int64_t blocks = batch + (5 * batch + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_handover, dim3((unsigned)blocks), dim3(256), 0, st, dst, src, batch, n_nodes);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_ham_stats(NutsDev N, HamSums S, int64_t batch)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    const int na = N.n_alpha[b];
    S.alpha[b] += N.alpha[b] / (double)(na > 0 ? na : 1);            // the division mcd_hmc_nuts does on the host
    S.depth[b] += N.depth[b];
    S.leaves[b] += N.leaf[b];
    S.diverged[b] += N.diverged[b];
}

hipError_t launch_ham_stats(const NutsDev& N, const HamSums& S, int64_t batch, hipStream_t st)
{
    if (batch < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ham_stats, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, N, S, batch);
    return hipGetLastError();
}

}  // namespace mcd
