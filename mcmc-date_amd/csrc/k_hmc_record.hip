// k_hmc_record.hip -- the sample recorder of the NUTS driver (mcd_hmc_record_*, hmc_capi.cpp) on the device (gfx950).
// The driver is host-driven (one launch per round of a transition, k_nuts.hip), so the recorder is one more launch at the end of a
// transition whose number is a multiple of the period: nothing here waits for anything, and nothing of the transition's kernels changes.
//
// A sample is the record of the Metropolis-Hastings driver's recorder (MhRec, mvn_kernels.h), so that the ring's readers -- k_mh_rec_unpack
// (k_mh.hip) and the ring front end of k_summary.hip -- serve both drivers: per chain heights [ld], rates [ld], then birth, death, tH, rMu,
// rVar, ln prior, ln likelihood, ln jacobianRootBranch, beta = 1, and in the seven doubles that are padding there the transition's
// diagnostics: tree depth, leapfrog steps, acceptance statistic, diverged flag, step size, joint0, 0.
//
//   k_hmc_record        one workgroup per chain, lanes over nodes (512 contiguous bytes per 64 nodes), the sixteen scalars by sixteen lanes
//   k_hmc_record_stats  the per-chain reductions of the diagnostics over a window of the ring (mcd_hmc_record_summary: nuts_stats)
//   k_hmc_moments       the position moments of mcd_hmc_nuts_run, summed in the order of the host loop they replace
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hmc_device.hpp"
#include "mvn_kernels.h"

namespace mcd {

__global__ __launch_bounds__(256) void k_hmc_record(HmcDev D, NutsDev N, MhRec R, int64_t sample)
{
    const int64_t b = blockIdx.x, B = D.batch;
    const int64_t slot = (sample - 1) % R.capacity;              // a ring; also the clamp: no store leaves the buffer (sample >= 1: the launcher)
    double* rec = R.base + (slot * B + b) * mh_rec_stride(D.ld);
    const double* H = D.H + b * D.ld;
    const double* Rt = D.R + b * D.ld;
    const int n = D.n_nodes, tid = threadIdx.x;
    for (int w = tid; w < n; w += 256) {
        rec[w] = H[w];
        rec[D.ld + w] = Rt[w];
    }
    if (tid >= 16) return;
    double v = 0.0;                                              // (15: the spare)
    if (tid < 5) {
        v = D.sc[tid * B + b];
    } else if (tid == 5) {
        v = D.lp[b];
    } else if (tid == 6) {
        v = D.ll[b];
    } else if (tid == 7) {                                       // the part of the ln target the kernels add (hmc_device.hpp)
        v = hmc_ln_root_branch(D, b);
    } else if (tid == 8) {
        v = 1.0;                                                 // beta: these chains are cold
    } else if (tid == 9) {
        v = (double)N.depth[b];
    } else if (tid == 10) {
        v = (double)N.leaf[b];
    } else if (tid == 11) {                                      // the division mcd_hmc_nuts does on the host
        const int na = N.n_alpha[b];
        v = N.alpha[b] / (double)(na > 0 ? na : 1);
    } else if (tid == 12) {
        v = (double)N.diverged[b];
    } else if (tid == 13) {
        v = D.eps[b];
    } else if (tid == 14) {
        v = N.joint0[b];
    }
    rec[2 * D.ld + tid] = v;
}

hipError_t launch_hmc_record(const HmcDev& D, const NutsDev& N, const MhRec& R, int64_t sample, hipStream_t st)
{
    if (R.base == nullptr || R.capacity < 1 || sample < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hmc_record, dim3((unsigned)D.batch), dim3(256), 0, st, D, N, R, sample);
    return hipGetLastError();
}

// one thread per chain; the counts are small integers, exact in fp64 whatever the order
__global__ __launch_bounds__(256) void k_hmc_record_stats(MhRecDims M, MhRec R, int64_t first, int64_t count, double* __restrict__ stats)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= M.batch) return;
    double div = 0.0, depth = 0.0, deepest = 0.0, leaves = 0.0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t slot = (first + i) % R.capacity;
        const double* t = R.base + (slot * M.batch + b) * mh_rec_stride(M.ld) + 2 * M.ld + 9;
        depth += t[0];
        deepest = fmax(deepest, t[0]);
        leaves += t[1];
        div += t[3];
    }
    stats[b * 4 + 0] = div;
    stats[b * 4 + 1] = depth / (double)count;
    stats[b * 4 + 2] = deepest;
    stats[b * 4 + 3] = leaves;
}

hipError_t launch_hmc_record_stats(const MhRecDims& S, const MhRec& R, int64_t first, int64_t count, double* stats, hipStream_t st)
{
    if (R.base == nullptr || R.capacity < 1 || count < 1 || first < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hmc_record_stats, dim3((unsigned)((S.batch + 255) / 256)), dim3(256), 0, st, S, R, first, count, stats);
    return hipGetLastError();
}

// one thread per coordinate, the chains in order: the sums of the host loop `for b: for k: s1[k] += x; s2[k] += x * x` to the bit (the
// build contracts no multiply-add); a wave's load of one chain is one contiguous row of q
__global__ __launch_bounds__(256) void k_hmc_moments(HmcDev D, double* __restrict__ s1, double* __restrict__ s2)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= D.dim) return;
    double a = s1[k], c = s2[k];
    for (int64_t b = 0; b < D.batch; ++b) {
        const double x = D.q[b * D.dim + k];
        a += x;
        c += x * x;
    }
    s1[k] = a;
    s2[k] = c;
}

hipError_t launch_hmc_moments(const HmcDev& D, double* s1, double* s2, hipStream_t st)
{
    hipLaunchKernelGGL(k_hmc_moments, dim3((unsigned)((D.dim + 255) / 256)), dim3(256), 0, st, D, s1, s2);
    return hipGetLastError();
}

}  // namespace mcd
