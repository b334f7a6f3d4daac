// k_prior_grad.hip -- gradient of the log prior with respect to the state (gfx950): the kernel of its own and its launcher.  The
// mapping, the dual numbers and the body of a chain's workgroup are prior_grad_device.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lds_optin.hpp"

#include "mvn_kernels.h"
#include "prior_grad_device.hpp"

namespace mcd {

__global__ void __launch_bounds__(256, 2) k_prior_grad(PriorDev P, const double* __restrict__ birth, const double* __restrict__ death,
                                                    const double* __restrict__ tH, const double* __restrict__ H,
                                                    const double* __restrict__ rMu, const double* __restrict__ rVar,
                                                    const double* __restrict__ Rt, int64_t lds, int64_t batch,
                                                    double* __restrict__ lp, double* __restrict__ g_birth,
                                                    double* __restrict__ g_death, double* __restrict__ g_tH,
                                                    double* __restrict__ g_H, double* __restrict__ g_rMu,
                                                    double* __restrict__ g_rVar, double* __restrict__ g_R)
{
    extern __shared__ double sh[];
    prior_grad_chain(P, birth, death, tH, H, rMu, rVar, Rt, lds, blockIdx.x, lp, g_birth, g_death, g_tH, g_H, g_rMu, g_rVar, g_R, sh,
                     (int)threadIdx.x, (int)blockDim.x);
}

hipError_t launch_prior_grad(const PriorDev& P, const double* birth, const double* death, const double* tH, const double* H,
                             const double* rMu, const double* rVar, const double* Rt, int64_t lds, int64_t batch, double* lp,
                             double* g_birth, double* g_death, double* g_tH, double* g_H, double* g_rMu, double* g_rVar, double* g_R,
                             hipStream_t st)
{
    if (batch <= 0) return hipSuccess;
    if (P.n_nodes > kPriorGradMaxNodes) return hipErrorInvalidValue;      // (mcd_prior_grad_batch and mcd_hmc_create* refuse by the same constant)
    const size_t bytes = sizeof(double) * (7 * (size_t)P.n_nodes + 2);
    if (bytes > 64 * 1024)                                   // more than 64 KiB of LDS (from 1170 nodes) has to be allowed once per device
        if (hipError_t e = allow_dynamic_lds<k_prior_grad>((int)(sizeof(double) * (7 * (size_t)kPriorGradMaxNodes + 2)))) return e;
    // waves per chain: as many as the tree has 64-node slices (at most 4) while the whole batch is resident at once (2 waves
    // per SIMD: 2048 on the chip); beyond that more waves per chain only add rounds (4096 chains x 255 nodes: 115 us with one
    // wave per chain, 143 with four)
    int waves = (P.n_nodes + 63) / 64;
    const int64_t fit = 2048 / batch;
    waves = waves > 4 ? 4 : waves;
    waves = waves > fit ? (int)fit : waves;
    waves = waves < 1 ? 1 : waves;
    hipLaunchKernelGGL(k_prior_grad, dim3((unsigned)batch), dim3(64 * waves), bytes, st, P, birth, death, tH, H, rMu, rVar, Rt, lds, batch, lp,
                       g_birth, g_death, g_tH, g_H, g_rMu, g_rVar, g_R);
    return hipGetLastError();
}

}  // namespace mcd
