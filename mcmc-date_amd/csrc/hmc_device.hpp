// hmc_device.hpp -- the position layout and the ln target of the Hamiltonian side, for every kernel file that needs them (k_hmc.hip and
// k_nuts_chain.hip through leapfrog_device.hpp, k_nuts.hip and k_nuts_across.hip through nuts_device.hpp, k_hmc_record.hip): the
// gradient entry and the state slot of a coordinate, ln jacobianRootBranch, ln target.  The build contracts no multiply-add, so one
// expression here gives every caller the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mvn_kernels.h"

namespace mcd {

// d ln target / d q_i for chain b, from the outputs of the two gradient kernels + the Jacobian factor 1 / rootBranch,
// rootBranch = tH rMu (t_l r_l + t_r r_r)                                             (app/Probability.hs:393-410)
__device__ __forceinline__ double hmc_grad_entry(const HmcDev& D, int64_t b, int field, int v)
{
    const int64_t B = D.batch;
    const double* H = D.H + b * D.ld;
    const double* R = D.R + b * D.ld;
    const int l = 1, r = D.root_right;
    switch (field) {
        case 0: return D.gp_sc[0 * B + b];
        case 1: return D.gp_sc[1 * B + b];
        case 2: return D.gp_sc[2 * B + b] + D.gl_tH[b] - 1.0 / D.sc[2 * B + b];
        case 4: return D.gp_sc[3 * B + b] + D.gl_rMu[b] - 1.0 / D.sc[3 * B + b];
        case 5: return D.gp_sc[4 * B + b];
        default: break;
    }
    const double S = (H[0] - H[l]) * R[l] + (H[0] - H[r]) * R[r];
    if (field == 3) {
        double j = 0.0;
        if (v == l || v == r) j = R[v] / S;                       // d/d h_v of -ln S
        if (v == 0) j = -(R[l] + R[r]) / S;
        return D.gp_H[b * D.ld + v] + D.gl_H[b * D.ld + v] + j;
    }
    double j = 0.0;
    if (v == l || v == r) j = -(H[0] - H[v]) / S;
    return D.gp_R[b * D.ld + v] + D.gl_R[b * D.ld + v] + j;
}

__device__ __forceinline__ double* hmc_state_slot(const HmcDev& D, int64_t b, int field, int v)
{
    const int64_t B = D.batch;
    switch (field) {
        case 0: return D.sc + 0 * B + b;
        case 1: return D.sc + 1 * B + b;
        case 2: return D.sc + 2 * B + b;
        case 4: return D.sc + 3 * B + b;
        case 5: return D.sc + 4 * B + b;
        case 3: return D.H + b * D.ld + v;
        default: return D.R + b * D.ld + v;
    }
}

// ln jacobianRootBranch of chain b's state: the sample recorder keeps it on its own
__device__ __forceinline__ double hmc_ln_root_branch(const HmcDev& D, int64_t b)
{
    const double* H = D.H + b * D.ld;
    const double* R = D.R + b * D.ld;
    const int l = 1, r = D.root_right;
    const double root_branch = D.sc[2 * D.batch + b] * D.sc[3 * D.batch + b] * ((H[0] - H[l]) * R[l] + (H[0] - H[r]) * R[r]);
    return log(1.0 / root_branch);
}

// ln prior + ln likelihood + ln jacobianRootBranch (app/Hamiltonian.hs:85-92) once the two gradient kernels have run at the state
__device__ __forceinline__ double hmc_ln_target(const HmcDev& D, int64_t b) { return D.lp[b] + D.ll[b] + hmc_ln_root_branch(D, b); }

}  // namespace mcd
