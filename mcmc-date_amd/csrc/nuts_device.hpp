// nuts_device.hpp -- device helpers shared by the NUTS kernels (k_nuts.hip: a workgroup per chain does everything; k_nuts_across.hip: the
// dense metric's products taken out into k_metric_gemm.hip): workgroup sum, gradient entry, state slot, direction draw.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

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

// the entries of k_hmc.hip's hmc_grad_entry / hmc_state_slot, needed here as well
__device__ __forceinline__ double nuts_grad_entry(const HmcDev& D, int64_t b, int field, int v)
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
        if (v == l || v == r) j = R[v] / S;
        if (v == 0) j = -(R[l] + R[r]) / S;
        return D.gp_H[b * D.ld + v] + D.gl_H[b * D.ld + v] + j;
    }
    double j = 0.0;
    if (v == l || v == r) j = -(H[0] - H[v]) / S;
    return D.gp_R[b * D.ld + v] + D.gl_R[b * D.ld + v] + j;
}

__device__ __forceinline__ double* nuts_state_slot(const HmcDev& D, int64_t b, int field, int v)
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

__device__ __forceinline__ int nuts_direction(uint64_t seed, int64_t chain, uint64_t transition, int j)
{
    double ua, ub;
    philox_block(mh_rng(seed, chain, transition), 0x10u + 2u * (uint32_t)j, ua, ub);
    return ua < 0.5 ? -1 : 1;
}

}  // namespace mcd
