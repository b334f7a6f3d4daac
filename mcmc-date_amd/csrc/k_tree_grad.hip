// k_tree_grad.hip -- tree state -> log-likelihood + gradient wrt the state (gfx950).  Device code: mvn_device.hpp.
#include "mvn_device.hpp"

namespace mcd {

// Both sweeps, then the chain rule from g = d ll / d distances back to heights, rates, tH, rMu (tree_grad_tail, mvn_device.hpp).  One
// chain per compute wave; e[v] = s * g[row(v)] * rate[v] is exchanged through the (by then idle) LDS ring, one private
// region per wave.
template <int R, int CW, int LW>
__global__ void __launch_bounds__(64 * (CW + LW)) k_tree_grad(MvnDev M, TreeDev T, const double* __restrict__ H,
                                                              const double* __restrict__ Rt, int64_t lds,
                                                              const double* __restrict__ tH,
                                                              const double* __restrict__ rMu, int64_t batch,
                                                              double* __restrict__ ll, double* __restrict__ gH,
                                                              double* __restrict__ gR, double* __restrict__ gtH,
                                                              double* __restrict__ grMu)
{
    constexpr int BT = 1;
    MCD_KERNEL_HEAD
    MCD_ACC_DECL
    if (wave >= CW) {                                      // loader role
        Stage<R, LW> st;
        const int lw = wave - CW;
        fwd_loader_prologue<R, LW>(M.Ft, ring, st, lw, lane);
        lds_barrier();
        fwd_loader_start<R, LW>(M.Ft, st, lw, lane);
        fwd_loader<R, LW, 0>(M.Ft, ring, st, lw, lane, ncols MCD_ACC_ARGS);
        bool started = false;
        bwd_loader<R, LW, R - 1>(M.Ut, ring, st, lw, lane, ncols, started);
        return;
    }
    double d[R][1], dist[R][1];
    load_tree<R, 1>(d, dist, M, T, H, Rt, lds, tH, rMu, b0, batch, lane);
    lds_barrier();
    fwd_compute<R, 1, 0>(d, ring, lane, ncols MCD_ACC_ARGS);
    finish_ll<R, 1>(d, M, b0, batch, ll, lane);
#pragma unroll
    for (int k = 0; k < R; ++k) d[k][0] *= M.invdiag[64 * k + lane];
    {
        bool started = false;
        bwd_compute<R, 1, R - 1>(d, ring, lane, ncols, started);
    }
    // now d = y = Sigma^-1 (dist - mu); g = -y.  The last barrier of the sweep has passed: the ring
    // is free.  n_nodes_pad <= 64 R + 64 doubles per compute wave fit in it (CW * 8.5 KiB <= 64 KiB).
    if (b0 >= batch) return;               // no barriers below
    tree_grad_tail<R>(d, dist, T, H, Rt, lds, tH, rMu, b0, reinterpret_cast<double*>(ring) + (size_t)wave * T.n_nodes_pad, lane, gH, gR, gtH, grMu);
}

template <int R>
static hipError_t launch_tree_grad_R(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds,
                                     const double* tH, const double* rMu, int64_t batch, double* ll, double* gH,
                                     double* gR, double* gtH, double* grMu, hipStream_t st)
{
    grad_launch_geometry<R>(batch, [&](auto cw_tag) {
        constexpr int CW = decltype(cw_tag)::value, LW = grad_loader_waves(R);
        const unsigned grid = (unsigned)((batch + CW - 1) / CW);
        hipLaunchKernelGGL((k_tree_grad<R, CW, LW>), dim3(grid), dim3(64 * (CW + LW)), 0, st, M, T, H, Rt, lds, tH, rMu, batch,
                       ll, gH, gR, gtH, grMu);
    });
    return hipGetLastError();
}

// the sweep of this compile's R group (sweep_groups.hpp; R = 16 has none: launch_tree_grad, sweep_launch.cpp)
hipError_t MCD_CAT(launch_tree_grad_g, MCD_RGROUP)(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds,
                                                   const double* tH, const double* rMu, int64_t batch, double* ll, double* gH, double* gR,
                                                   double* gtH, double* grMu, hipStream_t st)
{
#define CALL(R) launch_tree_grad_R<R>(M, T, H, Rt, lds, tH, rMu, batch, ll, gH, gR, gtH, grMu, st)
    MCD_DISPATCH_R(M.R, CALL)
#undef CALL
}

}  // namespace mcd
