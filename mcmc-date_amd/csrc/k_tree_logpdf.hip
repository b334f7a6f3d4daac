// k_tree_logpdf.hip -- tree state -> log-likelihood (+ root-branch Jacobian) (gfx950).  Device code: mvn_device.hpp.
//
// PRIOR variant (the two-launch Metropolis-Hastings step, mh_capi.cpp): the first J.n_wgs workgroups do not sweep -- each of
// their waves evaluates the ln prior of one chain's proposed state (mh_prior_role.hpp), which depends on the proposal only,
// like the likelihood the other workgroups compute: a lock step then costs accept + propose + max(likelihood, prior) instead of
// their sum.  The plain variant is what every other caller launches; its code is unchanged.
#define MCD_BID (blockIdx.x - bid_off)
#include "mvn_device.hpp"
#include "mh_prior_role.hpp"
#include <type_traits>

namespace mcd {

struct MhPriorJob {
    MhDev M;
    PriorDev P;
    int n_wgs;
    int wpc;       // waves per chain: 1, or 2 (mh_prior_role2)
};
struct NoJob {};

// The leading arguments are scalars and pointers only, in the order the likelihood role's first memory instructions need them, as
// far as the preloaded SGPRs reach (k_logpdf.hip): the factor stream for the loaders, the chain's state rows and the node count for
// the compute waves, then the slot tables, mu and 1/diag.  The prior variant reads J.n_wgs before it knows a wave's role, by a
// scalar load as before.  F: the stream FS reads (fwd_stream_ptr).
template <int R, int BT, int CW, int LW, bool PRIOR, int FS>
__global__ void __launch_bounds__(64 * (CW + LW)) k_tree_logpdf(const double* __restrict__ F, const double* __restrict__ H,
                                                                const double* __restrict__ Rt, int64_t lds, int64_t batch, int n_nodes,
                                                                int root_right, const int32_t* __restrict__ slot_node,
                                                                const int32_t* __restrict__ slot_parent, const double* __restrict__ mu,
                                                                const double* __restrict__ invdiag, const double* __restrict__ tH,
                                                                const double* __restrict__ rMu, int ncols, double* __restrict__ ll,
                                                                double* __restrict__ logjac, double c, double logdet,
                                                                std::conditional_t<PRIOR, MhPriorJob, NoJob> J)
{
    unsigned bid_off = 0;
    if constexpr (PRIOR) bid_off = (unsigned)J.n_wgs;
    MCD_KERNEL_HEAD_FS(FS)
    if constexpr (PRIOR) {
        if (blockIdx.x < bid_off) {                        // the prior role: a chain per wave (or per two), its state in a slice of the ring
            if (J.wpc == 2) {
                const int64_t pb = (int64_t)blockIdx.x * ((CW + LW) / 2) + (wave >> 1);
                const bool valid = pb < J.M.batch;
                mh_prior_role2(J.M, J.P, valid ? pb : J.M.batch - 1, valid, wave & 1, lane,
                               reinterpret_cast<double*>(ring) + (size_t)(wave >> 1) * mh_prior_role2_doubles(J.M.n_nodes));
                return;
            }
            const int64_t pb = (int64_t)blockIdx.x * (CW + LW) + wave;
            if (pb >= J.M.batch) return;
            double* hs = reinterpret_cast<double*>(ring) + (size_t)wave * 2 * J.M.n_nodes;
            mh_prior_role(J.M, J.P, pb, lane, hs, hs + J.M.n_nodes);
            return;
        }
    }
    MCD_ACC_DECL
    if (wave >= CW) {                                      // loader role
        fwd_loader_role<R, LW, FS>(F, ring, wave - CW, lane, ncols MCD_ACC_ARGS);
        return;
    }
    const MvnView M(mu, invdiag, 0, c, logdet);
    const TreeView T(n_nodes, root_right, slot_node, slot_parent);
    double d[R][BT], dist[R][BT];
    // a sampler's batch (two compute waves per workgroup) on trees up to 258 nodes: the state rows go through LDS (10 KiB beside
    // the ring: two workgroups still fit a CU); elsewhere the gather from global memory
    constexpr bool STAGED = (R <= 4 && BT == 1 && CW == 2);
    __shared__ double tstage[STAGED ? CW * 2 * (64 * R + 64) : 1];
    if constexpr (STAGED)
        load_tree_staged<R>(d, dist, M, T, H, Rt, lds, tH, rMu, b0, batch, lane, tstage + (size_t)wave * 2 * (64 * R + 64));
    else
        load_tree<R, BT>(d, dist, M, T, H, Rt, lds, tH, rMu, b0, batch, lane);
    if (logjac != nullptr && lane == 0) {
#pragma unroll
        for (int c = 0; c < BT; ++c)
            if (b0 + c < batch) logjac[b0 + c] = log(1.0 / dist[0][c]);  // app/Probability.hs:394, 409
    }
    lds_barrier();
    fwd_compute<R, BT, 0, FS>(d, ring, lane, ncols MCD_ACC_ARGS);
    finish_ll<R, BT>(d, M, b0, batch, ll, lane);
}

// one launch of k_tree_logpdf<R, BT, CW, LW, PRIOR, FS> with FS the forward stream in force (fwd_stream); the prior variant (the
// Metropolis-Hastings step's likelihood launch) keeps the padded stream whatever MCD_FSTREAM says: its workgroups of both roles share
// CUs two by two, which the LDS-DMA ring's four slots would not leave room for, and the compact stream staged through registers
// measured no gain on the sweep
template <int R, int BT, int CW, int LW, bool PRIOR, int FS, class JOB>
static void launch_tree_fs_k(unsigned grid, hipStream_t st, const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds,
                             const double* tH, const double* rMu, int64_t batch, double* ll, double* logjac, const JOB& J)
{
    hipLaunchKernelGGL((k_tree_logpdf<R, BT, CW, LW, PRIOR, FS>), dim3(grid), dim3(64 * (CW + LW)), 0, st, fwd_stream_ptr(M, FS), H, Rt, lds,
                       batch, T.n_nodes, T.root_right, T.slot_node, T.slot_parent, M.mu, M.invdiag, tH, rMu, M.ncols, ll, logjac, M.c, M.logdet, J);
}

template <int R, int BT, int CW, int LW, bool PRIOR, class... A>
static void launch_tree_fs(unsigned grid, hipStream_t st, const A&... a)
{
    if constexpr (fwd_stream_compact(R) && !PRIOR) {
        const int fs = fwd_stream<R>(CW);
        if (fs == 1) return launch_tree_fs_k<R, BT, CW, LW, PRIOR, 1>(grid, st, a...);
        if (fs == 2) return launch_tree_fs_k<R, BT, CW, LW, PRIOR, 2>(grid, st, a...);
    }
    launch_tree_fs_k<R, BT, CW, LW, PRIOR, 0>(grid, st, a...);
}

template <int R, bool PRIOR, class JOB>
static hipError_t launch_tree_logpdf_R(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds,
                                       const double* tH, const double* rMu, int64_t batch, double* ll, double* logjac, const JOB& job,
                                       hipStream_t st)
{
    const Geometry g = sweep_geometry(R, batch);
    constexpr int LW = Cfg<R>::LW;
    const int waves = g.cw + LW;
    int64_t wgs = (batch + g.cw * g.bt - 1) / (g.cw * g.bt);
    JOB J = job;
    if constexpr (PRIOR) {                                 // workgroups of the prior role in front of the sweeping ones
        // two waves per chain while every workgroup of both roles is resident at once (two of these workgroups fit a CU)
        const int per_wg = waves / 2;
        const bool two = (waves % 2 == 0) && wgs + (J.M.batch + per_wg - 1) / per_wg <= 512 &&
                         (size_t)per_wg * mh_prior_role2_doubles(J.M.n_nodes) * sizeof(double) <= (size_t)2 * Cfg<R>::SU * 64 * 16;
        J.wpc = two ? 2 : 1;
        const int chains = two ? per_wg : waves;
        J.n_wgs = (int)((J.M.batch + chains - 1) / chains);
        wgs += J.n_wgs;
    }
    const unsigned grid = (unsigned)wgs;
    if (g.cw == 2)
        launch_tree_fs<R, 1, 2, LW, PRIOR>(grid, st, M, T, H, Rt, lds, tH, rMu, batch, ll, logjac, J);
    else if (g.bt == 1)
        launch_tree_fs<R, 1, 4, LW, PRIOR>(grid, st, M, T, H, Rt, lds, tH, rMu, batch, ll, logjac, J);
    else if constexpr (R < 16)                             // large batches: two chains per compute wave share every factor read
        launch_tree_fs<R, 2, 4, LW, PRIOR>(grid, st, M, T, H, Rt, lds, tH, rMu, batch, ll, logjac, J);
    return hipGetLastError();
}

// the sweep of this compile's R group (sweep_groups.hpp)
hipError_t MCD_CAT(launch_tree_logpdf_g, MCD_RGROUP)(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds,
                                                     const double* tH, const double* rMu, int64_t batch, double* ll, double* logjac,
                                                     hipStream_t st)
{
#define CALL(R) launch_tree_logpdf_R<R, false, NoJob>(M, T, H, Rt, lds, tH, rMu, batch, ll, logjac, NoJob{}, st)
    MCD_DISPATCH_R(M.R, CALL)
#undef CALL
}

// ---- the same launch with the prior role in front (Metropolis-Hastings, two-launch path; launch_tree_logpdf_with_prior) ----
hipError_t MCD_CAT(launch_tree_logpdf_prior_g, MCD_RGROUP)(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds,
                                                           const double* tH, const double* rMu, int64_t batch, double* ll, double* logjac,
                                                           const MhDev& J, const PriorDev& JP, hipStream_t st)
{
    const MhPriorJob job{J, JP, 0, 1};
#define CALL(R) launch_tree_logpdf_R<R, true, MhPriorJob>(M, T, H, Rt, lds, tH, rMu, batch, ll, logjac, job, st)
    MCD_DISPATCH_R(M.R, CALL)
#undef CALL
}

}  // namespace mcd
