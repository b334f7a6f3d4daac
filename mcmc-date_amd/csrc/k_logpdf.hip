// k_logpdf.hip -- batched log-density, raw x (gfx950).  Device code: mvn_device.hpp.
// (The choice of form -- use_split, use_wide, the MCD_WIDE default -- and the public launch_logpdf live in sweep_launch.cpp.)
#include "mvn_device.hpp"
#include "stripe_device.hpp"

namespace mcd {

// The leading arguments are what the first memory instructions of either role need, scalars and pointers only: gfx950 preloads
// them into SGPRs at wave launch (-mllvm -amdgpu-kernarg-preload-count, Makefile), so the loads of x and the first LDS-DMA of the
// factor do not wait for a scalar load from a cold kernarg segment first.  14 dwords fit beside the kernarg pointer in the 16 user
// SGPRs: F (the stream FS reads, fwd_stream_ptr) .. ncols.  ll, c and logdet are used by finish_ll only and arrive the ordinary way.
template <int R, int BT, int CW, int LW, int FS>
__global__ void __launch_bounds__(64 * (CW + LW)) k_logpdf(const double* __restrict__ F, const double* __restrict__ mu,
                                                           const double* __restrict__ invdiag, const double* __restrict__ X, int64_t ldx,
                                                           int64_t batch, int n, int ncols, double* __restrict__ ll, double c, double logdet)
{
    MCD_KERNEL_HEAD_FS(FS)
    MCD_ACC_DECL
    MCD_T(0);
    if (wave >= CW) {                                      // loader role
        const int lw = wave - CW;
        fwd_loader_role<R, LW, FS>(F, ring, lw, lane, ncols MCD_ACC_ARGS);
        MCD_T(3);
        MCD_ACC_FLUSH(5);
        return;
    }
    const MvnView M(mu, invdiag, n, c, logdet);
    double d[R][BT];
    load_rawx<R, BT, FS == 2>(d, M, X, ldx, b0, batch, lane);
    MCD_T(1);
    lds_barrier();
    MCD_T(2);
    fwd_compute<R, BT, 0, FS>(d, ring, lane, ncols MCD_ACC_ARGS);
    MCD_T(3);
    finish_ll<R, BT>(d, M, b0, batch, ll, lane);
    MCD_T(4);
    MCD_ACC_FLUSH(5);
}

// The inverse stream (FS = 3; R = 3, 4, up to 512 chains): S stripe waves, two chains per workgroup, every wave a share of Fw of its
// own (stripe_device.hpp, which describes the forms; stripe_plan.hpp: stripe_form chooses).  The same arguments, preloaded the same way.
// SH: the shared prologue (the default) or the private one ("MCD_STRIPE_PROLOGUE" = 0); SC (with SH only): schedule 0, 1 or 2
// ("MCD_STRIPE_SCHED"; 2 is the default, whole sweeps only).  Wave 0 finishes both chains.  A/B, tests: the same bits.  Four kernels per R.
template <int R, int S, bool SH, int SC>
__global__ void __launch_bounds__(64 * S) k_logpdf_stripe(const double* __restrict__ Fw, const double* __restrict__ mu,
                                                          const double* __restrict__ invdiag, const double* __restrict__ X, int64_t ldx,
                                                          int64_t batch, int n, int ncols, double* __restrict__ ll, double c, double logdet)
{
    __shared__ d2 ring[SH ? Stripe<R, S>::D3 : Stripe<R, S>::D2];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    MCD_T(0);
    const MvnView M(mu, invdiag, n, c, logdet);
    stripe_dispatch<StripeWaveOf<R, S, SH, SC>>(wave, Fw, ring, M, X, ldx, (int64_t)blockIdx.x * 2, batch, ncols, ll, lane);
}

// Schedule 2 under the shared prologue with a finishing wave per chain, over the form F (stripe_device.hpp: StripeWavePlan): the body
// of the two kernels below.  c and logdet are not read here -- the finishing waves fetch them from their place in the arguments
// (kStripeArgC), which the kernels' list fixes: eight 8-byte arguments (n and ncols share one), then ll, c, logdet.
template <class F>
__device__ __forceinline__ void stripe_kernel_per_chain(d2* lds, const double* __restrict__ Fw, const double* __restrict__ mu,
                                                        const double* __restrict__ invdiag, const double* __restrict__ X, int64_t ldx, int64_t batch,
                                                        int n, int ncols, double* __restrict__ ll)
{
    static_assert(kStripeArgC == 8 * 8, "c follows Fw, mu, invdiag, X, ldx, batch, {n, ncols} and ll");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    MCD_T(0);
    const MvnView M(mu, invdiag, n, 0.0, 0.0);
    stripe_dispatch<StripeWavePlan<F, true>>(wave, Fw, lds, M, X, ldx, (int64_t)blockIdx.x * 2, batch, ncols, ll, lane);
}
// The diagonal parts through the LDS ring ("MCD_STRIPE_FINISH" = 0 keeps k_logpdf_stripe<R, S, true, 2>; the same bits).  Kernels of
// their own names: the audit of the generated code finds each by its prefix.
template <int R, int S>
__global__ void __launch_bounds__(64 * S) k_logpdf_stripe_fin(const double* __restrict__ Fw, const double* __restrict__ mu,
                                                              const double* __restrict__ invdiag, const double* __restrict__ X, int64_t ldx,
                                                              int64_t batch, int n, int ncols, double* __restrict__ ll, double c, double logdet)
{
    __shared__ d2 ring[Stripe<R, S>::LDS];
    stripe_kernel_per_chain<Stripe<R, S>>(ring, Fw, mu, invdiag, X, ldx, batch, n, ncols, ll);
}
// The diagonal parts by register load too ("MCD_STRIPE_DIAG" = 1; the same bits).  No ring: LDS is the exchange area and the hand-over
// of the partial sums.  The same arguments in the same places.
template <int R, int S>
__global__ void __launch_bounds__(64 * S) k_logpdf_stripe_reg(const double* __restrict__ Fw, const double* __restrict__ mu,
                                                              const double* __restrict__ invdiag, const double* __restrict__ X, int64_t ldx,
                                                              int64_t batch, int n, int ncols, double* __restrict__ ll, double c, double logdet)
{
    __shared__ d2 lds[StripeReg<R, S>::LDS];
    stripe_kernel_per_chain<StripeReg<R, S>>(lds, Fw, mu, invdiag, X, ldx, batch, n, ncols, ll);
}

template <class K>
static void launch_stripe_kernel(K kernel, const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, hipStream_t st)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)((batch + 1) / 2)), dim3(64 * kStripeWaves), 0, st, M.Fw, M.mu, M.invdiag, X, ldx, batch, M.n,
                       M.ncols, ll, M.c, M.logdet);
}
template <int R>
static void launch_stripe(const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, hipStream_t st)
{
    static_assert(kStripeUnset == MCD_OPT_UNSET, "stripe_form's unset option");
    constexpr int S = kStripeWaves;
    switch (stripe_form(opt_get(OPT_STRIPE_PROLOGUE), opt_get(OPT_STRIPE_SCHED), opt_get(OPT_STRIPE_FINISH), opt_get(OPT_STRIPE_DIAG), batch, R,
                        M.ncols)) {
    case kStripePrivate0: return launch_stripe_kernel(k_logpdf_stripe<R, S, false, 0>, M, X, ldx, batch, ll, st);
    case kStripeShared0: return launch_stripe_kernel(k_logpdf_stripe<R, S, true, 0>, M, X, ldx, batch, ll, st);
    case kStripeShared1: return launch_stripe_kernel(k_logpdf_stripe<R, S, true, 1>, M, X, ldx, batch, ll, st);
    case kStripeShared2: return launch_stripe_kernel(k_logpdf_stripe<R, S, true, 2>, M, X, ldx, batch, ll, st);
    case kStripeFin: return launch_stripe_kernel(k_logpdf_stripe_fin<R, S>, M, X, ldx, batch, ll, st);
    case kStripeReg: return launch_stripe_kernel(k_logpdf_stripe_reg<R, S>, M, X, ldx, batch, ll, st);
    }
}

template <int R, int BT, int CW, int LW, int FS>
static void launch_fs(const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, hipStream_t st)
{
    const int64_t per_wg = (int64_t)CW * BT;
    const unsigned grid = (unsigned)((batch + per_wg - 1) / per_wg);
    hipLaunchKernelGGL((k_logpdf<R, BT, CW, LW, FS>), dim3(grid), dim3(64 * (CW + LW)), 0, st, fwd_stream_ptr(M, FS), M.mu, M.invdiag, X, ldx,
                       batch, M.n, M.ncols, ll, M.c, M.logdet);
}

template <int R, int BT, int CW, int LW>
static void launch_geom(const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, hipStream_t st)
{
    if constexpr (fwd_stream_compact(R)) {
        constexpr bool INV = CW == 2 && BT == 1;           // the geometry the inverse stream replaces (one workgroup per CU)
        const int fs = fwd_stream<R>(CW, INV, INV && logpdf_inverse_window(MvnFacts(M), batch));
        if (fs == 1) return launch_fs<R, BT, CW, LW, 1>(M, X, ldx, batch, ll, st);
        if (fs == 2) return launch_fs<R, BT, CW, LW, 2>(M, X, ldx, batch, ll, st);
        if constexpr (INV)
            if (fs == 3) return launch_stripe<R>(M, X, ldx, batch, ll, st);   // (whatever LW: it has no loader waves)
    }
    launch_fs<R, BT, CW, LW, 0>(M, X, ldx, batch, ll, st);
}

template <int R>
static hipError_t launch_logpdf_R(const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, hipStream_t st)
{
    const Geometry g = sweep_geometry(R, batch);
    if constexpr (R == 3 || R == 4) {
        // Four loader waves beside the two compute waves at 129 .. 256 dimensions (round 4): one wave pulls 13 - 25 B/clk out of the L2, two do not
        // reach the CU's ingest rate -- N = 256 x 512 chains 7.62 -> 7.41 us per launch, N = 192 5.83 -> 5.50 (same box; 3 waves 8.46 / 6 waves 8.20
        // against 8.82 / 7.42 for 2 / 4 on a slower box); no gain at one or two row blocks.  mcd_set_option "MCD_LOADERS" = 2 keeps two (A/B).
        if (g.cw == 2 && opt_or(OPT_LOADERS, 4) == 4) {
            launch_geom<R, 1, 2, 4>(M, X, ldx, batch, ll, st);
            return hipGetLastError();
        }
    }
    if (g.cw == 2)
        launch_geom<R, 1, 2, Cfg<R>::LW>(M, X, ldx, batch, ll, st);
    else if (g.bt == 1)
        launch_geom<R, 1, 4, Cfg<R>::LW>(M, X, ldx, batch, ll, st);
    else if constexpr (R < 16)                             // (sweep_geometry: one chain per compute wave at R = 16)
        launch_geom<R, 2, 4, Cfg<R>::LW>(M, X, ldx, batch, ll, st);
    return hipGetLastError();
}

// the sweep of this compile's R group (sweep_groups.hpp)
hipError_t MCD_CAT(launch_logpdf_g, MCD_RGROUP)(const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, hipStream_t st)
{
#define CALL(R) launch_logpdf_R<R>(M, X, ldx, batch, ll, st)
    MCD_DISPATCH_R(M.R, CALL)
#undef CALL
}

}  // namespace mcd

#ifdef MCD_STAMP
extern "C" int mcd_debug_stamps(unsigned long long* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mcd::g_dbg), 64 * sizeof(unsigned long long));
}
#endif
#if defined(MCD_STAMP) && defined(MCD_STAMP_LIGHT) && MCD_RGROUP == 0
// the ring of the last 64 launches: hist [64][8][8], span [64][64][2], *n = launches completed
extern "C" int mcd_debug_hist(unsigned long long* hist, unsigned long long* span, unsigned int* n)
{
    if (hipMemcpyFromSymbol(hist, HIP_SYMBOL(mcd::g_hist), 64 * 8 * 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(span, HIP_SYMBOL(mcd::g_span), 64 * 64 * 2 * sizeof(unsigned long long)) != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(n, HIP_SYMBOL(mcd::g_launch), sizeof(unsigned int));
}
#endif
