#pragma once
// mvn_device.hpp -- CDNA4 (gfx950) device code for McmcDate's MVN phylogenetic log-likelihood.
//
// What is computed (reference: app/Probability.hs:166-173, 195-207; app/Tools.hs:36-48;
// lib/Mcmc/Tree/Types.hs:224-233; gradient: app/Probability.hs:361-388 by AD in the reference):
//
//   ll[b] = c + (-1/2) (logdetSigma + || L^-1 (x_b - mu) ||^2),   Sigma = L L^T,  c = -N ln sqrt(2 pi)
//
// Mapping ("column sweep").  A workgroup = CW compute waves + LW loader waves.
//   * A compute wave owns BT chains.  Lane l holds rows l, l+64, ..., l+64(R-1) of each chain's
//     residual in registers (R = ceil(N/64) doubles per chain per lane).
//   * The factor is pre-scaled on the host so that the solve needs no divide on the critical
//     path:  Lt[i][j] = L[i][j] / L[i][i] (i > j),  d~_i = (x_i - mu_i) / L[i][i].
//     Then for j = 0..N-1:  z_j = d~_j (already final);  d~_i -= Lt[i][j] z_j  for i > j.
//   * z_j lives in lane (j mod 64): it is broadcast with two v_readlane_b32 into an SGPR pair
//     and consumed as the scalar operand of v_fma_f64 -- no cross-lane reduction inside the
//     sweep.  The broadcast of column j+1 is issued between the FMAs of column j (measured:
//     27.5 instead of 35 cycles per column at R = 4, tools/microbench/lat2.hip).  The only
//     reduction is the final sum z^2 (DPP + readlane).
//   * Lt is consumed in CHUNKS of CP column pairs through a two-slot LDS ring.  One CU can take in
//     only ~25-45 B/clk of L2-resident data and one wave only ~13-25 B/clk (tools/microbench/
//     stream.hip), and every LDS write costs the writing wave issue time, so dedicated LOADER
//     waves (global -> registers -> ds_write_b128, 16 B per lane, 1 KiB per wave-instruction,
//     three chunks ahead) feed the ring while the compute waves only read it (ds_read_b128,
//     conflict-free) and run the FMA chain.  One s_barrier per chunk for all waves.
//   * Rows on/above the diagonal inside a 64-row block multiply stored zeros (exact for
//     finite data; a non-finite z_j turns the chain's result into NaN, which the sampler
//     rejects exactly like the reference's NaN/Inf -- see DESIGN.md "Non-finite inputs").
//   * The gradient kernels run the mirrored sweep with Ut = scaled L^T from the last column
//     to the first on the same registers:  y = L^-T z = Sigma^-1 (x - mu),  grad_x = -y.
//
// No MFMA on purpose: this is TRSV + DOT (north_star), fp64 FMA on the vector ALU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "fc_layout.hpp"
#include "mvn_kernels.h"
#include "options.h"
#include "sweep_groups.hpp"

namespace mcd {

// native 2 x f64 vector: loads/stores stay first-class values (HIP's double2 class copies through
// memcpy, which pins register arrays to scratch)
typedef double d2 __attribute__((ext_vector_type(2)));


// ---------------------------------------------------------------------------------------
// cross-lane helpers (wave64)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double readlane64(double v, int srclane /* wave-uniform */)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, srclane);
    hi = __builtin_amdgcn_readlane(hi, srclane);
    return __hiloint2double(hi, lo);
}

template <int CTRL>
__device__ __forceinline__ double dpp_mov64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// Sum over the 64 lanes, result wave-uniform.  Fixed order => bit-reproducible.
__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_mov64<0xB1>(v);   // quad_perm [1,0,3,2]  (xor 1)
    v += dpp_mov64<0x4E>(v);   // quad_perm [2,3,0,1]  (xor 2)
    v += dpp_mov64<0x124>(v);  // row_ror:4
    v += dpp_mov64<0x128>(v);  // row_ror:8  -> every lane holds its 16-lane row sum
    return (readlane64(v, 0) + readlane64(v, 16)) + (readlane64(v, 32) + readlane64(v, 48));
}

// All LDS operations of this wave done, then workgroup barrier.  Deliberately NOT __syncthreads():
// that would also drain vmcnt and serialise the global prefetch that is still in flight.
// NOTE: pointers into the LDS ring must never be __restrict__: other waves rewrite the ring between
// barriers, and with a noalias pointer the compiler may keep values loaded from a slot across the
// barrier (seen once: chunk ci+2 computed with chunk ci's factor values when registers allowed it).
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

#define MCD_SB __builtin_amdgcn_sched_barrier(0)

// Diagnostic builds only (-DMCD_STAMP): wave-level timestamps of workgroup 0 at a few milestones.
// -DMCD_STAMP_LIGHT (with MCD_STAMP; k_logpdf.hip, `make stamp_headline`): the milestones only, kept per launch in a ring of the
// last 64 launches together with entry / exit of every workgroup on workgroup 0's XCD -- the budget of a graph-replayed launch
// (tools/microbench/headline_phases.py); no accumulators inside the sweep, so the loop under test is the shipped one.
#if defined(MCD_STAMP) && defined(MCD_STAMP_LIGHT)
__device__ unsigned long long g_dbg[64];
__device__ unsigned long long g_hist[64][8][8];            // [launch % 64][wave][milestone] of workgroup 0
__device__ unsigned long long g_span[64][64][2];           // [launch % 64][i][entry, exit] of compute wave 0 of workgroup 8 i
__device__ unsigned int g_launch;                          // launches completed (bumped by workgroup 0 at its exit)
#define MCD_T(idx)                                                                               \
    do {                                                                                         \
        unsigned long long t_;                                                                   \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");              \
        if ((threadIdx.x & 63) == 0) {                                                           \
            const unsigned ln_ = __atomic_load_n(&g_launch, __ATOMIC_RELAXED) & 63u;             \
            if (blockIdx.x == 0) g_hist[ln_][threadIdx.x >> 6][(idx)] = t_;                       \
            if ((blockIdx.x & 7) == 0 && (blockIdx.x >> 3) < 64 && threadIdx.x == 0 && ((idx) == 0 || (idx) == 4)) \
                g_span[ln_][blockIdx.x >> 3][(idx) == 0 ? 0 : 1] = t_;                           \
            if (blockIdx.x == 0 && threadIdx.x == 0 && (idx) == 4) __atomic_fetch_add(&g_launch, 1u, __ATOMIC_RELAXED); \
        }                                                                                        \
    } while (0)
#define MCD_ACC_DECL
#define MCD_ACC(idx) do { } while (0)
#define MCD_ACC_PARAMS
#define MCD_ACC_ARGS
#define MCD_ACC_FLUSH(base) do { } while (0)
#elif defined(MCD_STAMP)
__device__ unsigned long long g_dbg[64];
#define MCD_T(idx)                                                                               \
    do {                                                                                         \
        unsigned long long t_;                                                                   \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");              \
        if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) g_dbg[(threadIdx.x >> 6) * 8 + (idx)] = t_; \
    } while (0)
// accumulate the cycles since the previous MCD_ACC of this wave into bucket idx (idx < 0: restart)
__device__ __forceinline__ void mcd_acc(int idx, unsigned long long& tprev, unsigned long long* acc)
{
    unsigned long long t_;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    if (idx >= 0) acc[idx] += t_ - tprev;
    tprev = t_;
}
#define MCD_ACC_DECL unsigned long long tprev_ = 0, acc_[4] = {0, 0, 0, 0};
#define MCD_ACC(idx) mcd_acc(idx, tprev_, acc_)
#define MCD_ACC_PARAMS , unsigned long long& tprev_, unsigned long long* acc_
#define MCD_ACC_ARGS , tprev_, acc_
#define MCD_ACC_FLUSH(base)                                                                      \
    do {                                                                                         \
        if (blockIdx.x == 0 && (threadIdx.x & 63) == 0)                                          \
            for (int i_ = 0; i_ < 3; ++i_) g_dbg[(threadIdx.x >> 6) * 8 + (base) + i_] = acc_[i_]; \
    } while (0)
#else
#define MCD_T(idx) do { } while (0)
#define MCD_ACC_DECL
#define MCD_ACC(idx) do { } while (0)
#define MCD_ACC_PARAMS
#define MCD_ACC_ARGS
#define MCD_ACC_FLUSH(base) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------
// Factor stream.  Element (row = 64k + lane, column j) of a scaled triangular factor padded to
// NP = 64 R lives at   (((j >> 1) * R + k) * 64 + lane) * 2 + (j & 1)    ("pair-interleaved
// column layout": one 16-byte load per lane fetches two adjacent columns, a wave-instruction
// reads one contiguous 1-KiB UNIT = (column pair, row block)).
// ---------------------------------------------------------------------------------------
template <int R>
struct Cfg {
    static constexpr int SU = sweep_slot_units(R);          // 1-KiB units per LDS ring slot (two slots)
    static constexpr int LW = sweep_loader_waves(R);        // loader waves per workgroup
    // column pairs per chunk: CP * R <= SU
    static constexpr int CP = (R == 1) ? 32 : (R == 2) ? 16 : (R <= 4) ? 8 : (R <= 8) ? 4 : (SU / 16);
    static constexpr int CPB = 32 / CP;                     // chunks per 64-column block
    static constexpr int NCHUNK = R * CPB;
    static constexpr int CCOLS = 2 * CP;                    // columns per chunk
    static_assert(CP == fc_cp(R), "fc_layout.hpp: the same chunks");
};

constexpr int floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }

// Staging registers of one loader wave: its share (units u = i * LW + lw) of the chunks in flight.
// Set s holds a chunk of parity s.
template <int R, int LW>
struct Stage {
    static constexpr int MAXU = (Cfg<R>::CP * R + LW - 1) / LW;
    d2 v[2][MAXU];
};

// chunk of a sweep: column pairs [p0, p0 + CP), row blocks [KLO, KHI).  Unit u of the chunk goes to
// loader u % LW.  When the unit count is not a multiple of LW the surplus slots of the schedule
// reload the last unit (harmless) and skip the LDS store.
template <int R, int LW, int KLO, int KHI, int SET>
__device__ __forceinline__ void stage_load(Stage<R, LW>& st, const double* __restrict__ F, int p0, int lw, int lane)
{
    constexpr int NK = KHI - KLO;
    constexpr int NU = Cfg<R>::CP * NK;
#pragma unroll
    for (int i = 0; i < (NU + LW - 1) / LW; ++i) {
        int u = i * LW + lw;                              // wave-uniform
        if constexpr (NU % LW != 0) u = u < NU ? u : NU - 1;
        const int p = p0 + u / NK, k = KLO + u % NK;
        st.v[SET][i] = reinterpret_cast<const d2*>(F)[((size_t)p * R + k) * 64 + lane];
    }
}
// (Measured and dropped in round 4: the lanes of a DIAGONAL row block's unit that hold stored zeros -- rows up to the unit's first column,
// about a fifth of the whole stream at R = 4 -- not loading but staging the zero themselves.  Fewer bytes, but the exec-masked loads and the
// selects in the loaders' issue stream cost far more than the bytes saved: 7.6 -> 13.5 us per launch at N = 256 x 512 chains, same bits.)

template <int R, int LW, int KLO, int KHI, int SET>
__device__ __forceinline__ void stage_store(const Stage<R, LW>& st, d2* slot, int lw, int lane)
{
    constexpr int NU = Cfg<R>::CP * (KHI - KLO);
#pragma unroll
    for (int i = 0; i < (NU + LW - 1) / LW; ++i) {
        const int u = i * LW + lw;
        if constexpr (NU % LW != 0) {
            if (u < NU) slot[u * 64 + lane] = st.v[SET][i];
        } else {
            slot[u * 64 + lane] = st.v[SET][i];
        }
    }
}

// ---- the compact stream Fc (fc_layout.hpp) -------------------------------------------------------------------------------
// FS (factor stream) 0: Ft, register-staged, two ring slots; 1: Fc, register-staged, two slots; 2: Fc by LDS-DMA
// (global_load_lds_dwordx4: a wave-instruction writes one lane-linear unit straight into its slot), NS slots.  With Fc a chunk
// is fc_chunk_units consecutive units, copied as they are; the diagonal units' lanes on or above the diagonal are read from a
// zero unit behind the slots (fwd_unit), written once before the first barrier.  Compact streams serve R <= 4 (every chunk's
// diagonal part is a whole number of units there, and the loaders' schedule is compile-time: at most four chunks per block).
// (FS 3, the inverse stream Fw of the raw-x log-density, has a kernel of its own without this ring: stripe_device.hpp.)
template <int R, int FS>
struct Ring {
    // slots: LDS-DMA keeps two chunks in flight across a barrier beside the one being read and the one waited for, as register
    // staging does (measured at N = 256 x 512 chains: 3 slots 7.20 us per step, 4 slots 7.18-7.20, 5 slots 7.78)
    static constexpr int NS = FS == 2 ? 4 : 2;
    static constexpr int STRIDE = FS == 2 ? fc_chunk_units(R, 0) : Cfg<R>::SU;   // units per slot (chunk 0 is the largest)
    static constexpr int ZERO = NS * STRIDE * 64;                            // the zero unit (d2 index; FS > 0)
    static constexpr int D2 = ZERO + (FS > 0 ? 64 : 0);
    static_assert(FS >= 0 && FS <= 2, "the ring's streams");
    static_assert(FS == 0 || (R <= 4 && fc_chunk_units(R, 0) <= Cfg<R>::SU), "compact streams: R <= 4");
};

template <int R, int LW, int CI, int SET>
__device__ __forceinline__ void stage_load_c(Stage<R, LW>& st, const double* __restrict__ Fc, int lw, int lane)
{
    constexpr int NU = fc_chunk_units(R, CI), B = fc_chunk_base(R, CI);
#pragma unroll
    for (int i = 0; i < (NU + LW - 1) / LW; ++i) {
        int u = i * LW + lw;                              // wave-uniform
        if constexpr (NU % LW != 0) u = u < NU ? u : NU - 1;
        st.v[SET][i] = reinterpret_cast<const d2*>(Fc)[((size_t)B + u) * 64 + lane];
    }
}

template <int R, int LW, int CI, int SET>
__device__ __forceinline__ void stage_store_c(const Stage<R, LW>& st, d2* slot, int lw, int lane)
{
    constexpr int NU = fc_chunk_units(R, CI);
#pragma unroll
    for (int i = 0; i < (NU + LW - 1) / LW; ++i) {
        const int u = i * LW + lw;
        if constexpr (NU % LW != 0) {
            if (u < NU) slot[u * 64 + lane] = st.v[SET][i];
        } else {
            slot[u * 64 + lane] = st.v[SET][i];
        }
    }
}

// Unit (pair p of the chunk, row block JB + k) of chunk LC of block JB, this lane's 16 bytes.  FS 0: the padded layout.  Compact:
// the diagonal unit from the chunk's diagonal part where the lane is below the diagonal, else from the zero unit (one compare
// and one select, issued with the LDS prefetch); the off-diagonal units behind the diagonal part.
template <int R, int JB, int LC, int FS>
__device__ __forceinline__ d2 fwd_unit(const d2* slot, const d2* zu, int p, int k, int lane)
{
    constexpr int NK = R - JB;
    if constexpr (FS == 0) {
        return slot[(p * NK + k) * 64 + lane];
    } else {
        constexpr int CP = Cfg<R>::CP;
        if (k == 0) {
            const int pl = LC * CP + p;
            const d2* a = lane > 2 * pl ? slot + (fc_diag_start(R, LC, p) - (2 * pl + 1) + lane) : zu + lane;
            return *a;
        }
        return slot[(fc_diag_units(R, LC) + p * (NK - 1) + (k - 1)) * 64 + lane];
    }
}

// LDS -> VGPR prefetch distance (column pairs).  One wave per SIMD has nothing else to overlap the
// ~100-cycle LDS latency with, so the factor values of pair p + LDS_PD are requested before pair p
// is applied.
// (At R = 16 a prefetch buffer is 16 row blocks deep: one pair ahead there -- with two the gradient kernels, which hold both sweeps'
// buffers, spill 200 to 1 200 registers.  The sweeps are the fallback at that size: the row split and the multiply form serve it.)
template <int R> struct LdsPd { static constexpr int PD = (R >= 16) ? 1 : 2; };

// =======================================================================================
// forward sweep
// =======================================================================================
// Apply one chunk (CP column pairs starting at column offset jj0 of block JB) from an LDS slot.
template <int R, int BT, int JB, int JJ0, int FS>
__device__ __forceinline__ void fwd_apply(double (&d)[R][BT], const d2* slot, const d2* zu, int lane)
{
    constexpr int jj0 = JJ0;
    constexpr int LC = JJ0 / Cfg<R>::CCOLS;
    constexpr int CP = Cfg<R>::CP;
    constexpr int NK = R - JB;
    constexpr int LDS_PD = LdsPd<R>::PD;
    constexpr int NBUF = LDS_PD + 1;
    d2 l[NBUF][NK];
#pragma unroll
    for (int p = 0; p < LDS_PD && p < CP; ++p)
#pragma unroll
        for (int k = 0; k < NK; ++k) l[p % NBUF][k] = fwd_unit<R, JB, LC, FS>(slot, zu, p, k, lane);
    double z[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) z[b] = readlane64(d[JB][b], jj0);
#pragma unroll
    for (int p = 0; p < CP; ++p) {
        if (p + LDS_PD < CP) {
#pragma unroll
            for (int k = 0; k < NK; ++k) l[(p + LDS_PD) % NBUF][k] = fwd_unit<R, JB, LC, FS>(slot, zu, p + LDS_PD, k, lane);
        }
        MCD_SB;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int jj = jj0 + 2 * p + h;
            const bool last = (p == CP - 1) && (h == 1);
            // row block JB first: it holds row j+1, whose value is the next column's z
#pragma unroll
            for (int b = 0; b < BT; ++b) d[JB][b] = fma(-(h ? l[p % NBUF][0].y : l[p % NBUF][0].x), z[b], d[JB][b]);
            MCD_SB;
            if constexpr (NK > 1) {
#pragma unroll
                for (int b = 0; b < BT; ++b)
                    d[JB + 1][b] = fma(-(h ? l[p % NBUF][1].y : l[p % NBUF][1].x), z[b], d[JB + 1][b]);
                MCD_SB;
            }
            double zn[BT];
            if (!last) {
#pragma unroll
                for (int b = 0; b < BT; ++b) zn[b] = readlane64(d[JB][b], jj + 1);   // broadcast for column j+1
            }
            MCD_SB;
#pragma unroll
            for (int k = 2; k < NK; ++k) {
#pragma unroll
                for (int b = 0; b < BT; ++b)
                    d[JB + k][b] = fma(-(h ? l[p % NBUF][k].y : l[p % NBUF][k].x), z[b], d[JB + k][b]);
            }
            MCD_SB;
            if (!last) {
#pragma unroll
                for (int b = 0; b < BT; ++b) z[b] = zn[b];
            }
        }
    }
}

// ---- compute role -------------------------------------------------------------------------
// The chunk index is a compile-time constant so that every v_readlane has an immediate lane
// select (a lane select in a freshly written SGPR costs ~9 cycles per column, lat2.hip).
template <int R, int BT, int JB, int LC, int FS>
__device__ __forceinline__ bool fwd_compute_chunks(double (&d)[R][BT], const d2* ring, int lane, int ncols MCD_ACC_PARAMS)
{
    using C = Cfg<R>;
    if constexpr (LC < C::CPB) {
        constexpr int CI = JB * C::CPB + LC;
        if (CI * C::CCOLS >= ncols) return false;        // workgroup-uniform
        MCD_ACC(-1);
        fwd_apply<R, BT, JB, LC * C::CCOLS, FS>(d, ring + (CI % Ring<R, FS>::NS) * Ring<R, FS>::STRIDE * 64, ring + Ring<R, FS>::ZERO, lane);
        MCD_ACC(0);
        lds_barrier();
        MCD_ACC(1);
        return fwd_compute_chunks<R, BT, JB, LC + 1, FS>(d, ring, lane, ncols MCD_ACC_ARGS);
    } else {
        return true;
    }
}

template <int R, int BT, int JB, int FS = 0>
__device__ __forceinline__ void fwd_compute(double (&d)[R][BT], const d2* ring, int lane, int ncols MCD_ACC_PARAMS)
{
    if constexpr (JB < R) {
        if (!fwd_compute_chunks<R, BT, JB, 0, FS>(d, ring, lane, ncols MCD_ACC_ARGS)) return;
        fwd_compute<R, BT, JB + 1, FS>(d, ring, lane, ncols MCD_ACC_ARGS);
    }
}

// ---- loader role --------------------------------------------------------------------------
// Chunk ci = JB * CPB + lc.  On entry staging set SLOT^1 holds the loader's share of chunk ci+1
// (block JB1) and set SLOT that of chunk ci+2 (both in flight); chunk ci+3 (block JB3) is requested
// here.  The LDS write of chunk ci+1 goes to slot SLOT^1, which every compute wave has finished
// reading (barrier of chunk ci-1).
template <int R, int LW, int JB, int JB1, int JB3, int SLOT>
__device__ __forceinline__ bool fwd_loader_chunk(const double* __restrict__ Ft, d2* ring, Stage<R, LW>& st,
                                                 int lw, int lane, int ncols, int lc MCD_ACC_PARAMS)
{
    using C = Cfg<R>;
    const int ci = JB * C::CPB + lc;
    if (ci * C::CCOLS >= ncols) return false;
    MCD_ACC(-1);
    if constexpr (JB1 < R) stage_store<R, LW, JB1, R, SLOT ^ 1>(st, ring + (SLOT ^ 1) * C::SU * 64, lw, lane);
    MCD_ACC(0);
    if constexpr (JB3 < R) stage_load<R, LW, JB3, R, SLOT ^ 1>(st, Ft, (ci + 3) * C::CP, lw, lane);
    MCD_ACC(2);
    lds_barrier();
    MCD_ACC(1);
    return true;
}

template <int R, int LW, int JB, int LC>
__device__ __forceinline__ bool fwd_loader_tail(const double* __restrict__ Ft, d2* ring, Stage<R, LW>& st,
                                                int lw, int lane, int ncols MCD_ACC_PARAMS)
{
    constexpr int CPB = Cfg<R>::CPB;
    if constexpr (LC < CPB) {
        constexpr int JB1 = JB + (LC + 1) / CPB;
        constexpr int JB3 = JB + (LC + 3) / CPB;
        constexpr int SLOT = (JB * CPB + LC) & 1;
        if (!fwd_loader_chunk<R, LW, JB, JB1, JB3, SLOT>(Ft, ring, st, lw, lane, ncols, LC MCD_ACC_ARGS)) return false;
        return fwd_loader_tail<R, LW, JB, LC + 1>(Ft, ring, st, lw, lane, ncols MCD_ACC_ARGS);
    } else {
        return true;
    }
}

template <int R, int LW, int JB>
__device__ __forceinline__ void fwd_loader(const double* __restrict__ Ft, d2* ring, Stage<R, LW>& st, int lw,
                                           int lane, int ncols MCD_ACC_PARAMS)
{
    constexpr int CPB = Cfg<R>::CPB;
    if constexpr (JB < R) {
        constexpr int T0 = CPB >= 4 ? CPB - 4 : 0;          // first chunk of the compile-time tail
        for (int lc = 0; lc + 4 < CPB; lc += 2) {           // interior: the next three chunks are in this block
            if (!fwd_loader_chunk<R, LW, JB, JB, JB, 0>(Ft, ring, st, lw, lane, ncols, lc MCD_ACC_ARGS)) return;
            if (!fwd_loader_chunk<R, LW, JB, JB, JB, 1>(Ft, ring, st, lw, lane, ncols, lc + 1 MCD_ACC_ARGS)) return;
        }
        if (!fwd_loader_tail<R, LW, JB, T0>(Ft, ring, st, lw, lane, ncols MCD_ACC_ARGS)) return;
        fwd_loader<R, LW, JB + 1>(Ft, ring, st, lw, lane, ncols MCD_ACC_ARGS);
    }
}

// Start of the stream.  Only chunk 0 is requested before the first barrier: the compute waves' state loads
// share the CU's memory pipeline with the loaders, and a deeper initial burst (chunks 0-2 = 96 KiB)
// held the first barrier back by ~1.5k cycles.  Chunks 1 and 2 are requested right after the barrier
// (fwd_loader_start), while the compute waves apply chunk 0.
template <int R, int LW>
__device__ __forceinline__ void fwd_loader_prologue(const double* __restrict__ Ft, d2* ring, Stage<R, LW>& st, int lw,
                                                    int lane)
{
    stage_load<R, LW, 0, R, 0>(st, Ft, 0, lw, lane);
    stage_store<R, LW, 0, R, 0>(st, ring, lw, lane);
}

template <int R, int LW>
__device__ __forceinline__ void fwd_loader_start(const double* __restrict__ Ft, Stage<R, LW>& st, int lw, int lane)
{
    using C = Cfg<R>;
    if constexpr (C::NCHUNK > 1) stage_load<R, LW, 1 / C::CPB, R, 1>(st, Ft, C::CP, lw, lane);
    if constexpr (C::NCHUNK > 2) stage_load<R, LW, 2 / C::CPB, R, 0>(st, Ft, 2 * C::CP, lw, lane);
}

// ---- loader role, compact stream ----------------------------------------------------------------------------------------
// FS = 1: the schedule of fwd_loader above (chunk ci+1 written to its slot, ci+3 requested, one barrier per chunk) over Fc, every
// chunk index compile-time.
template <int R, int LW, int CI>
__device__ __forceinline__ void fc_loader(const double* __restrict__ Fc, d2* ring, Stage<R, LW>& st, int lw, int lane,
                                          int ncols MCD_ACC_PARAMS)
{
    using C = Cfg<R>;
    if constexpr (CI < C::NCHUNK) {
        if (CI * C::CCOLS >= ncols) return;
        constexpr int S = (CI + 1) & 1;
        MCD_ACC(-1);
        if constexpr (CI + 1 < C::NCHUNK) stage_store_c<R, LW, CI + 1, S>(st, ring + S * C::SU * 64, lw, lane);
        MCD_ACC(0);
        if constexpr (CI + 3 < C::NCHUNK) stage_load_c<R, LW, CI + 3, S>(st, Fc, lw, lane);
        MCD_ACC(2);
        lds_barrier();
        MCD_ACC(1);
        fc_loader<R, LW, CI + 1>(Fc, ring, st, lw, lane, ncols MCD_ACC_ARGS);
    }
}

// chunk 0 and the zero unit into the ring before the first barrier; chunks 1 and 2 requested after it (fc_loader_start)
template <int R, int LW>
__device__ __forceinline__ void fc_loader_prologue(const double* __restrict__ Fc, d2* ring, Stage<R, LW>& st, int lw, int lane)
{
    stage_load_c<R, LW, 0, 0>(st, Fc, lw, lane);
    if (lw == 0) ring[Ring<R, 1>::ZERO + lane] = d2{0.0, 0.0};
    stage_store_c<R, LW, 0, 0>(st, ring, lw, lane);
}

template <int R, int LW>
__device__ __forceinline__ void fc_loader_start(const double* __restrict__ Fc, Stage<R, LW>& st, int lw, int lane)
{
    if constexpr (Cfg<R>::NCHUNK > 1) stage_load_c<R, LW, 1, 1>(st, Fc, lw, lane);
    if constexpr (Cfg<R>::NCHUNK > 2) stage_load_c<R, LW, 2, 0>(st, Fc, lw, lane);
}

// FS = 2: LDS-DMA.  Chunk ci goes to slot ci % NS.  Between the barriers that publish chunks ci and ci+1 a loader requests chunk
// ci + NS - 1 (into the slot of chunk ci-1, which every compute wave finished reading before the first of them), then waits with
// a counted vmcnt for its share of chunk ci+1 and leaves the later chunks in flight across the barrier.  LDS-DMA writes count on
// vmcnt only: the barrier is lds_barrier (lgkmcnt), never __syncthreads(), whose vmcnt(0) would drain the stream.
template <int R, int LW, int FS, int CI>
__device__ __forceinline__ void fc_dma_chunk(const double* __restrict__ Fc, d2* ring, int lw, int lane)
{
    if constexpr (CI < Cfg<R>::NCHUNK) {
        constexpr int NU = fc_chunk_units(R, CI), B = fc_chunk_base(R, CI);
        const __attribute__((address_space(1))) d2* src =
            (const __attribute__((address_space(1))) d2*)reinterpret_cast<const d2*>(Fc) + ((size_t)B * 64 + lane);
        d2* slot = ring + (CI % Ring<R, FS>::NS) * Ring<R, FS>::STRIDE * 64;
#pragma unroll
        for (int i = 0; i < (NU + LW - 1) / LW; ++i) {
            const int u = i * LW + lw;                    // wave-uniform
            if (NU % LW == 0 || u < NU)
                __builtin_amdgcn_global_load_lds(src + u * 64, (__attribute__((address_space(3))) void*)(slot + u * 64), 16, 0, 0);
        }
    }
}

// the fewest LDS-DMAs any loader wave issues for chunks [c0, c1): a wave that issued more waits for a little more than it must
constexpr int fc_dma_min(int R, int LW, int c0, int c1)
{
    int s = 0;
    for (int c = c0; c < c1 && c < fc_nchunk(R); ++c) s += fc_chunk_units(R, c) / LW;
    return s;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt()
{
    static_assert(N >= 0 && N < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));   // vmcnt(N), expcnt / lgkmcnt not waited for
}

template <int R, int LW, int FS, int CI>
__device__ __forceinline__ void fc_dma_loader_chunks(const double* __restrict__ Fc, d2* ring, int lw, int lane, int ncols)
{
    using C = Cfg<R>;
    constexpr int NS = Ring<R, FS>::NS;
    if constexpr (CI < C::NCHUNK) {
        if (CI * C::CCOLS >= ncols) return;
        fc_dma_chunk<R, LW, FS, CI + NS - 1>(Fc, ring, lw, lane);
        if constexpr (CI + 1 < C::NCHUNK) wait_vmcnt<fc_dma_min(R, LW, CI + 2, CI + NS)>();
        lds_barrier();
        fc_dma_loader_chunks<R, LW, FS, CI + 1>(Fc, ring, lw, lane, ncols);
    }
}

template <int R, int LW, int FS, int C0, int C1>
__device__ __forceinline__ void fc_dma_chunks(const double* __restrict__ Fc, d2* ring, int lw, int lane)
{
    if constexpr (C0 < C1) {
        fc_dma_chunk<R, LW, FS, C0>(Fc, ring, lw, lane);
        fc_dma_chunks<R, LW, FS, C0 + 1, C1>(Fc, ring, lw, lane);
    }
}

// the whole loader role of FS = 2, first barrier included.  The stream runs from the first instruction: chunks 0 .. NS-2 are requested
// back to back, and only chunk 0 is waited for before the first barrier.
//   slots: chunk c goes to slot c % NS, so chunks 0 .. NS-2 fill NS-1 different slots of a ring nobody has read yet; slot NS-1 stays
//     free for chunk NS-1, which the loop requests at CI = 0 -- the state the loop has always started from.
//   counter: a wave's LDS-DMAs complete in the order it issued them, and it issues at least fc_dma_min(R, LW, 1, NS-1) of them for
//     chunks 1 .. NS-2 after its share of chunk 0.  Once vmcnt is down to that number, whatever is still in flight belongs to
//     those later chunks: the wave's share of chunk 0 is in LDS.  (A wave that issued more than the minimum waits for a little more.)
//   across launches: a workgroup's loaders end on vmcnt(0), so nothing of one launch is in flight into LDS when the next one starts.
template <int R, int LW, int FS>
__device__ __forceinline__ void fc_dma_loader(const double* __restrict__ Fc, d2* ring, int lw, int lane, int ncols)
{
    constexpr int NS = Ring<R, FS>::NS;
    if (lw == 0) ring[Ring<R, FS>::ZERO + lane] = d2{0.0, 0.0};
    fc_dma_chunks<R, LW, FS, 0, NS - 1>(Fc, ring, lw, lane);
    wait_vmcnt<fc_dma_min(R, LW, 1, NS - 1)>();
    MCD_T(1);
    lds_barrier();
    MCD_T(2);
    fc_dma_loader_chunks<R, LW, FS, 0>(Fc, ring, lw, lane, ncols);
    wait_vmcnt<0>();                                       // (nothing in flight into the ring when the wave ends)
}

// The loader role of a forward sweep for stream FS, first barrier included (MCD_T: the milestones of the diagnostic builds).
// F: the stream FS reads -- Ft (FS = 0) or Fc (fwd_stream_ptr).
template <int R, int LW, int FS>
__device__ __forceinline__ void fwd_loader_role(const double* __restrict__ F, d2* ring, int lw, int lane, int ncols MCD_ACC_PARAMS)
{
    if constexpr (FS == 2) {
        fc_dma_loader<R, LW, FS>(F, ring, lw, lane, ncols);
    } else if constexpr (FS == 1) {
        Stage<R, LW> st;
        fc_loader_prologue<R, LW>(F, ring, st, lw, lane);
        MCD_T(1);
        lds_barrier();
        MCD_T(2);
        fc_loader_start<R, LW>(F, st, lw, lane);
        fc_loader<R, LW, 0>(F, ring, st, lw, lane, ncols MCD_ACC_ARGS);
    } else {
        Stage<R, LW> st;
        fwd_loader_prologue<R, LW>(F, ring, st, lw, lane);
        MCD_T(1);
        lds_barrier();
        MCD_T(2);
        fwd_loader_start<R, LW>(F, st, lw, lane);
        fwd_loader<R, LW, 0>(F, ring, st, lw, lane, ncols MCD_ACC_ARGS);
    }
}

// =======================================================================================
// backward sweep.  Ut holds the scaled transpose: element (row r, column i) = L[i][r] / L[r][r] for
// r < i, zero otherwise; column block IB touches row blocks k <= IB.  Chunks are visited from the
// one that holds column ncols-1 down to chunk 0, columns inside a chunk from high to low.
// =======================================================================================
template <int R, int BT, int IB, int II0>
__device__ __forceinline__ void bwd_apply(double (&d)[R][BT], const d2* slot, int lane)
{
    constexpr int ii0 = II0;
    constexpr int CP = Cfg<R>::CP;
    constexpr int NK = IB + 1;
    constexpr int LDS_PD = LdsPd<R>::PD;
    constexpr int NBUF = LDS_PD + 1;
    d2 u[NBUF][NK];
    // pairs are visited CP-1, CP-2, ..., 0; q counts visited pairs
#pragma unroll
    for (int q = 0; q < LDS_PD && q < CP; ++q)
#pragma unroll
        for (int k = 0; k < NK; ++k) u[q % NBUF][k] = slot[((CP - 1 - q) * NK + k) * 64 + lane];
    double y[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) y[b] = readlane64(d[IB][b], ii0 + 2 * CP - 1);
#pragma unroll
    for (int q = 0; q < CP; ++q) {
        const int p = CP - 1 - q;
        if (q + LDS_PD < CP) {
#pragma unroll
            for (int k = 0; k < NK; ++k) u[(q + LDS_PD) % NBUF][k] = slot[((p - LDS_PD) * NK + k) * 64 + lane];
        }
        MCD_SB;
#pragma unroll
        for (int h = 1; h >= 0; --h) {
            const int ii = ii0 + 2 * p + h;
            const bool last = (p == 0) && (h == 0);
            // row block IB first: it holds row i-1, whose value is the next column's y
#pragma unroll
            for (int b = 0; b < BT; ++b) d[IB][b] = fma(-(h ? u[q % NBUF][IB].y : u[q % NBUF][IB].x), y[b], d[IB][b]);
            MCD_SB;
            if constexpr (NK > 1) {
#pragma unroll
                for (int b = 0; b < BT; ++b)
                    d[IB - 1][b] = fma(-(h ? u[q % NBUF][IB - 1].y : u[q % NBUF][IB - 1].x), y[b], d[IB - 1][b]);
                MCD_SB;
            }
            double yn[BT];
            if (!last) {
#pragma unroll
                for (int b = 0; b < BT; ++b) yn[b] = readlane64(d[IB][b], ii - 1);
            }
            MCD_SB;
#pragma unroll
            for (int k = IB - 2; k >= 0; --k) {
#pragma unroll
                for (int b = 0; b < BT; ++b) d[k][b] = fma(-(h ? u[q % NBUF][k].y : u[q % NBUF][k].x), y[b], d[k][b]);
            }
            MCD_SB;
            if (!last) {
#pragma unroll
                for (int b = 0; b < BT; ++b) y[b] = yn[b];
            }
        }
    }
}

// ---- compute role -------------------------------------------------------------------------
// `started` is false until the top chunk (the first one with columns < ncols) is reached; the
// loaders publish it with one extra barrier that the compute waves match here.
template <int R, int BT, int IB, int LC>
__device__ __forceinline__ void bwd_compute_chunks(double (&d)[R][BT], const d2* ring, int lane, int ncols,
                                                   bool& started)
{
    using C = Cfg<R>;
    if constexpr (LC >= 0) {
        constexpr int CI = IB * C::CPB + LC;
        if (CI * C::CCOLS < ncols) {                       // workgroup-uniform
            if (!started) {
                lds_barrier();                             // top chunk published by the loaders
                started = true;
            }
            bwd_apply<R, BT, IB, LC * C::CCOLS>(d, ring + (CI & 1) * C::SU * 64, lane);
            lds_barrier();
        }
        bwd_compute_chunks<R, BT, IB, LC - 1>(d, ring, lane, ncols, started);
    }
}

template <int R, int BT, int IB>
__device__ __forceinline__ void bwd_compute(double (&d)[R][BT], const d2* ring, int lane, int ncols,
                                            bool& started)
{
    if constexpr (IB >= 0) {
        bwd_compute_chunks<R, BT, IB, Cfg<R>::CPB - 1>(d, ring, lane, ncols, started);
        bwd_compute<R, BT, IB - 1>(d, ring, lane, ncols, started);
    }
}

// ---- loader role --------------------------------------------------------------------------
template <int R, int LW, int IB, int IB1, int IB2, int IB3, int SLOT>
__device__ __forceinline__ void bwd_loader_chunk(const double* __restrict__ Ut, d2* ring, Stage<R, LW>& st,
                                                 int lw, int lane, int ncols, int lc, bool& started)
{
    using C = Cfg<R>;
    const int ci = IB * C::CPB + lc;
    if (ci * C::CCOLS >= ncols) return;                  // above the swept columns (workgroup-uniform)
    if (!started) {                                        // top chunk: fill the pipeline
        stage_load<R, LW, 0, IB + 1, SLOT>(st, Ut, ci * C::CP, lw, lane);
        if constexpr (IB1 >= 0) stage_load<R, LW, 0, IB1 + 1, SLOT ^ 1>(st, Ut, (ci - 1) * C::CP, lw, lane);
        stage_store<R, LW, 0, IB + 1, SLOT>(st, ring + SLOT * C::SU * 64, lw, lane);
        if constexpr (IB2 >= 0) stage_load<R, LW, 0, IB2 + 1, SLOT>(st, Ut, (ci - 2) * C::CP, lw, lane);
        lds_barrier();
        started = true;
    }
    if constexpr (IB1 >= 0) stage_store<R, LW, 0, IB1 + 1, SLOT ^ 1>(st, ring + (SLOT ^ 1) * C::SU * 64, lw, lane);
    if constexpr (IB3 >= 0) stage_load<R, LW, 0, IB3 + 1, SLOT ^ 1>(st, Ut, (ci - 3) * C::CP, lw, lane);
    lds_barrier();
}

template <int R, int LW, int IB, int LC>
__device__ __forceinline__ void bwd_loader_tail(const double* __restrict__ Ut, d2* ring, Stage<R, LW>& st,
                                                int lw, int lane, int ncols, bool& started)
{
    constexpr int CPB = Cfg<R>::CPB;
    if constexpr (LC >= 0) {
        constexpr int IB1 = IB + floordiv(LC - 1, CPB);
        constexpr int IB2 = IB + floordiv(LC - 2, CPB);
        constexpr int IB3 = IB + floordiv(LC - 3, CPB);
        constexpr int SLOT = (IB * CPB + LC) & 1;
        bwd_loader_chunk<R, LW, IB, IB1, IB2, IB3, SLOT>(Ut, ring, st, lw, lane, ncols, LC, started);
        bwd_loader_tail<R, LW, IB, LC - 1>(Ut, ring, st, lw, lane, ncols, started);
    }
}

template <int R, int LW, int IB>
__device__ __forceinline__ void bwd_loader(const double* __restrict__ Ut, d2* ring, Stage<R, LW>& st, int lw,
                                           int lane, int ncols, bool& started)
{
    constexpr int CPB = Cfg<R>::CPB;
    if constexpr (IB >= 0) {
        for (int lc = CPB - 1; lc >= 5; lc -= 2) {         // interior: the next three chunks are in this block
            bwd_loader_chunk<R, LW, IB, IB, IB, IB, 1>(Ut, ring, st, lw, lane, ncols, lc, started);
            bwd_loader_chunk<R, LW, IB, IB, IB, IB, 0>(Ut, ring, st, lw, lane, ncols, lc - 1, started);
        }
        bwd_loader_tail<R, LW, IB, (CPB >= 4 ? 3 : CPB - 1)>(Ut, ring, st, lw, lane, ncols, started);
        bwd_loader<R, LW, IB - 1>(Ut, ring, st, lw, lane, ncols, started);
    }
}

// ---------------------------------------------------------------------------------------
// state -> residual prologues (compute waves)
// ---------------------------------------------------------------------------------------
// What the prologues and finish_ll read of a handle and of a topology.  The likelihood kernels (k_logpdf.hip, k_tree_logpdf.hip)
// build them from their leading scalar arguments, which the hardware hands over in SGPRs at wave launch (kernarg preload: a struct
// passed by value in front of them would switch it off); the gradient kernels still pass their MvnDev / TreeDev.
struct MvnView {
    const double* mu;
    const double* invdiag;
    int n;                     // rows of x that exist (load_rawx only)
    double c, logdet;          // finish_ll only
    __device__ MvnView(const double* mu_, const double* invdiag_, int n_, double c_, double logdet_)
        : mu(mu_), invdiag(invdiag_), n(n_), c(c_), logdet(logdet_) {}
    __device__ MvnView(const MvnDev& M) : mu(M.mu), invdiag(M.invdiag), n(M.n), c(M.c), logdet(M.logdet) {}
};
struct TreeView {
    int n_nodes, root_right;
    const int32_t* slot_node;
    const int32_t* slot_parent;
    __device__ TreeView(int n_nodes_, int root_right_, const int32_t* slot_node_, const int32_t* slot_parent_)
        : n_nodes(n_nodes_), root_right(root_right_), slot_node(slot_node_), slot_parent(slot_parent_) {}
    __device__ TreeView(const TreeDev& T) : n_nodes(T.n_nodes), root_right(T.root_right), slot_node(T.slot_node), slot_parent(T.slot_parent) {}
};

// AHEAD: every load is issued before the first value is used -- a padded row or a chain beyond the batch reads a clamped address
// and the value is dropped for mu.  (The load under `if (row < n)` with mu as the other branch makes each row block's x wait for its
// mu: R dependent round trips.  Behind the register-staged loaders that chain hides under chunk 0's arrival and AHEAD measured no
// gain; behind the LDS-DMA loaders, whose first NS-1 chunks are queued in front of every later load of the CU, it held the first
// barrier back -- profiles/r10_headline_ab.txt.  k_logpdf sets it for FS = 2.)  Same values, same arithmetic, same bits.
template <int R, int BT, bool AHEAD = false>
__device__ __forceinline__ void load_rawx(double (&d)[R][BT], const MvnView& M, const double* __restrict__ X, int64_t ldx,
                                          int64_t b0, int64_t batch, int lane)
{
    if constexpr (AHEAD) {
        double m[R], iv[R], xr[R][BT];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int row = 64 * k + lane;
            m[k] = M.mu[row];
            iv[k] = M.invdiag[row];
            const int rc = row < M.n ? row : M.n - 1;
#pragma unroll
            for (int c = 0; c < BT; ++c) {
                const int64_t bc = (b0 + c < batch) ? b0 + c : batch - 1;
                xr[k][c] = X[bc * ldx + rc];
            }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int row = 64 * k + lane;
#pragma unroll
            for (int c = 0; c < BT; ++c) {
                const double xv = (row < M.n && b0 + c < batch) ? xr[k][c] : m[k];
                d[k][c] = (xv - m[k]) * iv[k];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int row = 64 * k + lane;
            const double m = M.mu[row];        // padded: 0
            const double iv = M.invdiag[row];  // padded: 1
#pragma unroll
            for (int c = 0; c < BT; ++c) {
                const int64_t b = b0 + c;
                double xv = m;
                if (row < M.n && b < batch) xv = X[b * ldx + row];
                d[k][c] = (xv - m) * iv;       // dxs = xs - mu  (app/Probability.hs:171), then row scaling
            }
        }
    }
}

// distances from the tree state -- app/Probability.hs:201-207 with app/Tools.hs:36-48 and
// lib/Mcmc/Tree/Types.hs:224-233 folded into index tables (slot -> node, node -> parent).
template <int R, int BT>
__device__ __forceinline__ void load_tree(double (&d)[R][BT], double (&dist)[R][BT], const MvnView& M, const TreeView& T,
                                          const double* __restrict__ H, const double* __restrict__ Rt, int64_t lds,
                                          const double* __restrict__ tH, const double* __restrict__ rMu, int64_t b0,
                                          int64_t batch, int lane)
{
    double s[BT];
#pragma unroll
    for (int c = 0; c < BT; ++c) {
        const int64_t b = (b0 + c < batch) ? b0 + c : batch - 1;
        s[c] = tH[b] * rMu[b];             // :205-207  (tH * rMu)
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int row = 64 * k + lane;
        const double m = M.mu[row];
        const double iv = M.invdiag[row];
        const int a = T.slot_node[row];    // -1 for padded rows
        const int pa = T.slot_parent[row]; // 0 for padded rows
#pragma unroll
        for (int c = 0; c < BT; ++c) {
            const int64_t b = (b0 + c < batch) ? b0 + c : batch - 1;
            const double* h = H + b * lds;
            const double* r = Rt + b * lds;
            double v = 0.0;
            if (a >= 0) {
                v = (h[pa] - h[a]) * r[a];                           // zipWith (*) times rates
                if (row == 0) v = v + (h[0] - h[T.root_right]) * r[T.root_right];  // sumFirstTwo
                v = v * s[c];                                         // map (* (tH * rMu))
            }
            dist[k][c] = v;
            d[k][c] = (v - m) * iv;
        }
    }
}

// The same with the chain's height and rate rows passed through LDS (`stage`: 2 (64 R + 64) doubles private to the wave): the
// rows are read contiguously, side by side with the slot tables -- one round trip -- and the gather by node id happens in LDS,
// where load_tree gathers from global memory once the tables have arrived: two dependent round trips and a line per lane.
// Same arithmetic, same bits.  One chain per wave (BT = 1).
template <int R>
__device__ __forceinline__ void load_tree_staged(double (&d)[R][1], double (&dist)[R][1], const MvnView& M, const TreeView& T,
                                                 const double* __restrict__ H, const double* __restrict__ Rt, int64_t lds,
                                                 const double* __restrict__ tH, const double* __restrict__ rMu, int64_t b0,
                                                 int64_t batch, int lane, double* stage)
{
    constexpr int NP = 64 * R + 64;
    const int64_t b = (b0 < batch) ? b0 : batch - 1;
    const double* __restrict__ h = H + b * lds;
    const double* __restrict__ r = Rt + b * lds;
    const int nn = T.n_nodes;                              // <= 64 R + 2
    double hv[R + 1], rv[R + 1], m[R], iv[R];
    int a[R], pa[R];
#pragma unroll
    for (int i = 0; i <= R; ++i) {
        const int v = 64 * i + lane;
        const int vc = v < nn ? v : nn - 1;
        hv[i] = h[vc];
        rv[i] = r[vc];
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int row = 64 * k + lane;
        m[k] = M.mu[row];
        iv[k] = M.invdiag[row];
        a[k] = T.slot_node[row];           // -1 for padded rows
        pa[k] = T.slot_parent[row];        // 0 for padded rows
    }
    const double s = tH[b] * rMu[b];       // :205-207  (tH * rMu)
    const int rr = T.root_right;
#pragma unroll
    for (int i = 0; i <= R; ++i) {
        stage[64 * i + lane] = hv[i];
        stage[NP + 64 * i + lane] = rv[i];
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);    // lgkmcnt(0): the rows are in LDS (one wave: LDS operations complete in order)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int row = 64 * k + lane;
        double v = 0.0;
        if (a[k] >= 0) {
            v = (stage[pa[k]] - stage[a[k]]) * stage[NP + a[k]];                           // zipWith (*) times rates
            if (row == 0) v = v + (stage[0] - stage[rr]) * stage[NP + rr];                 // sumFirstTwo
            v = v * s;                                                                      // map (* (tH * rMu))
        }
        dist[k][0] = v;
        d[k][0] = (v - m[k]) * iv[k];
    }
}

template <int R, int BT>
__device__ __forceinline__ void finish_ll(const double (&d)[R][BT], const MvnView& M, int64_t b0, int64_t batch,
                                          double* __restrict__ ll, int lane)
{
#pragma unroll
    for (int c = 0; c < BT; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(d[k][c], d[k][c], s);
        const double q = wave_sum(s);
        if (lane == 0 && b0 + c < batch) ll[b0 + c] = M.c + (-0.5) * (M.logdet + q);  // app/Probability.hs:169
    }
}

// Chain rule from g = d ll / d distances back to heights, rates, tH, rMu (SURVEY.md 8a A7:
// d ll/d r_v = s g t_v, d ll/d h_v = s (sum_children g_c r_c - g_v r_v), d ll/d tH = g.d / tH) for chain b by the wave that
// holds d = y = Sigma^-1 (dist - mu), g = -y, after both sweeps.  e[v] = s * g[row(v)] * rate[v] is exchanged through e: n_nodes_pad
// doubles of LDS private to the wave.  No barriers.  (k_tree_grad.hip; the one-launch NUTS transition, k_nuts_chain.hip)
template <int R>
__device__ __forceinline__ void tree_grad_tail(const double (&d)[R][1], const double (&dist)[R][1], const TreeDev& T, const double* H, const double* Rt,
                                               int64_t lds, const double* tH, const double* rMu, int64_t b, double* e, int lane, double* gH,
                                               double* gR, double* gtH, double* grMu)
{
    const double s = tH[b] * rMu[b];
    const double* h = H + b * lds;
    const double* r = Rt + b * lds;
    double gd = 0.0;
    if (lane == 0) e[0] = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int row = 64 * k + lane;
        const int a = T.slot_node[row];
        const double g = -d[k][0];
        gd = fma(g, dist[k][0], gd);
        if (a >= 0) {
            const int pa = T.slot_parent[row];
            const double sg = s * g;
            gR[b * lds + a] = sg * (h[pa] - h[a]);
            e[a] = sg * r[a];
            if (row == 0) {
                const int a2 = T.root_right;
                gR[b * lds + a2] = sg * (h[0] - h[a2]);
                e[a2] = sg * r[a2];
            }
        }
    }
    const double gdot = wave_sum(gd);
    if (lane == 0) {
        gR[b * lds] = gdot == gdot ? 0.0 : gdot;   // stem rate: unused by the likelihood (a NaN chain: NaN, as every other entry)
        gtH[b] = gdot / tH[b];
        grMu[b] = gdot / rMu[b];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's e[] writes have landed (wave-private region)
    for (int v = lane; v < T.n_nodes; v += 64) {
        double acc = (v == 0) ? 0.0 : -e[v];
        for (int ci = T.child_ptr[v]; ci < T.child_ptr[v + 1]; ++ci) acc += e[T.child_idx[ci]];
        gH[b * lds + v] = acc;
    }
}

// ---------------------------------------------------------------------------------------
// Kernel skeleton.  Waves 0 .. CW-1 compute, waves CW .. CW+LW-1 load.  Every wave of a
// workgroup takes part in every barrier, also compute waves whose chains lie beyond the batch
// (they work on clamped inputs and store nothing): no early exits before the last barrier.
// ---------------------------------------------------------------------------------------
// (MCD_BID: the workgroup's index among the likelihood workgroups; a kernel that puts workgroups of another role in front of
// them -- k_tree_logpdf.hip -- defines it before including this header)
#ifndef MCD_BID
#define MCD_BID blockIdx.x
#endif
// (MCD_KERNEL_HEAD_FS: for a kernel that takes `ncols` as an argument of its own)
#define MCD_KERNEL_HEAD                                                         \
    MCD_KERNEL_HEAD_FS(0)                                                       \
    const int ncols = M.ncols;   /* swept columns: N rounded up to whole chunks (host: sweep_chunk_columns) */
#define MCD_KERNEL_HEAD_FS(FS_)                                                 \
    __shared__ d2 ring[Ring<R, (FS_)>::D2];                                     \
    const int lane = threadIdx.x & 63;                                          \
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);          \
    const int64_t b0 = ((int64_t)MCD_BID * CW + wave) * BT;

// The forward factor stream of the column sweep (host side; mcd_set_option "MCD_FSTREAM", A/B and tests): compact streams at 129 ..
// 256 dimensions (R = 3, 4), the padded one elsewhere.  By default the compact stream by LDS-DMA where a workgroup has a CU to itself
// anyway (two compute waves: up to 512 chains), and the padded stream with four compute waves: there two workgroups share a CU on
// the two-slot ring, which the four DMA slots would not leave room for, and the compact stream staged through registers measured no
// gain on the sweep; MCD_FSTREAM = 1 or 2 forces a compact stream in every geometry (tests).  The choice itself
// is sweep_fwd_stream (sweep_groups.hpp); inverse: the launch may take the inverse stream (raw x in the two-compute-wave geometry: k_logpdf_stripe) and the
// call lies in the window where it is the default (logpdf_inverse_window) -- without it MCD_FSTREAM = 3 means the geometry's default.
template <int R>
static inline int fwd_stream(int cw, bool has_inverse = false, bool inverse_window = false)
{
    return sweep_fwd_stream(R, cw, has_inverse, inverse_window);
}
// the factor a sweep with stream fs reads (the kernels' first argument)
static inline const double* fwd_stream_ptr(const MvnDev& M, int fs) { return fs == 0 ? M.Ft : fs == 3 ? M.Fw : M.Fc; }

// The workgroup of a gradient sweep (host side; k_grad.hip, k_tree_grad.hip): go(std::integral_constant<int, CW>) launches with CW compute
// waves and grad_loader_waves(R) loaders.
// (the gradient holds the forward AND the backward sweep's staging: above R = 6 four compute waves per workgroup, and at R = 12 four
// loader waves, no longer fit two waves per SIMD -- 140 .. 1 219 spilled registers -- so those sizes take two compute waves, and two
// loaders from R = 12: one wave per SIMD, the whole register file.  The sweeps are the fallback there: up to 1024 chains the row split
// serves the gradient, from 2048 the multiply form.)
constexpr int grad_loader_waves(int R) { return (R == 12) ? 2 : sweep_loader_waves(R); }
template <int R, class GO>
static inline void grad_launch_geometry(int64_t batch, GO go)
{
    if constexpr (R >= 8) {
        go(std::integral_constant<int, 2>{});
    } else {
        if (pick_geometry(batch).cw == 2)
            go(std::integral_constant<int, 2>{});
        else
            go(std::integral_constant<int, 4>{});
    }
}

}  // namespace mcd
