#pragma once
// stripe_device.hpp -- the inverse stream (FS = 3) of the raw-x log-density at R = 3, 4 and up to 512 chains: z = W (x - mu) with
// W = L^-1 read from Fw (fc_layout.hpp) by S "stripe" waves, no loader waves and no barrier inside the sweep.
//
// What every form shares
//   * One workgroup serves 2 chains; every stripe wave holds both (the accumulators a[R][2]) and multiplies only the units dealt to it
//     (stripe_deal.hpp).  Nothing forces two waves to read the same bytes, so each wave loads its own units, and ordering inside a
//     wave is the wave's own counters: a wave's loads land in issue order, so once vmcnt is down to the number of loads issued behind
//     unit u, unit u is there.  The compiler does not know which load a read depends on and would wait for all of them, so the loads
//     and the reads behind them are asm statements, with the waits written out; for the same reason the loads of x, mu and 1/diag,
//     issued before the first unit, are asm loads waited for by count.
//   * Order of additions, fixed: within a wave a row's additions follow the wave's list (chunk after chunk; a chunk's diagonal part
//     pair by pair, then its off-diagonal pairs, per pair column 2p before 2p + 1, row blocks ascending).  Wave 0's accumulators
//     start at r_i invdiag_i, the others at 0.  After its last unit the waves hand their partial sums over through LDS; one barrier;
//     z_i = ((a0 + a1) + a2) + ... in wave order, then finish_ll's operations.  Every form below keeps operands and order, so all give
//     the same bits.  The bits belong to the S the library is built with (kStripeWaves): another S deals the units differently.
//   * Every wave's code is its own instantiation (W is a template parameter): list positions, slots, wait counts and lane selects
//     are immediates.  stripe_dispatch sends a wave to its body.
//   * The waves end on vmcnt(0): nothing of one launch is in flight when the next one starts.
//   * The lookahead A (kStripeAhead, -DMCD_STRIPE_AHEAD; kStripeRegAhead, -DMCD_STRIPE_REG_AHEAD for the form without a ring): units
//     requested ahead of the unit being read, and the prologue's burst.
// The forms (stripe_plan.hpp: stripe_form chooses one per launch from the options and the launch's shape; k_logpdf.hip: launch_stripe)
//   * The LDS ring (Stripe<R, S>): each wave loads its units by LDS-DMA into a ring of D units that only it reads, the u-th unit of its
//     list at slot u mod D, and reads them by ds_read_b128; the DMA of unit u + A (A <= D) is issued once the reads of unit u have
//     returned.  A sweep that stops early (ncols < 64 R) has requested up to A units behind the cut; they land in the wave's own ring
//     and are never read.
//   * The prologue.  Private (MCD_STRIPE_PROLOGUE = 0; stripe_prologue_private): every wave loads x, mu and 1/diag for itself.  Shared
//     (the default; stripe_prologue_shared): row block k belongs to wave k mod S, which loads mu_k, 1/diag_k and both chains' x_k in
//     front of its first unit, forms r = x - mu and t = r invdiag with the operations of the private prologue and stores both into an
//     exchange area ([r | t][R][64 lanes][2 chains], one 16-byte access per lane for both chains).  One barrier that waits for LDS only
//     -- the loads stay in flight across it -- then every wave reads what it needs of r and wave 0 also t.
//   * Schedule 0 (MCD_STRIPE_SCHED = 0, and the private prologue's only one; stripe_chunks): chunk after chunk, wait, read, request,
//     multiply, the column broadcasts by v_readlane.
//   * Schedule 1 (MCD_STRIPE_SCHED = 1, and every sweep that stops early; stripe_sched, stripe_ahead).  A wave alone on its SIMD is
//     bound by its own VALU issue, and a wave body of schedule 0 spends 404 lane selects beside 322 multiply-adds (R = 4).  r stays in
//     the exchange area for the whole launch, both chains of a row in one 16-byte slot, so the broadcast of column j is one
//     ds_read_b128 of the same address in every lane and the multiply-add takes it as a vector operand: the same value.  And the unit
//     reads and broadcasts of group g + 1 (stripe_plan.hpp: stripe_groups) go into a second register set and are issued in front of the
//     multiply-adds of group g.  A group whose chunk the early stop cuts is neither waited for nor read.
//   * Schedule 2 (the default; whole sweeps only; StripeWavePlan over stripe_plan_sched, stripe_plan_ahead).  Every unit has one
//     reader, the wave that requested it, and an off-diagonal unit needs no lane shift -- lane l's 16 bytes are the two entries of row
//     l that lane l multiplies.  Those units (three quarters of the stream at R = 4) skip LDS: one global_load_dwordx4 with a scalar
//     base, 16 l as the vector offset and an immediate brings the unit into a register ring, with no vector address arithmetic, no M0
//     write, no ds_read and no lgkmcnt wait.  Both kinds of request count on vmcnt in issue order; one constexpr plan per wave
//     (stripe_plan.hpp) holds every request's kind, slot, base and immediate and every group's wait, and is proved at compile time.
//     The wave body is written once over a FORM, which supplies the plan and the LDS layout:
//       - Stripe<R, S>: the diagonal parts keep their LDS-DMAs, ring slots and lane-shifted reads (k_logpdf_stripe<R, S, true, 2>,
//         k_logpdf_stripe_fin);
//       - StripeReg<R, S> (MCD_STRIPE_DIAG = 1, the default from kStripeDiagFrom chains on; k_logpdf_stripe_reg): the diagonal parts by
//         register load too, see there.
//   * The finish.  Wave 0 finishes both chains (MCD_STRIPE_FINISH = 0, and every form but schedule 2's), or each chain is finished by
//     a wave of its own (schedule 2's default; stripe_finish_chain).  Wave 0's finish stands in both wave bodies, StripeWavePlan and
//     StripeWaveLoop, word for word: as a function of its own it changed the generated code of the eight k_logpdf_stripe kernels.
// Measured and not kept (profiles/r16_stripe_schedule_ab.txt, docs/experiments/r16_stripe_read_ahead_fill.diff): the read-ahead
// without the broadcasts, a fill of the ring behind the operand loads, a burst shorter than the lookahead.
#include <type_traits>

#include "mvn_device.hpp"
#include "stripe_deal.hpp"
#include "stripe_plan.hpp"

namespace mcd {

#ifndef MCD_STRIPE_WAVES
#define MCD_STRIPE_WAVES 4
#endif
constexpr int kStripeWaves = MCD_STRIPE_WAVES;
// Measured (profiles/r14_stripe_prologue_ab.txt; N = 256 x 512 chains, us per launch): A = 32, the whole ring, 5.96; 24 5.73; 20 5.66;
// 16 5.54; 14 5.47; 12 5.44; 10 5.49; 8 5.61.  With A = 32 a CU's four waves requested 128 KiB before they looked at anything, and the
// loads of x stood in that queue; 4 x 12 KiB still covers the latency-bandwidth product (about 28 KiB) with room to spare.
#ifndef MCD_STRIPE_AHEAD
#define MCD_STRIPE_AHEAD 12
#endif
constexpr int kStripeAhead = MCD_STRIPE_AHEAD;

// The ring's layout, and as a form of schedule 2's wave body: the diagonal parts through the ring
template <int R_, int S_>
struct Stripe {
    static constexpr int R = R_, S = S_;
    static_assert((R == 3 || R == 4) && (S == 4 || S == 8), "stripe kernel: R = 3, 4; S = 4, 8");
    // ring units per wave: S D KiB + the waves' zero units within 160 KiB, and x loads + D DMAs within the 6 bits of vmcnt
    static constexpr int D = 128 / S;
    static constexpr int A = kStripeAhead < D ? kStripeAhead : D;   // the lookahead (units), at most the ring
    static_assert(A >= 1, "MCD_STRIPE_AHEAD");
    static constexpr int ZERO = S * D * 64;               // the waves' zero units (d2 index)
    static constexpr int D2 = ZERO + S * 64;
    static constexpr int EXCH = D2;                       // the shared prologue's exchange area [r | t][R][64] (d2 index: both chains)
    static constexpr int D3 = EXCH + 2 * R * 64;
    static_assert(D3 * 16 <= 160 * 1024, "LDS");
    // leading loads in front of the DMAs: 4 R (private prologue, wave 0), 4 per row block owned (shared)
    static_assert(4 * R + D < 64, "vmcnt");
    static constexpr StripeDeal T = stripe_deal(R, S);
    static constexpr bool RING = true;                    // the form: an LDS ring and zero units; the plan's lookahead and register slots;
    static constexpr int AHEAD = A, NS = kStripeRegSlots;
    static constexpr int HAND = 0, REGION = D * 1024;     // the hand-over of the partial sums in the waves' ring regions (d2 index; bytes)
    static constexpr int LDS = D3;
};

// LDS byte address of a pointer into the ring
__device__ __forceinline__ unsigned lds_addr(const void* p)
{
    return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)p;
}

template <int N>
__device__ __forceinline__ void asm_wait_vmcnt()
{
    static_assert(N >= 0 && N < 64, "vmcnt");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// 16 bytes per lane from LDS, outside the compiler's bookkeeping; lds_landed() before the first use
template <int OFF>
__device__ __forceinline__ void lds_read16(d2& v, unsigned addr)
{
    static_assert(OFF >= 0 && OFF < 65536, "ds offset");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_write16(unsigned addr, d2 v)
{
    static_assert(OFF >= 0 && OFF < 65536, "ds offset");
    asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
template <int N, int M>
__device__ __forceinline__ void lds_landed(d2 (&v)[M])
{
    static_assert(N <= M, "lds_landed");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(v[i]));
}

__device__ __forceinline__ void asm_load8(double& v, const double* p)
{
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
}

// the DMA of unit UNIT of Fw into slot SLOT of the wave's ring; my: the ring's LDS byte address (an integer: a pointer converted back
// from the generic address space would carry a null check into every M0 write)
template <int UNIT, int SLOT>
__device__ __forceinline__ void stripe_dma(const double* __restrict__ Fw, unsigned my, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)                       // (an LDS pointer is 32 bits wide on the device only)
    const __attribute__((address_space(1))) d2* src =
        (const __attribute__((address_space(1))) d2*)reinterpret_cast<const d2*>(Fw) + ((size_t)UNIT * 64 + lane);
    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(my + SLOT * 1024u), 16, 0, 0);
#endif
}
// ... of list positions [U0, U1)
template <int R, int S, int W, int U0, int U1>
__device__ __forceinline__ void stripe_issue(const double* __restrict__ Fw, unsigned my, int lane)
{
    if constexpr (U0 < U1) {
        stripe_dma<Stripe<R, S>::T.unit[W][U0], U0 % Stripe<R, S>::D>(Fw, my, lane);
        stripe_issue<R, S, W, U0 + 1, U1>(Fw, my, lane);
    }
}

// The groups of wave W (stripe_plan.hpp), the group of its off-diagonal pairs of chunk CI (-1: none), the list position behind the last
// of those pairs (-1) and their units
template <int R, int S, int W>
constexpr StripeGroups stripe_groups()
{
    return stripe_groups(Stripe<R, S>::T, R, W);
}
template <int R, int S, int W, int CI>
constexpr int stripe_pairs_group()
{
    constexpr StripeGroups Q = stripe_groups<R, S, W>();
    for (int g = 0; g < Q.n; ++g)
        if (Q.ci[g] == CI && Q.diag[g] == 0) return g;
    return -1;
}
template <int R, int S, int W, int CI>
constexpr int stripe_pairs_end()
{
    constexpr int g = stripe_pairs_group<R, S, W, CI>();
    return g < 0 ? -1 : stripe_groups<R, S, W>().end[g < 0 ? 0 : g];
}
template <int R, int S, int W, int CI>
constexpr int stripe_pairs_units()
{
    constexpr int g = stripe_pairs_group<R, S, W, CI>();
    return g < 0 ? 0 : stripe_groups<R, S, W>().end[g < 0 ? 0 : g] - stripe_groups<R, S, W>().beg[g < 0 ? 0 : g];
}
// registers a group's reads fill, and the columns it multiplies (two per pair)
template <int R, int S, int W, int GI>
constexpr int stripe_group_regs()
{
    constexpr StripeGroups Q = stripe_groups<R, S, W>();
    return Q.diag[GI] != 0 ? 8 : Q.end[GI] - Q.beg[GI];
}
template <int R, int S, int W, int GI>
constexpr int stripe_group_cols()
{
    constexpr StripeGroups Q = stripe_groups<R, S, W>();
    return Q.diag[GI] != 0 ? 16 : 2 * (Q.end[GI] - Q.beg[GI]) / (R - 1 - Q.ci[GI] / 4);
}

// The LDS addresses of the eight column pairs of a diagonal part in the ring, chunk LC of its block, the part's first unit at list
// position DPOS: pair p's lanes 2 pl + 1 .. 63 lie back to back in the part, the others read the wave's zero unit.  la, za: the ring's
// and the zero unit's LDS byte address + 16 lane.  PIN: every address is formed where this stands.
template <int R, int S, int LC, int DPOS, bool PIN>
__device__ __forceinline__ void stripe_diag_addrs(unsigned (&ad)[8], unsigned la, unsigned za, int lane)
{
    constexpr int D = Stripe<R, S>::D;
    static_assert(fc_diag_units(R, LC) <= D, "a group within the ring");
    constexpr bool WRAP = DPOS % D + fc_diag_units(R, LC) > D;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int pl = LC * 8 + p;
        int i = (DPOS % D) * 64 + fc_diag_start(R, LC, p) - (2 * pl + 1) + lane;
        if (WRAP) i = i >= D * 64 ? i - D * 64 : i;
        ad[p] = lane > 2 * pl ? la - 16u * (unsigned)lane + 16u * (unsigned)i : za;
        if constexpr (PIN) asm volatile("" : "+v"(ad[p]));   // (formed here: hoisted to the kernel's top the 32 addresses of a wave cost it its registers)
    }
}

// off-diagonal pairs P .. 7 of chunk CI that wave W owns: reads of all of them first, then the multiply-adds
template <int R, int S, int W, int CI, int P, int NREAD>
__device__ __forceinline__ void stripe_pairs_read(d2 (&l)[8 * 3], unsigned la)
{
    if constexpr (P < 8) {
        constexpr int D = Stripe<R, S>::D, NKO = R - 1 - CI / 4;
        constexpr int pos = Stripe<R, S>::T.pair_pos[W][CI][P];
        if constexpr (pos >= 0) {
            if constexpr (NKO >= 1) lds_read16<((pos + 0) % D) * 1024>(l[NREAD + 0], la);
            if constexpr (NKO >= 2) lds_read16<((pos + 1) % D) * 1024>(l[NREAD + 1], la);
            if constexpr (NKO >= 3) lds_read16<((pos + 2) % D) * 1024>(l[NREAD + 2], la);
            stripe_pairs_read<R, S, W, CI, P + 1, NREAD + NKO>(l, la);
        } else {
            stripe_pairs_read<R, S, W, CI, P + 1, NREAD>(l, la);
        }
    }
}
template <int R, int S, int W, int CI, int P, int NREAD>
__device__ __forceinline__ void stripe_pairs_apply(const d2 (&l)[8 * 3], const double (&r)[R][2], double (&a)[R][2])
{
    if constexpr (P < 8) {
        constexpr int JB = CI / 4, NKO = R - 1 - JB, jj = (CI % 4) * 16 + 2 * P;
        if constexpr (Stripe<R, S>::T.pair_pos[W][CI][P] >= 0) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                double z[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) z[b] = readlane64(r[JB][b], jj + h);
#pragma unroll
                for (int k = 0; k < NKO; ++k)
#pragma unroll
                    for (int b = 0; b < 2; ++b) a[JB + 1 + k][b] = fma(h ? l[NREAD + k].y : l[NREAD + k].x, z[b], a[JB + 1 + k][b]);
            }
            stripe_pairs_apply<R, S, W, CI, P + 1, NREAD + NKO>(l, r, a);
        } else {
            stripe_pairs_apply<R, S, W, CI, P + 1, NREAD>(l, r, a);
        }
    }
}

// Schedule 0.  Chunk CI and the ones behind it.  ISSUED: DMAs issued so far (list positions 0 .. ISSUED - 1); every wait leaves the DMAs
// behind the last unit it needs in flight, and every group of reads is followed by the DMAs up to A units behind it.  (A lookahead
// shorter than a group: the rest of the group is requested in front of its wait; everything before the group has been read, so its
// slots are free.)
template <int R, int S, int W, int CI, int ISSUED>
__device__ __forceinline__ void stripe_chunks(const double* __restrict__ Fw, unsigned my, unsigned la, unsigned za, const double (&r)[R][2],
                                              double (&a)[R][2], int lane, int ncols)
{
    using G = Stripe<R, S>;
    if constexpr (CI < fc_nchunk(R)) {
        if (CI * 16 >= ncols) return;                      // workgroup-uniform: a suffix of every wave's list
        constexpr int D = G::D, A = G::A, NU = G::T.n[W], JB = CI / 4, LC = CI % 4;
        constexpr int dpos = G::T.diag_pos[W][CI];
        constexpr int dend = dpos >= 0 ? dpos + fc_diag_units(R, LC) : 0;
        constexpr int issued0 = stripe_max(ISSUED, dend);
        constexpr int issued1 = dpos >= 0 ? stripe_max(issued0, stripe_min(NU, dend + A)) : ISSUED;
        if constexpr (dpos >= 0) {
            d2 l[8];
            unsigned ad[8];
            stripe_diag_addrs<R, S, LC, dpos, false>(ad, la, za, lane);
            stripe_issue<R, S, W, ISSUED, issued0>(Fw, my, lane);
            asm_wait_vmcnt<issued0 - dend>();
            if constexpr (CI == 0) MCD_T(2);
#pragma unroll
            for (int p = 0; p < 8; ++p) lds_read16<0>(l[p], ad[p]);
            lds_landed<8>(l);
            stripe_issue<R, S, W, issued0, issued1>(Fw, my, lane);
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        a[JB][b] = fma(h ? l[p].y : l[p].x, readlane64(r[JB][b], (LC * 8 + p) * 2 + h), a[JB][b]);
        }
        constexpr int pend = stripe_pairs_end<R, S, W, CI>();
        constexpr int issued1p = stripe_max(issued1, pend);
        constexpr int issued2 = pend >= 0 ? stripe_max(issued1p, stripe_min(NU, pend + A)) : issued1;
        if constexpr (pend >= 0) {
            static_assert(stripe_pairs_units<R, S, W, CI>() <= D, "a group within the ring");
            d2 l[8 * 3];
            stripe_issue<R, S, W, issued1, issued1p>(Fw, my, lane);
            asm_wait_vmcnt<issued1p - pend>();
            if constexpr (CI == 0 && dpos < 0) MCD_T(2);
            stripe_pairs_read<R, S, W, CI, 0, 0>(l, la);
            lds_landed<stripe_pairs_units<R, S, W, CI>()>(l);
            stripe_issue<R, S, W, issued1p, issued2>(Fw, my, lane);
            stripe_pairs_apply<R, S, W, CI, 0, 0>(l, r, a);
        }
        stripe_chunks<R, S, W, CI + 1, issued2>(Fw, my, la, za, r, a, lane, ncols);
    }
}

// Schedule 1.  The ds_reads of group GI's units (stripe_chunks' addresses and offsets)
template <int R, int S, int W, int GI>
__device__ __forceinline__ void stripe_group_read(d2 (&l)[8 * 3], unsigned la, unsigned za, int lane)
{
    constexpr StripeGroups Q = stripe_groups<R, S, W>();
    static_assert(stripe_group_regs<R, S, W, GI>() <= Stripe<R, S>::D, "a group within the ring");
    if constexpr (Q.diag[GI] != 0) {
        unsigned ad[8];
        stripe_diag_addrs<R, S, Q.ci[GI] % 4, Q.beg[GI], false>(ad, la, za, lane);
#pragma unroll
        for (int p = 0; p < 8; ++p) lds_read16<0>(l[p], ad[p]);
    } else {
        stripe_pairs_read<R, S, W, Q.ci[GI], 0, 0>(l, la);
    }
}
// The column broadcasts of a group out of the exchange area instead of v_readlane: both chains' r of one column in one 16-byte read,
// every lane the same address (xa: the area's LDS byte address; r of row block k, row j at xa + 1024 k + 16 j).  z[c]: the group's
// c-th column in the order of its multiply-adds.  The values are the ones the prologue's get reads, so the multiply-adds keep their bits.
template <int R, int S, int W, int CI, int P, int NZ>
__device__ __forceinline__ void stripe_pairs_bcast(d2 (&z)[16], unsigned xa)
{
    if constexpr (P < 8) {
        constexpr int JB = CI / 4, jj = (CI % 4) * 16 + 2 * P;
        if constexpr (Stripe<R, S>::T.pair_pos[W][CI][P] >= 0) {
            static_assert(NZ + 2 <= 16, "columns of a group");
            lds_read16<(JB * 64 + jj) * 16>(z[NZ], xa);
            lds_read16<(JB * 64 + jj + 1) * 16>(z[NZ + 1], xa);
            stripe_pairs_bcast<R, S, W, CI, P + 1, NZ + 2>(z, xa);
        } else {
            stripe_pairs_bcast<R, S, W, CI, P + 1, NZ>(z, xa);
        }
    }
}
template <int R, int S, int W, int CI, int P, int NREAD, int NZ>
__device__ __forceinline__ void stripe_pairs_apply_bcast(const d2 (&l)[8 * 3], const d2 (&z)[16], double (&a)[R][2])
{
    if constexpr (P < 8) {
        constexpr int JB = CI / 4, NKO = R - 1 - JB;
        if constexpr (Stripe<R, S>::T.pair_pos[W][CI][P] >= 0) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int k = 0; k < NKO; ++k)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        a[JB + 1 + k][b] = fma(h ? l[NREAD + k].y : l[NREAD + k].x, b ? z[NZ + h].y : z[NZ + h].x, a[JB + 1 + k][b]);
            stripe_pairs_apply_bcast<R, S, W, CI, P + 1, NREAD + NKO, NZ + 2>(l, z, a);
        } else {
            stripe_pairs_apply_bcast<R, S, W, CI, P + 1, NREAD, NZ>(l, z, a);
        }
    }
}
template <int ROW, int C>
__device__ __forceinline__ void stripe_diag_bcast(d2 (&z)[16], unsigned xa)
{
    if constexpr (C < 16) {
        lds_read16<(ROW + C) * 16>(z[C], xa);
        stripe_diag_bcast<ROW, C + 1>(z, xa);
    }
}
template <int R, int S, int W, int GI>
__device__ __forceinline__ void stripe_group_bcast(d2 (&z)[16], unsigned xa)
{
    constexpr StripeGroups Q = stripe_groups<R, S, W>();
    constexpr int CI = Q.ci[GI], JB = CI / 4, LC = CI % 4;
    if constexpr (Q.diag[GI] != 0) {
        stripe_diag_bcast<JB * 64 + LC * 16, 0>(z, xa);
    } else {
        stripe_pairs_bcast<R, S, W, CI, 0, 0>(z, xa);
    }
}
template <int R, int S, int W, int GI>
__device__ __forceinline__ void stripe_group_apply(const d2 (&l)[8 * 3], const d2 (&z)[16], double (&a)[R][2])
{
    constexpr StripeGroups Q = stripe_groups<R, S, W>();
    constexpr int CI = Q.ci[GI], JB = CI / 4;
    if constexpr (Q.diag[GI] != 0) {
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int b = 0; b < 2; ++b) a[JB][b] = fma(h ? l[p].y : l[p].x, b ? z[2 * p + h].y : z[2 * p + h].x, a[JB][b]);
    } else {
        stripe_pairs_apply_bcast<R, S, W, CI, 0, 0, 0>(l, z, a);
    }
}
// The schedule behind group GI: its unit reads and broadcasts have landed in L[GI & 1] and Z[GI & 1], and ISSUED DMAs are out.  If the
// early stop does not cut group GI + 1: wait for its units, read them and its broadcasts into the other register set, multiply GI
// meanwhile, then lgkmcnt(0) and the DMAs up to A units behind GI + 1 (everything up to GI + 1 has been read: their slots are free).
// The waits are stripe_chunks', every one a constexpr function of ISSUED.  A group that is cut is not touched; the branch is
// workgroup-uniform and no value in flight crosses a join.
template <int R, int S, int W, int GI, int ISSUED>
__device__ __forceinline__ void stripe_ahead(const double* __restrict__ Fw, unsigned my, unsigned la, unsigned za, unsigned xa, double (&a)[R][2],
                                             d2 (&L)[2][8 * 3], d2 (&Z)[2][16], int lane, int ncols)
{
    using G = Stripe<R, S>;
    constexpr StripeGroups Q = stripe_groups<R, S, W>();
    if constexpr (GI + 1 < Q.n) {
        if (__builtin_expect(Q.ci[GI + 1] * 16 < ncols, 1)) {   // (the cut's multiply-adds out of the straight line)
            constexpr int NU = G::T.n[W], e1 = Q.end[GI + 1];
            constexpr int issued0 = stripe_max(ISSUED, e1);
            constexpr int issued1 = stripe_max(issued0, stripe_min(NU, e1 + G::A));
            stripe_issue<R, S, W, ISSUED, issued0>(Fw, my, lane);
            asm_wait_vmcnt<issued0 - e1>();
            stripe_group_read<R, S, W, GI + 1>(L[(GI + 1) & 1], la, za, lane);
            stripe_group_bcast<R, S, W, GI + 1>(Z[(GI + 1) & 1], xa);
            MCD_SB;
            stripe_group_apply<R, S, W, GI>(L[GI & 1], Z[GI & 1], a);
            MCD_SB;
            lds_landed<stripe_group_regs<R, S, W, GI + 1>()>(L[(GI + 1) & 1]);
            lds_landed<stripe_group_cols<R, S, W, GI + 1>()>(Z[(GI + 1) & 1]);
            stripe_issue<R, S, W, issued0, issued1>(Fw, my, lane);
            stripe_ahead<R, S, W, GI + 1, issued1>(Fw, my, la, za, xa, a, L, Z, lane, ncols);
            return;
        }
    }
    stripe_group_apply<R, S, W, GI>(L[GI & 1], Z[GI & 1], a);
}
// ... and its head: the first group as stripe_chunks reads it, its broadcasts (which wait for no DMA) in front of its vmcnt wait
template <int R, int S, int W, int ISSUED>
__device__ __forceinline__ void stripe_sched(const double* __restrict__ Fw, unsigned my, unsigned la, unsigned za, unsigned xa, double (&a)[R][2],
                                             int lane, int ncols)
{
    using G = Stripe<R, S>;
    constexpr StripeGroups Q = stripe_groups<R, S, W>();
    if constexpr (Q.n > 0) {
        if (Q.ci[0] * 16 >= ncols) return;                 // workgroup-uniform: a suffix of every wave's list
        constexpr int NU = G::T.n[W], e0 = Q.end[0];
        constexpr int issued0 = stripe_max(ISSUED, e0);
        constexpr int issued1 = stripe_max(issued0, stripe_min(NU, e0 + G::A));
        d2 L[2][8 * 3], Z[2][16];
        stripe_group_bcast<R, S, W, 0>(Z[0], xa);
        stripe_issue<R, S, W, ISSUED, issued0>(Fw, my, lane);
        asm_wait_vmcnt<issued0 - e0>();
        MCD_T(2);
        stripe_group_read<R, S, W, 0>(L[0], la, za, lane);
        lds_landed<stripe_group_regs<R, S, W, 0>()>(L[0]);
        lds_landed<stripe_group_cols<R, S, W, 0>()>(Z[0]);
        stripe_issue<R, S, W, issued0, issued1>(Fw, my, lane);
        stripe_ahead<R, S, W, 0, issued1>(Fw, my, la, za, xa, a, L, Z, lane, ncols);
    }
}

// ---- schedule 2: the wave body over a form F (Stripe<R, S> above, StripeReg<R, S> below) and the plan the form asks for ----
// StripeReg: every unit by register load (MCD_STRIPE_DIAG = 1: k_logpdf_stripe_reg).  Through the ring a diagonal part goes global -> LDS
// -> register, only to be shifted by a lane offset: per part 7, 5, 3 or 1 LDS-DMAs (each with a vector address add, an M0 write and a
// literal move), eight ds_read_b128 whose addresses take three VALU instructions each, and an lgkmcnt(0) in front of the group's
// multiply-adds.  A per-lane load address says the same shift: pair pl of a part is one global_load_dwordx4 whose lanes l > 2 pl read
// base + imm + 16 l (stripe_plan.hpp, proved against fc_diag_start at compile time), and whose lanes l <= 2 pl -- zeros the stream does
// not store -- read a unit of zeros behind the stream (mvn_capi.cpp).  They are not skipped: the multiply-adds stay the same operations
// on every lane, so 0 x inf is still NaN.  One v_cmp and one v_cndmask per pair choose between 16 l and the pair's constant offset to the
// zero unit.  Every group is a register group.  No ring, no zero units in LDS: LDS holds the exchange area and, behind it, the
// hand-over of the partial sums ([w][k][c][lane], 8 bytes, as under the ring).
template <int R_, int S_>
struct StripeReg {
    static constexpr int R = R_, S = S_;
    static constexpr bool RING = false;
    static constexpr int AHEAD = kStripeRegAhead, NS = kStripeRegRing;
    static constexpr int EXCH = 0;                        // the exchange area [r | t][R][64] (d2 index)
    static constexpr int HAND = 2 * R * 64;               // the hand-over: R x 64 d2 (= [R][2][64] doubles) per wave
    static constexpr int REGION = R * 1024;               // ... in bytes
    static constexpr int LDS = HAND + S * R * 64;         // 24 KiB at R = 4, S = 4
    static_assert(stripe_plans_cover(R, S, kStripeRegAhead, true), "stripe register plan: every off-diagonal unit and every (part, pair) once");
};
// The wave's plan, proved at compile time
template <class F, int W>
struct StripePlanOf {
    static constexpr StripePlan P = stripe_plan(F::R, F::S, W, F::AHEAD, !F::RING);
    static_assert(stripe_plan_check(P, F::R, F::S, W) == 0, "stripe plan: waits, outstanding operations, slot reuse, immediates, lane addresses");
    static_assert(P.NS == F::NS && (F::RING ? P.D == Stripe<F::R, F::S>::D && P.n == Stripe<F::R, F::S>::T.n[W] : P.D == 0), "stripe plan: the rings");
};
// One request into a register slot: lane l's 16 bytes at base + voff + IMM.  Outside the compiler's bookkeeping like asm_load8: the
// covering vmcnt wait and stripe_regs_pin() before the first use.
template <int IMM>
__device__ __forceinline__ void stripe_load_reg(d2& v, unsigned voff, const char* base /* wave-uniform */)
{
    static_assert(IMM >= -4096 && IMM <= 4095, "global offset");
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=&v"(v) : "v"(voff), "s"(base), "n"(IMM) : "memory");
}
// requests [U0, U1) of the plan, each by its kind; voff = 16 lane
template <class F, int W, int U0, int U1>
__device__ __forceinline__ void stripe_issue_plan(const double* __restrict__ Fw, unsigned my, int lane, unsigned voff, d2 (&RR)[F::NS])
{
    if constexpr (U0 < U1) {
        constexpr const StripePlan& P = StripePlanOf<F, W>::P;
        constexpr int slot = P.slot[U0], base = P.base[U0];
        if constexpr (P.kind[U0] == 0) {
            stripe_dma<P.unit[U0], slot>(Fw, my, lane);
        } else if constexpr (P.thr[U0] < 0) {
            stripe_load_reg<P.imm[U0]>(RR[slot], voff, reinterpret_cast<const char*>(Fw) + base);
        } else {
            constexpr int thr = P.thr[U0];
            constexpr unsigned zoff = (unsigned)P.zoff[U0];
            unsigned v = lane > thr ? voff : zoff;         // (stripe_plan.hpp: stripe_lane_voff, which the plan's check evaluates)
            asm volatile("" : "+v"(v));                    // (formed here, like stripe_diag_addrs' addresses)
            stripe_load_reg<P.imm[U0]>(RR[slot], v, reinterpret_cast<const char*>(Fw) + base);
        }
        stripe_issue_plan<F, W, U0 + 1, U1>(Fw, my, lane, voff, RR);
    }
}
// behind the covering wait: the registers of requests [U0, U1) are the loaded values from here on
template <class F, int W, int U0, int U1>
__device__ __forceinline__ void stripe_regs_pin(d2 (&RR)[F::NS])
{
    if constexpr (U0 < U1) {
        constexpr int slot = StripePlanOf<F, W>::P.slot[U0];
        asm volatile("" : "+v"(RR[slot]));
        stripe_regs_pin<F, W, U0 + 1, U1>(RR);
    }
}
// the ds_reads of a diagonal part that came through the ring (stripe_group_read's addresses)
template <class F, int W, int GI>
__device__ __forceinline__ void stripe_diag_read(d2 (&l)[8], unsigned la, unsigned za, int lane)
{
    constexpr const StripePlan& P = StripePlanOf<F, W>::P;
    constexpr int dpos = Stripe<F::R, F::S>::T.diag_pos[W][P.gci[GI]];
    static_assert(dpos >= 0 && P.slot[P.gbeg[GI]] == dpos % Stripe<F::R, F::S>::D, "the part's ring slots");
    unsigned ad[8];
    stripe_diag_addrs<F::R, F::S, P.gci[GI] % 4, dpos, true>(ad, la, za, lane);
#pragma unroll
    for (int p = 0; p < 8; ++p) lds_read16<0>(l[p], ad[p]);
}
// the multiply-adds of stripe_pairs_apply_bcast, the units out of their register slots: group GI's requests follow each other round the
// register ring, pair after pair, row blocks ascending
template <class F, int W, int GI, int P_, int NREAD, int NZ>
__device__ __forceinline__ void stripe_pairs_apply_reg(const d2 (&RR)[F::NS], const d2 (&z)[16], double (&a)[F::R][2])
{
    if constexpr (P_ < 8) {
        constexpr const StripePlan& P = StripePlanOf<F, W>::P;
        constexpr int CI = P.gci[GI], JB = CI / 4, NKO = F::R - 1 - JB, pos = Stripe<F::R, F::S>::T.pair_pos[W][CI][P_];
        if constexpr (pos >= 0) {
            constexpr int u0 = P.gbeg[GI] + NREAD, s0 = P.slot[u0];   // (the plan's members in constant expressions only)
            static_assert(u0 + NKO <= P.gend[GI] && P.unit[u0] == Stripe<F::R, F::S>::T.unit[W][pos] && P.thr[u0] < 0, "a pair's requests");
            static_assert(P.slot[u0 + NKO - 1] == (s0 + NKO - 1) % F::NS, "a pair's slots");
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int k = 0; k < NKO; ++k) {
                    const d2& l = RR[(s0 + k) % F::NS];
#pragma unroll
                    for (int b = 0; b < 2; ++b) a[JB + 1 + k][b] = fma(h ? l.y : l.x, b ? z[NZ + h].y : z[NZ + h].x, a[JB + 1 + k][b]);
                }
            stripe_pairs_apply_reg<F, W, GI, P_ + 1, NREAD + NKO, NZ + 2>(RR, z, a);
        } else {
            stripe_pairs_apply_reg<F, W, GI, P_ + 1, NREAD, NZ>(RR, z, a);
        }
    }
}
// ... and of stripe_group_apply: a part's pair p out of l (the ring) or out of the slot of its request
template <class F, int W, int GI>
__device__ __forceinline__ void stripe_plan_apply(const d2 (&RR)[F::NS], const d2 (&l)[8], const d2 (&z)[16], double (&a)[F::R][2])
{
    constexpr const StripePlan& P = StripePlanOf<F, W>::P;
    constexpr int JB = P.gci[GI] / 4, s0 = P.slot[P.gbeg[GI]];
    if constexpr (P.gdiag[GI] != 0) {
        constexpr bool DMA = P.kind[P.gbeg[GI]] == 0;
        static_assert(DMA || (P.gend[GI] - P.gbeg[GI] == 8 && P.pair[P.gbeg[GI]] == 0), "a part's requests");
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const d2& v = DMA ? l[p] : RR[(s0 + p) % F::NS];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int b = 0; b < 2; ++b) a[JB][b] = fma(h ? v.y : v.x, b ? z[2 * p + h].y : z[2 * p + h].x, a[JB][b]);
        }
    } else {
        stripe_pairs_apply_reg<F, W, GI, 0, 0, 0>(RR, z, a);
    }
}
// The schedule behind group GI (stripe_ahead's, every count out of the plan): group GI's units are in L[GI & 1] (a part out of the ring) or
// in their register slots, its broadcasts in Z[GI & 1].  Then group GI + 1's broadcasts; an LDS-DMA group's wait and LDS reads; the
// multiply-adds of GI; a register group's wait, which needs no instruction in front of the multiply-adds; lgkmcnt(0); the requests up
// to A behind GI + 1, into the slots GI and the groups before it have left.  (A plan without LDS-DMA groups has no L.)
// There is no early stop: this schedule runs whole sweeps only (stripe_plan.hpp: stripe_form; the others run schedule 1).
// With the stop's branches every cut leaves register loads in flight into registers the compiler holds dead, and the generated code
// kept ring registers alive across the cuts' tails until it spilled them, loads in flight included.
template <class F, int W, int GI>
__device__ __forceinline__ void stripe_plan_ahead(const double* __restrict__ Fw, unsigned my, unsigned xa, unsigned voff, double (&a)[F::R][2],
                                                  d2 (&RR)[F::NS], d2 (&L)[2][8], d2 (&Z)[2][16], unsigned la, unsigned za, int lane)
{
    constexpr int R = F::R, S = F::S;
    constexpr const StripePlan& P = StripePlanOf<F, W>::P;   // (its members in constant expressions only: read at run time they are loads)
    if constexpr (GI + 1 < P.ng) {
        constexpr int N = GI + 1;
        constexpr bool DMA = P.kind[P.gbeg[N]] == 0;
        stripe_group_bcast<R, S, W, N>(Z[N & 1], xa);
        if constexpr (DMA) {
            stripe_issue_plan<F, W, P.gpost[GI], P.gpre[N]>(Fw, my, lane, voff, RR);
            asm_wait_vmcnt<P.gwait[N]>();
            stripe_diag_read<F, W, N>(L[N & 1], la, za, lane);
        }
        MCD_SB;
        stripe_plan_apply<F, W, GI>(RR, L[GI & 1], Z[GI & 1], a);
        MCD_SB;
        if constexpr (DMA) {
            lds_landed<8>(L[N & 1]);
        } else {
            stripe_issue_plan<F, W, P.gpost[GI], P.gpre[N]>(Fw, my, lane, voff, RR);
            asm_wait_vmcnt<P.gwait[N]>();
            stripe_regs_pin<F, W, P.gbeg[N], P.gend[N]>(RR);
        }
        lds_landed<stripe_group_cols<R, S, W, N>()>(Z[N & 1]);
        stripe_issue_plan<F, W, P.gpre[N], P.gpost[N]>(Fw, my, lane, voff, RR);
        stripe_plan_ahead<F, W, N>(Fw, my, xa, voff, a, RR, L, Z, la, za, lane);
    } else {
        stripe_plan_apply<F, W, GI>(RR, L[GI & 1], Z[GI & 1], a);
    }
}
// ... and its head
template <class F, int W>
__device__ __forceinline__ void stripe_plan_sched(const double* __restrict__ Fw, unsigned my, unsigned xa, unsigned voff, double (&a)[F::R][2],
                                                  d2 (&RR)[F::NS], unsigned la, unsigned za, int lane, int ncols)
{
    constexpr int R = F::R, S = F::S;
    constexpr const StripePlan& P = StripePlanOf<F, W>::P;
    // Never taken (stripe_sched_whole).  The branch ends the prologue's basic block: as one block with the sweep, the compiler's
    // scheduling ran the kernel out of its 256 registers and copied ring registers with loads in flight (tools/stripe_inflight_audit.py).
    // The prologue's register loads are out here and nothing on this path reads them, so they are waited for before the path joins
    // the wave's end, where the compiler places address arithmetic in front of the written vmcnt(0).
    if (ncols <= 0) {
        MCD_SB;
        asm_wait_vmcnt<0>();
        MCD_SB;
        return;
    }
    d2 L[2][8], Z[2][16];
    stripe_group_bcast<R, S, W, 0>(Z[0], xa);
    stripe_issue_plan<F, W, P.pro, P.gpre[0]>(Fw, my, lane, voff, RR);
    asm_wait_vmcnt<P.gwait[0]>();
    MCD_T(2);
    if constexpr (P.kind[P.gbeg[0]] == 0) {
        stripe_diag_read<F, W, 0>(L[0], la, za, lane);
        lds_landed<8>(L[0]);
    } else {
        stripe_regs_pin<F, W, P.gbeg[0], P.gend[0]>(RR);
    }
    lds_landed<stripe_group_cols<R, S, W, 0>()>(Z[0]);
    stripe_issue_plan<F, W, P.gpre[0], P.gpost[0]>(Fw, my, lane, voff, RR);
    stripe_plan_ahead<F, W, 0>(Fw, my, xa, voff, a, RR, L, Z, la, za, lane);
}

// The private prologue: x, mu and (wave 0) 1/diag of both chains in front of the first DMA: a padded row or a chain beyond the batch
// reads a clamped address and the value is dropped for mu (load_rawx)
template <int R, int S, int W>
__device__ __forceinline__ void stripe_prologue_private(const double* __restrict__ Fw, unsigned mya, const MvnView& M, const double* __restrict__ X,
                                                        int64_t ldx, int64_t b0, int64_t batch, double (&r)[R][2], double (&a)[R][2], int lane)
{
    using G = Stripe<R, S>;
    constexpr int PRO = stripe_min(G::A, G::T.n[W]);
    double xr[R][2], m[R], iv[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int row = 64 * k + lane;
        asm_load8(m[k], M.mu + row);
        if constexpr (W == 0) asm_load8(iv[k], M.invdiag + row);
        const int rc = row < M.n ? row : M.n - 1;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int64_t bc = (b0 + c < batch) ? b0 + c : batch - 1;
            asm_load8(xr[k][c], X + bc * ldx + rc);
        }
    }
    stripe_issue<R, S, W, 0, PRO>(Fw, mya, lane);
    asm_wait_vmcnt<PRO>();                                 // the loads in front of the DMAs have returned
#pragma unroll
    for (int k = 0; k < R; ++k) {
        asm volatile("" : "+v"(m[k]), "+v"(xr[k][0]), "+v"(xr[k][1]));
        if constexpr (W == 0) asm volatile("" : "+v"(iv[k]));
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int row = 64 * k + lane;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double xv = (row < M.n && b0 + c < batch) ? xr[k][c] : m[k];
            r[k][c] = xv - m[k];
            if constexpr (W == 0) a[k][c] = r[k][c] * iv[k];
            else a[k][c] = 0.0;
        }
    }
    MCD_T(1);
}

// The exchange area: r of row block k at ea + 1024 k, t at ea + 1024 (R + k) (ea: the lane's byte address in the area), .x chain 0.
// put: the owned row blocks I .. NO - 1 of wave W, r and t formed exactly as the private prologue forms them
template <int R, int S, int W, int I, int NO>
__device__ __forceinline__ void stripe_exchange_put(const double (&xr)[NO + 1][2], const double (&m)[NO + 1], const double (&iv)[NO + 1], unsigned ea,
                                                    int n, int64_t b0, int64_t batch, int lane)
{
    if constexpr (I < NO) {
        constexpr int k = W + I * S;
        const int row = 64 * k + lane;
        double rr[2], tt[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double xv = (row < n && b0 + c < batch) ? xr[I][c] : m[I];
            rr[c] = xv - m[I];
            tt[c] = rr[c] * iv[I];
        }
        lds_write16<k * 1024>(ea, d2{rr[0], rr[1]});
        lds_write16<(R + k) * 1024>(ea, d2{tt[0], tt[1]});
        stripe_exchange_put<R, S, W, I + 1, NO>(xr, m, iv, ea, n, b0, batch, lane);
    }
}
// get: all R row blocks of r (Q = 0) or t (Q = 1); lds_landed() before the first use
template <int R, int Q, int K>
__device__ __forceinline__ void stripe_exchange_get(d2 (&e)[R], unsigned ea)
{
    if constexpr (K < R) {
        lds_read16<(Q * R + K) * 1024>(e[K], ea);
        stripe_exchange_get<R, Q, K + 1>(e, ea);
    }
}

// The shared prologue: the same loads, selection and operations, but only for the row blocks k = W, W + S, ... < R this wave owns
// (four loads each); r and t = r invdiag go through the exchange area, one LDS-only barrier, every wave reads r and wave 0 t.
// GETR = false (schedules 1 and 2, which broadcast r out of the exchange area): r is not read back into registers.
// burst(): the wave's first PRO requests (and whatever else the schedule wants done while the loads are out).
template <int R, int S, int W, bool GETR, int PRO, class Burst>
__device__ __forceinline__ void stripe_prologue_shared(unsigned ea, const MvnView& M, const double* __restrict__ X, int64_t ldx, int64_t b0,
                                                       int64_t batch, double (&r)[R][2], double (&a)[R][2], int lane, Burst burst)
{
    constexpr int NO = W < R ? (R - W + S - 1) / S : 0;    // row blocks owned
    double xr[NO + 1][2], m[NO + 1], iv[NO + 1];
#pragma unroll
    for (int i = 0; i < NO; ++i) {
        const int row = 64 * (W + i * S) + lane;
        asm_load8(m[i], M.mu + row);
        asm_load8(iv[i], M.invdiag + row);
        const int rc = row < M.n ? row : M.n - 1;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int64_t bc = (b0 + c < batch) ? b0 + c : batch - 1;
            asm_load8(xr[i][c], X + bc * ldx + rc);
        }
    }
    burst();
    asm_wait_vmcnt<PRO>();                                 // the loads in front of the burst have returned
#pragma unroll
    for (int i = 0; i < NO; ++i) asm volatile("" : "+v"(m[i]), "+v"(iv[i]), "+v"(xr[i][0]), "+v"(xr[i][1]));
    MCD_T(1);
    stripe_exchange_put<R, S, W, 0, NO>(xr, m, iv, ea, M.n, b0, batch, lane);
    lds_barrier();                                         // (lgkmcnt only: the loads stay in flight)
    d2 e[R], et[R];
    if constexpr (GETR) stripe_exchange_get<R, 0, 0>(e, ea);
    if constexpr (W == 0) stripe_exchange_get<R, 1, 0>(et, ea);
    if constexpr (GETR) lds_landed<R>(e);
    if constexpr (W == 0) lds_landed<R>(et);
#pragma unroll
    for (int k = 0; k < R; ++k)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if constexpr (GETR) r[k][c] = c ? e[k].y : e[k].x;
            if constexpr (W == 0) a[k][c] = c ? et[k].y : et[k].x;
            else a[k][c] = 0.0;
        }
    MCD_T(5);
}

// ---- the finish per chain (MCD_STRIPE_FINISH = 1, the default; schedule 2 only: k_logpdf_stripe_fin, k_logpdf_stripe_reg) ----
// Behind the hand-over barrier wave 0 alone forms z for both chains and runs finish_ll<R, 2>, chain 0 to its store before chain 1's
// reduction begins, while three waves idle.  Here wave kStripeFinishWave + c finishes chain c: z_k = ((a0_k + a1_k) + a2_k) + a3_k in
// wave order, its own partial out of its registers; s = fma(z_k, z_k, s), k ascending; wave_sum; ll = c + (-0.5)(logdet + q) -- the
// operations of finish_ll for that chain in its order, so the bits are that finish's.  One barrier as there, reached by every
// wave on every path.
//   * The hand-over keeps the 8-byte layout [w][k][c][lane] in the waves' regions.  A finishing wave wants one chain only: a
//     ds_read_b64 at 8 lane + const covers all 64 banks once per 32 lanes (2 LDS cycles, no conflict).  With {c0, c1} in 16-byte slots
//     it would read twice the bytes into twice the registers (ds_read_b128: 4 cycles) to drop half, and one ds_write_b128 moves its
//     operands no faster than the two ds_write_b64 it replaces (13 cycles against 2 x 6).
//   * A wave stores only what another wave reads: both chains, or the chain it does not finish.
//   * The reads are asm (the compiler put a wait of its own behind every few of them): all issued, one lgkmcnt(0).
//   * c and logdet: kernel arguments 10 and 11 lie behind the preloaded dwords.  The finishing waves fetch them at entry, by an asm
//     scalar load the compiler cannot sink in front of the barrier, and wait for them behind the wave sum.  (Any lgkmcnt(0) covers
//     the load, and every LDS wait of this kernel is one; the exchange barrier's is the first.)
//   * Waves 0 and 1 finish: they are the last at the barrier, and so store one chain's partials in front of it, not two.  Measured
//     (profiles/r19_stripe_finish_ab.txt): waves 2 and 3 (-DMCD_STRIPE_FINISH_WAVE=2) 4.509 us per launch against 4.472.
//   * Measured and not kept (docs/experiments/r19_stripe_x_first_late_t.diff): x loaded in front of mu and 1/diag (+0.04 us), and
//     wave 0's t left in flight until the first group's wait (level).
#ifndef MCD_STRIPE_FINISH_WAVE
#define MCD_STRIPE_FINISH_WAVE 0
#endif
constexpr int kStripeFinishWave = MCD_STRIPE_FINISH_WAVE;  // chain c of the workgroup is finished by wave kStripeFinishWave + c
constexpr int kStripeArgC = 0x40;                          // byte offset of c (logdet: + 8) in the kernel's arguments (k_logpdf.hip)
typedef unsigned stripe_u4 __attribute__((ext_vector_type(4)));
// c and logdet into four SGPRs, outside the compiler's bookkeeping like asm_load8: stripe_args_landed() before the first use
__device__ __forceinline__ void stripe_args_load(stripe_u4& v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx4 %0, %1, %2" : "=&s"(v) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "n"(kStripeArgC) : "memory");
#endif
}
__device__ __forceinline__ void stripe_args_landed(stripe_u4& v)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v)::"memory");
}
template <int OFF>
__device__ __forceinline__ void lds_read8(double& v, unsigned addr)
{
    static_assert(OFF >= 0 && OFF < 65536, "ds offset");
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
}
// REGION: bytes from one wave's partials to the next wave's
template <int R, int S, int W, int C, int I, int REGION>
__device__ __forceinline__ void stripe_finish_get(double (&p)[S][R], unsigned pa)
{
    if constexpr (I < S * R) {
        constexpr int w = I / R, k = I % R;
        if constexpr (w != W) lds_read8<(k * 2 + C) * 512>(p[w][k], pa + (unsigned)(w * REGION));   // (a region may be 32 KiB: past the offset field)
        stripe_finish_get<R, S, W, C, I + 1, REGION>(p, pa);
    }
}
// chain C of the workgroup, by wave W: pa = the hand-over's LDS byte address + 8 lane; cl = c and logdet in flight
template <int R, int S, int W, int C, int REGION>
__device__ __forceinline__ void stripe_finish_chain(const double (&a)[R][2], unsigned pa, stripe_u4& cl, int64_t b0, int64_t batch,
                                                    double* __restrict__ ll, int lane)
{
    double p[S][R];
    stripe_finish_get<R, S, W, C, 0, REGION>(p, pa);       // every other wave's partials of chain C, one wait
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int w = 0; w < S; ++w)
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (w != W) asm volatile("" : "+v"(p[w][k]));
    MCD_T(7);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        double z = W == 0 ? a[k][C] : p[0][k];
#pragma unroll
        for (int w = 1; w < S; ++w) z = z + (w == W ? a[k][C] : p[w][k]);
        s = fma(z, z, s);
    }
    const double q = wave_sum(s);
    stripe_args_landed(cl);
    const double c = __hiloint2double((int)cl.y, (int)cl.x), logdet = __hiloint2double((int)cl.w, (int)cl.z);
    if (lane == 0 && b0 + C < batch) ll[b0 + C] = c + (-0.5) * (logdet + q);   // (finish_ll's line)
}

// The wave bodies, as types for stripe_dispatch: wave W of the workgroup runs Body::run<W>.
// Schedule 2's wave over the form F.  PER_CHAIN: wave kStripeFinishWave + c finishes chain c; otherwise wave 0 finishes both.
// lds: the kernel's LDS, F::LDS d2.  The wave's hand-over region is, under the ring form, its ring.
template <class F, bool PER_CHAIN>
struct StripeWavePlan {
static constexpr int S = F::S;
template <int W>
static __device__ __forceinline__ void run(const double* __restrict__ Fw, d2* lds, const MvnView& M, const double* __restrict__ X, int64_t ldx,
                                           int64_t b0, int64_t batch, int ncols, double* __restrict__ ll, int lane)
{
    constexpr int R = F::R;
    constexpr const StripePlan& P = StripePlanOf<F, W>::P;
    static_assert(kStripeFinishWave >= 0 && kStripeFinishWave + 2 <= S, "MCD_STRIPE_FINISH_WAVE");
    constexpr int C = PER_CHAIN ? W - kStripeFinishWave : -1;   // the chain this wave finishes, if 0 or 1
    constexpr bool FIN = C == 0 || C == 1;
    stripe_u4 cl;
    if constexpr (FIN) stripe_args_load(cl);
    d2* my = lds + F::HAND + W * (F::REGION / 16);
    const unsigned voff = 16u * (unsigned)lane, xa = lds_addr(lds + F::EXCH);
    unsigned mya = 0, la = 0, za = 0;
    if constexpr (F::RING) {
        d2* zu = lds + F::ZERO + W * 64;
        zu[lane] = d2{0.0, 0.0};
        mya = lds_addr(my), la = mya + voff, za = lds_addr(zu) + voff;
    }
    double r[R][2], a[R][2];
    d2 RR[F::NS];
    stripe_prologue_shared<R, S, W, false, P.pro>(xa + voff, M, X, ldx, b0, batch, r, a, lane,
                                                  [&]() __attribute__((always_inline)) { stripe_issue_plan<F, W, 0, P.pro>(Fw, mya, lane, voff, RR); });
    stripe_plan_sched<F, W>(Fw, mya, xa, voff, a, RR, la, za, lane, ncols);
    MCD_T(3);
    MCD_SB;                                                // (nothing of the hand-over moves in front of the wait: the path that skips the
    asm_wait_vmcnt<0>();                                   //  sweep joins here, and the audit of the generated code follows every path)
    MCD_SB;
    double* part = reinterpret_cast<double*>(my);
    if constexpr (PER_CHAIN) {
#pragma unroll
        for (int k = 0; k < R; ++k)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (c != C) part[(k * 2 + c) * 64 + lane] = a[k][c];
        lds_barrier();
        if constexpr (FIN) {
            MCD_T(6);
            stripe_finish_chain<R, S, W, C, F::REGION>(a, lds_addr(lds + F::HAND) + 8u * (unsigned)lane, cl, b0, batch, ll, lane);
            MCD_T(4);
        }
    } else {
        if constexpr (W > 0) {
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int c = 0; c < 2; ++c) part[(k * 2 + c) * 64 + lane] = a[k][c];
        }
        lds_barrier();
        if constexpr (W == 0) {
#pragma unroll
            for (int w = 1; w < S; ++w) {
                const double* pw = reinterpret_cast<const double*>(lds + w * Stripe<R, S>::D * 64);
#pragma unroll
                for (int k = 0; k < R; ++k)
#pragma unroll
                    for (int c = 0; c < 2; ++c) a[k][c] = a[k][c] + pw[(k * 2 + c) * 64 + lane];
            }
            finish_ll<R, 2>(a, M, b0, batch, ll, lane);
            MCD_T(4);
        }
    }
}
};
// Schedules 0 and 1, under the private (SH = false, schedule 0 only) or the shared prologue
template <int R, int S_, bool SH, int SC>
struct StripeWaveLoop {
static constexpr int S = S_;
static_assert(SH || SC == 0, "the schedule goes with the shared prologue");
static_assert(SC == 0 || SC == 1, "MCD_STRIPE_SCHED");
template <int W>
static __device__ __forceinline__ void run(const double* __restrict__ Fw, d2* ring, const MvnView& M, const double* __restrict__ X, int64_t ldx,
                                           int64_t b0, int64_t batch, int ncols, double* __restrict__ ll, int lane)
{
    using G = Stripe<R, S>;
    {
        constexpr int D = G::D, NU = G::T.n[W], PRO = stripe_min(G::A, NU);
        d2* my = ring + W * D * 64;
        d2* zu = ring + G::ZERO + W * 64;
        zu[lane] = d2{0.0, 0.0};
        const unsigned mya = lds_addr(my);
        double r[R][2], a[R][2];
        if constexpr (SH)
            stripe_prologue_shared<R, S, W, SC == 0, PRO>(lds_addr(ring + G::EXCH) + 16u * (unsigned)lane, M, X, ldx, b0, batch, r, a, lane,
                                                          [&]() __attribute__((always_inline)) { stripe_issue<R, S, W, 0, PRO>(Fw, mya, lane); });
        else stripe_prologue_private<R, S, W>(Fw, mya, M, X, ldx, b0, batch, r, a, lane);
        const unsigned la = mya + 16u * (unsigned)lane;
        const unsigned za = lds_addr(zu) + 16u * (unsigned)lane;
        if constexpr (SC != 0) stripe_sched<R, S, W, PRO>(Fw, mya, la, za, lds_addr(ring + G::EXCH), a, lane, ncols);
        else stripe_chunks<R, S, W, 0, PRO>(Fw, mya, la, za, r, a, lane, ncols);
        MCD_T(3);
        asm_wait_vmcnt<0>();
        double* part = reinterpret_cast<double*>(my);
        if constexpr (W > 0) {
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int c = 0; c < 2; ++c) part[(k * 2 + c) * 64 + lane] = a[k][c];
        }
        lds_barrier();
        if constexpr (W == 0) {
#pragma unroll
            for (int w = 1; w < S; ++w) {
                const double* pw = reinterpret_cast<const double*>(ring + w * Stripe<R, S>::D * 64);
#pragma unroll
                for (int k = 0; k < R; ++k)
#pragma unroll
                    for (int c = 0; c < 2; ++c) a[k][c] = a[k][c] + pw[(k * 2 + c) * 64 + lane];
            }
            finish_ll<R, 2>(a, M, b0, batch, ll, lane);
            MCD_T(4);
        }
    }
}

};
// the wave body of k_logpdf_stripe<R, S, SH, SC>
template <int R, int S, bool SH, int SC>
using StripeWaveOf = std::conditional_t<SC == 2, StripeWavePlan<Stripe<R, S>, false>, StripeWaveLoop<R, S, SH, SC>>;
template <class Body, int W = 0>
__device__ __forceinline__ void stripe_dispatch(int wave, const double* __restrict__ Fw, d2* lds, const MvnView& M, const double* __restrict__ X,
                                                int64_t ldx, int64_t b0, int64_t batch, int ncols, double* __restrict__ ll, int lane)
{
    if (wave == W) {
        Body::template run<W>(Fw, lds, M, X, ldx, b0, batch, ncols, ll, lane);
    } else {
        if constexpr (W + 1 < Body::S) stripe_dispatch<Body, W + 1>(wave, Fw, lds, M, X, ldx, b0, batch, ncols, ll, lane);
    }
}

}  // namespace mcd
