#pragma once
// stripe_device.hpp -- the inverse stream (FS = 3) of the raw-x log-density at R = 3, 4 and up to 512 chains: z = W (x - mu) with
// W = L^-1 read from Fw (fc_layout.hpp) by S "stripe" waves, no loader waves and no barrier inside the sweep.
//
//   * One workgroup serves 2 chains; every stripe wave holds both (r[R][2] and the accumulators a[R][2]) and multiplies only the units
//     dealt to it (stripe_deal.hpp).  Nothing forces two waves to read the same bytes, so each wave loads its own units by LDS-DMA
//     into a ring of D units that only it reads: the u-th unit of its list lives at slot u mod D.
//   * Ordering inside a wave is the wave's own counters.  A wave's LDS-DMAs land in issue order, so once vmcnt is down to the number
//     of DMAs issued behind unit u, unit u is in LDS; the DMA of unit u + D is issued once the ds_reads of unit u have returned.
//     The compiler does not know which DMA a ds_read depends on and would wait for all of them, so the ring is read by ds_read_b128
//     in asm statements, with the waits written out; for the same reason the loads of x, mu and 1/diag, issued before the first
//     DMA, are asm loads waited for by count.
//   * Order of additions, fixed: within a wave a row's additions follow the wave's list (chunk after chunk; a chunk's diagonal part
//     pair by pair, then its off-diagonal pairs, per pair column 2p before 2p + 1, row blocks ascending).  Wave 0's accumulators
//     start at r_i invdiag_i, the others at 0.  After its last unit each wave w > 0 stores a into its own ring region; one barrier;
//     wave 0 forms z_i = ((a0 + a1) + a2) + ... in wave order and runs finish_ll.  The bits belong to the S the library is built with
//     (kStripeWaves): another S deals the units differently.
//   * Every wave's code is its own instantiation (W is a template parameter): list positions, ring slots, wait counts and the
//     v_readlane lane selects of the column broadcasts are immediates.
//   * The waves end on vmcnt(0): nothing of one launch is in flight into LDS when the next one starts.  A sweep that stops early
//     (ncols < 64 R) has requested up to D units behind the cut; they land in the wave's own ring and are never read.
#include "mvn_device.hpp"
#include "stripe_deal.hpp"

namespace mcd {

#ifndef MCD_STRIPE_WAVES
#define MCD_STRIPE_WAVES 4
#endif
constexpr int kStripeWaves = MCD_STRIPE_WAVES;

template <int R, int S>
struct Stripe {
    static_assert((R == 3 || R == 4) && (S == 4 || S == 8), "stripe kernel: R = 3, 4; S = 4, 8");
    // ring units per wave: S D KiB + the waves' zero units within 160 KiB, and x loads + D DMAs within the 6 bits of vmcnt
    static constexpr int D = 128 / S;
    static constexpr int ZERO = S * D * 64;               // the waves' zero units (d2 index)
    static constexpr int D2 = ZERO + S * 64;
    static_assert(D2 * 16 <= 160 * 1024, "LDS");
    static_assert(4 * R + D < 64, "vmcnt");
    static constexpr StripeDeal T = stripe_deal(R, S);
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

// the DMAs of list positions [U0, U1); my: the LDS byte address of the wave's ring (an integer: a pointer converted back from the
// generic address space would carry a null check into every M0 write)
template <int R, int S, int W, int U0, int U1>
__device__ __forceinline__ void stripe_issue(const double* __restrict__ Fw, unsigned my, int lane)
{
    if constexpr (U0 < U1) {
#if defined(__HIP_DEVICE_COMPILE__)                       // (an LDS pointer is 32 bits wide on the device only)
        constexpr int g = Stripe<R, S>::T.unit[W][U0];
        const __attribute__((address_space(1))) d2* src =
            (const __attribute__((address_space(1))) d2*)reinterpret_cast<const d2*>(Fw) + ((size_t)g * 64 + lane);
        __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(my + (U0 % Stripe<R, S>::D) * 1024u), 16, 0, 0);
#endif
        stripe_issue<R, S, W, U0 + 1, U1>(Fw, my, lane);
    }
}

constexpr int stripe_min(int a, int b) { return a < b ? a : b; }

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
// the list position behind the last of wave W's off-diagonal pairs of chunk CI (-1: none), and their units
template <int R, int S, int W, int CI>
constexpr int stripe_pairs_end()
{
    int e = -1;
    for (int p = 0; p < 8; ++p)
        if (Stripe<R, S>::T.pair_pos[W][CI][p] >= 0) e = Stripe<R, S>::T.pair_pos[W][CI][p] + (R - 1 - CI / 4);
    return e;
}
template <int R, int S, int W, int CI>
constexpr int stripe_pairs_units()
{
    int n = 0;
    for (int p = 0; p < 8; ++p)
        if (Stripe<R, S>::T.pair_pos[W][CI][p] >= 0) n += R - 1 - CI / 4;
    return n;
}

// Chunk CI and the ones behind it.  ISSUED: DMAs issued so far (list positions 0 .. ISSUED - 1); every wait leaves the DMAs behind the
// last unit it needs in flight, and every group of reads is followed by the DMAs into the slots it has just freed.
template <int R, int S, int W, int CI, int ISSUED>
__device__ __forceinline__ void stripe_chunks(const double* __restrict__ Fw, unsigned my, unsigned la, unsigned za, const double (&r)[R][2],
                                              double (&a)[R][2], int lane, int ncols)
{
    using G = Stripe<R, S>;
    if constexpr (CI < fc_nchunk(R)) {
        if (CI * 16 >= ncols) return;                      // workgroup-uniform: a suffix of every wave's list
        constexpr int D = G::D, NU = G::T.n[W], JB = CI / 4, LC = CI % 4;
        constexpr int dpos = G::T.diag_pos[W][CI];
        constexpr int dend = dpos >= 0 ? dpos + fc_diag_units(R, LC) : 0;
        constexpr int issued1 = dpos >= 0 ? stripe_min(NU, dend + D) : ISSUED;
        if constexpr (dpos >= 0) {
            // the diagonal part: pair p's lanes 2 pl + 1 .. 63 lie back to back in the part, the others read the wave's zero unit
            constexpr bool WRAP = dpos % D + fc_diag_units(R, LC) > D;
            d2 l[8];
            unsigned ad[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int pl = LC * 8 + p;
                int i = (dpos % D) * 64 + fc_diag_start(R, LC, p) - (2 * pl + 1) + lane;
                if (WRAP) i = i >= D * 64 ? i - D * 64 : i;
                ad[p] = lane > 2 * pl ? la - 16u * (unsigned)lane + 16u * (unsigned)i : za;
            }
            asm_wait_vmcnt<ISSUED - dend>();
            if constexpr (CI == 0) MCD_T(2);
#pragma unroll
            for (int p = 0; p < 8; ++p) lds_read16<0>(l[p], ad[p]);
            lds_landed<8>(l);
            stripe_issue<R, S, W, ISSUED, issued1>(Fw, my, lane);
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        a[JB][b] = fma(h ? l[p].y : l[p].x, readlane64(r[JB][b], (LC * 8 + p) * 2 + h), a[JB][b]);
        }
        constexpr int pend = stripe_pairs_end<R, S, W, CI>();
        constexpr int issued2 = pend >= 0 ? stripe_min(NU, pend + D) : issued1;
        if constexpr (pend >= 0) {
            d2 l[8 * 3];
            asm_wait_vmcnt<issued1 - pend>();
            if constexpr (CI == 0 && dpos < 0) MCD_T(2);
            stripe_pairs_read<R, S, W, CI, 0, 0>(l, la);
            lds_landed<stripe_pairs_units<R, S, W, CI>()>(l);
            stripe_issue<R, S, W, issued1, issued2>(Fw, my, lane);
            stripe_pairs_apply<R, S, W, CI, 0, 0>(l, r, a);
        }
        stripe_chunks<R, S, W, CI + 1, issued2>(Fw, my, la, za, r, a, lane, ncols);
    }
}

template <int R, int S, int W>
__device__ __forceinline__ void stripe_wave(const double* __restrict__ Fw, d2* ring, const MvnView& M, const double* __restrict__ X, int64_t ldx,
                                            int64_t b0, int64_t batch, int ncols, double* __restrict__ ll, int lane)
{
    using G = Stripe<R, S>;
    constexpr int D = G::D, NU = G::T.n[W], PRO = stripe_min(D, NU);
    d2* my = ring + W * D * 64;
    d2* zu = ring + G::ZERO + W * 64;
    zu[lane] = d2{0.0, 0.0};
    // x, mu and (wave 0) 1/diag of both chains in front of the first DMA: a padded row or a chain beyond the batch reads a clamped
    // address and the value is dropped for mu (load_rawx)
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
    const unsigned mya = lds_addr(my);
    stripe_issue<R, S, W, 0, PRO>(Fw, mya, lane);
    asm_wait_vmcnt<PRO>();                                 // the loads in front of the DMAs have returned
#pragma unroll
    for (int k = 0; k < R; ++k) {
        asm volatile("" : "+v"(m[k]), "+v"(xr[k][0]), "+v"(xr[k][1]));
        if constexpr (W == 0) asm volatile("" : "+v"(iv[k]));
    }
    double r[R][2], a[R][2];
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
    const unsigned la = mya + 16u * (unsigned)lane;
    const unsigned za = lds_addr(zu) + 16u * (unsigned)lane;
    stripe_chunks<R, S, W, 0, PRO>(Fw, mya, la, za, r, a, lane, ncols);
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
            const double* pw = reinterpret_cast<const double*>(ring + w * D * 64);
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int c = 0; c < 2; ++c) a[k][c] = a[k][c] + pw[(k * 2 + c) * 64 + lane];
        }
        finish_ll<R, 2>(a, M, b0, batch, ll, lane);
        MCD_T(4);
    }
}

template <int R, int S, int W>
__device__ __forceinline__ void stripe_dispatch(int wave, const double* __restrict__ Fw, d2* ring, const MvnView& M, const double* __restrict__ X,
                                                int64_t ldx, int64_t b0, int64_t batch, int ncols, double* __restrict__ ll, int lane)
{
    if (wave == W) {
        stripe_wave<R, S, W>(Fw, ring, M, X, ldx, b0, batch, ncols, ll, lane);
    } else {
        if constexpr (W + 1 < S) stripe_dispatch<R, S, W + 1>(wave, Fw, ring, M, X, ldx, b0, batch, ncols, ll, lane);
    }
}

}  // namespace mcd
