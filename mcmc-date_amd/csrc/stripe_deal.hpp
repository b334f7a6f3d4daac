// stripe_deal.hpp -- which stripe wave of the inverse-stream kernel (stripe_device.hpp: k_logpdf_stripe) owns which 1-KiB unit of the
// inverse stream Fw (fc_layout.hpp: the compact layout, host_factor.cpp: pack_inverse_forward); plain constexpr C++, shared by the
// host (sweep_launch.cpp: mcd_stripe_deal_selftest_) and the device.
//
// z = W r has no dependent column chain, so the S waves of a workgroup each multiply a share of W of their own, loaded by that wave
// into LDS that only it reads.  The stream is dealt in PIECES of whole units:
//   * the diagonal part of a chunk (7, 5, 3 or 1 units holding the chunk's 8 column pairs: a pair's lanes straddle units, so the
//     part stays whole), and
//   * the off-diagonal units of one column pair (R - 1 - JB consecutive units, row blocks JB + 1 .. R - 1).
// Off-diagonal pair P (counted over the whole stream, 8 per chunk) goes to wave P mod S.  The diagonal parts go, largest first (all
// 7-unit parts in block order, then the 5-, 3- and 1-unit parts), each to the wave that holds the fewest diagonal units so far; a tie
// goes to the first such wave counted from wave (JB + LC) mod S on, so that a block's parts go to different waves (S = 4, R = 4: wave w
// takes part (w - JB) mod 4 of block JB) and no wave is left with the whole last block behind the others' last unit.  At R = 4 every
// wave ends with 256 / S units; at R = 3 the waves differ by at most 2 units.
// A wave's LIST is its pieces in stream order -- chunk after chunk, a chunk's diagonal part before its pairs -- which is ascending
// column order: a sweep that stops at ncols < 64 R cuts a suffix of every list (the chunks with 16 CI >= ncols).
#pragma once

#include "fc_layout.hpp"

namespace mcd {

constexpr int kStripeMaxWaves = 8;
constexpr int kStripeMaxUnits = 80;                       // of one wave's list (R = 4, S = 4: 64)

struct StripeDeal {
    int n[kStripeMaxWaves];                               // units of wave w's list
    int unit[kStripeMaxWaves][kStripeMaxUnits];           // the u-th unit of the list: its index in Fw
    int diag_pos[kStripeMaxWaves][16];                    // list position of chunk ci's diagonal part, -1: another wave's
    int pair_pos[kStripeMaxWaves][16][8];                 // list position of the first off-diagonal unit of pair p of chunk ci, -1
    int diag_owner[16];
};

constexpr StripeDeal stripe_deal(int R, int S)
{
    StripeDeal d{};
    const int CPB = fc_cpb(R), CP = fc_cp(R), NC = fc_nchunk(R);
    int load[kStripeMaxWaves] = {};
    for (int lc = 0; lc < CPB; ++lc)
        for (int jb = 0; jb < R; ++jb) {
            int w = (jb + lc) % S;
            for (int i = 1; i < S; ++i)
                if (load[(jb + lc + i) % S] < load[w]) w = (jb + lc + i) % S;
            d.diag_owner[jb * CPB + lc] = w;
            load[w] += fc_diag_units(R, lc);
        }
    for (int w = 0; w < S; ++w) {
        int u = 0;
        for (int ci = 0; ci < 16; ++ci) {
            d.diag_pos[w][ci] = -1;
            for (int p = 0; p < 8; ++p) d.pair_pos[w][ci][p] = -1;
        }
        for (int ci = 0; ci < NC; ++ci) {
            const int base = fc_chunk_base(R, ci), du = fc_diag_units(R, ci % CPB), nko = R - 1 - ci / CPB;
            if (d.diag_owner[ci] == w) {
                d.diag_pos[w][ci] = u;
                for (int i = 0; i < du; ++i) d.unit[w][u++] = base + i;
            }
            for (int p = 0; p < CP && nko > 0; ++p)
                if ((ci * CP + p) % S == w) {
                    d.pair_pos[w][ci][p] = u;
                    for (int k = 0; k < nko; ++k) d.unit[w][u++] = base + du + p * nko + k;
                }
        }
        d.n[w] = u;
    }
    return d;
}

// every unit of Fw has exactly one owner, and the waves' shares are as even as stated above
constexpr bool stripe_deal_ok(int R, int S)
{
    const StripeDeal d = stripe_deal(R, S);
    const int total = fc_total_units(R);
    int seen[256] = {};
    int lo = d.n[0], hi = d.n[0], sum = 0;
    for (int w = 0; w < S; ++w) {
        if (d.n[w] > kStripeMaxUnits) return false;
        for (int u = 0; u < d.n[w]; ++u) {
            if (d.unit[w][u] < 0 || d.unit[w][u] >= total || seen[d.unit[w][u]]++) return false;
        }
        lo = d.n[w] < lo ? d.n[w] : lo;
        hi = d.n[w] > hi ? d.n[w] : hi;
        sum += d.n[w];
    }
    if (sum != total) return false;
    if (R == 4) return lo == hi;
    return 4 * S * (hi - lo) <= total;                    // hi - lo <= a quarter of the mean
}
static_assert(stripe_deal_ok(4, 4) && stripe_deal_ok(4, 8) && stripe_deal_ok(3, 4) && stripe_deal_ok(3, 8), "stripe deal");

}  // namespace mcd
