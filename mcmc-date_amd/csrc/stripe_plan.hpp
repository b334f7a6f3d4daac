// stripe_plan.hpp -- the request plan of one stripe wave of the inverse-stream kernel under schedule 2 (stripe_device.hpp), and the form
// a launch of the stripe kernel takes; plain constexpr C++, shared by the host (sweep_launch.cpp: mcd_stripe_plan_selftest_,
// mcd_stripe_regplan_selftest_; tests/cpp/test_stripe_plan.cpp, test_stripe_plan_reg.cpp) and the device.
//
// A wave works through the GROUPS of its list (stripe_deal.hpp) in list order: a chunk's diagonal part, or the wave's off-diagonal pairs
// of a chunk (stripe_groups).  A plan position is a REQUEST, of one of two kinds:
//   * LDS-DMA: one unit of a diagonal part into slot u mod D of the wave's ring; the part's column pairs straddle units and are read
//     back with a lane shift;
//   * register load: one global_load_dwordx4 into slot (register loads before it) mod NS of a register ring.  Lane l reads
//     Fw + base + imm + 16 l: a scalar base, the lane's vector offset and a 13-bit immediate.
//       - An off-diagonal unit is one such load: lane l's 16 bytes are the two entries of row l.  One base (Fw + 8192 k + 4096) serves
//         the eight units 8 k .. 8 k + 7.
//       - A diagonal part, where the plan takes it by register load (diag_by_reg: k_logpdf_stripe_reg), is eight, one per column pair:
//         pair pl = 8 LC + p keeps the lanes 2 pl + 1 .. 63 of its diagonal unit, back to back from lane fc_diag_start(R, LC, p) of the
//         part on, so lane l > thr = 2 pl finds its 16 bytes at part + 16 (fc_diag_start(R, LC, p) - (2 pl + 1)) + 16 l -- the element
//         the lane-shifted ring read picks.  A lane l <= thr, whose entries are zeros the stream does not store, reads a unit of zeros
//         that stands behind the stream on the device (fc_total_units(R) x 1024 bytes from Fw on): its vector offset is zoff = (that
//         address) - (base + imm) instead of 16 l.  One scalar base per part: the eight offsets span less than the immediate's 13 bits.
// Both kinds count on vmcnt in issue order, so a wait is a count over the mixed sequence.  For every group the plan holds what is issued
// in front of its wait (pre), the vmcnt of the wait, and what is issued behind it (post: up to A requests behind the group).
// stripe_plan_check replays the sequence and proves what the device code relies on; the device static_asserts it.
#pragma once

#include "stripe_deal.hpp"

namespace mcd {

constexpr int kStripeRegSlots = 24;                       // register ring beside the LDS ring: the lookahead + the largest off-diagonal group
constexpr int kStripeRegRing = 32;                        // ... with the parts by register load: the lookahead + a part's 8 + a group
constexpr int kStripeMaxGroups = 32;
constexpr int kStripeMaxReq = 96;                         // requests of one wave (R = 4, S = 4, parts by register load: 48 + 4 x 8 = 80)
constexpr int kStripeBaseSpan = 8192, kStripeBaseBias = 4096;   // bytes of Fw one scalar base covers; the base sits in their middle
#ifndef MCD_STRIPE_REG_AHEAD
#define MCD_STRIPE_REG_AHEAD 12
#endif
constexpr int kStripeRegAhead = MCD_STRIPE_REG_AHEAD;     // the lookahead of k_logpdf_stripe_reg, in requests (measured 10 .. 16)

constexpr int stripe_min(int a, int b) { return a < b ? a : b; }
constexpr int stripe_max(int a, int b) { return a > b ? a : b; }

// The groups of wave W, in list order: chunk, 1 for its diagonal part, list positions [beg, end)
struct StripeGroups {
    int n;
    int ci[kStripeMaxGroups], diag[kStripeMaxGroups], beg[kStripeMaxGroups], end[kStripeMaxGroups];
};
constexpr StripeGroups stripe_groups(const StripeDeal& d, int R, int W)
{
    StripeGroups q{};
    for (int ci = 0; ci < fc_nchunk(R); ++ci) {
        if (d.diag_pos[W][ci] >= 0) {
            q.ci[q.n] = ci, q.diag[q.n] = 1, q.beg[q.n] = d.diag_pos[W][ci];
            q.end[q.n++] = d.diag_pos[W][ci] + fc_diag_units(R, ci % fc_cpb(R));
        }
        int beg = -1, end = -1;
        for (int p = 0; p < fc_cp(R); ++p)
            if (d.pair_pos[W][ci][p] >= 0) {
                if (beg < 0) beg = d.pair_pos[W][ci][p];
                end = d.pair_pos[W][ci][p] + (R - 1 - ci / fc_cpb(R));
            }
        if (end >= 0) q.ci[q.n] = ci, q.diag[q.n] = 0, q.beg[q.n] = beg, q.end[q.n++] = end;
    }
    return q;
}

struct StripePlan {
    int n, lead, pro, A, D, NS;                           // requests; leading loads of the prologue; its burst; lookahead; ring units; register slots
    int kind[kStripeMaxReq];                              // 0: LDS-DMA, 1: register load
    int slot[kStripeMaxReq];                              // ring slot (u mod D) or register slot
    int base[kStripeMaxReq], imm[kStripeMaxReq];          // register loads: lane l reads Fw + base + imm + 16 l, unless l <= thr
    int thr[kStripeMaxReq];                               // -1: every lane; 2 pl: lanes 0 .. 2 pl read zeros
    int zoff[kStripeMaxReq];                              // the vector offset of those lanes: base + imm + zoff = the zero unit
    int unit[kStripeMaxReq], pair[kStripeMaxReq];         // the unit in Fw (a part's pair: the part's first), the pair 0 .. 7 of a part or -1
    int group[kStripeMaxReq];                             // the group that reads the request
    int ng;
    int gci[kStripeMaxGroups], gdiag[kStripeMaxGroups];   // chunk; 1: the diagonal part
    int gbeg[kStripeMaxGroups], gend[kStripeMaxGroups];   // requests [beg, end)
    int gpre[kStripeMaxGroups];                           // requests issued once the group's wait is reached
    int gwait[kStripeMaxGroups];                          // the vmcnt of that wait
    int gpost[kStripeMaxGroups];                          // requests issued behind the wait
};

constexpr int stripe_zero(int R) { return fc_total_units(R) * 1024; }   // the zero unit's byte offset from Fw
constexpr int stripe_pair_off(int R, int lc, int p) { return 16 * (fc_diag_start(R, lc, p) - (2 * (lc * fc_cp(R) + p) + 1)); }
// the vector offset lane l of request u forms: the device's arithmetic (stripe_device.hpp: stripe_issue_plan), in its unsigned 32 bits
constexpr unsigned stripe_lane_voff(const StripePlan& p, int u, int l) { return l > p.thr[u] ? 16u * (unsigned)l : (unsigned)p.zoff[u]; }

// A: the lookahead in requests, both kinds together (at most the ring that bounds it: D, or NS where there is no LDS ring)
constexpr StripePlan stripe_plan(int R, int S, int W, int A, bool diag_by_reg = false)
{
    StripePlan p{};
    const StripeDeal d = stripe_deal(R, S);
    const StripeGroups q = stripe_groups(d, R, W);
    const int CPB = fc_cpb(R), CP = fc_cp(R);
    p.D = diag_by_reg ? 0 : 128 / S;
    p.NS = diag_by_reg ? kStripeRegRing : kStripeRegSlots;
    p.A = stripe_min(A, diag_by_reg ? p.NS : p.D);
    p.lead = W < R ? 4 * ((R - W + S - 1) / S) : 0;
    p.ng = q.n;
    int u = 0, nreg = 0;
    for (int g = 0; g < q.n; ++g) {
        const int lc = q.ci[g] % CPB;
        p.gci[g] = q.ci[g], p.gdiag[g] = q.diag[g], p.gbeg[g] = u;
        if (q.diag[g] && diag_by_reg) {
            const int part = d.unit[W][q.beg[g]] * 1024;
            int lo = stripe_pair_off(R, lc, 0), hi = lo;   // what the part's immediates have to span
            for (int c = 1; c < CP; ++c) {
                lo = stripe_min(lo, stripe_pair_off(R, lc, c));
                hi = stripe_max(hi, stripe_pair_off(R, lc, c));
            }
            const int bias = stripe_max(0, (lo + hi) / 2 / 16 * 16);
            for (int c = 0; c < CP; ++c, ++u) {
                p.kind[u] = 1, p.slot[u] = nreg++ % p.NS, p.unit[u] = part / 1024, p.pair[u] = c;
                p.thr[u] = 2 * (lc * CP + c);
                p.base[u] = part + bias;
                p.imm[u] = stripe_pair_off(R, lc, c) - bias;
                p.zoff[u] = stripe_zero(R) - (p.base[u] + p.imm[u]);
            }
        } else {
            for (int v = q.beg[g]; v < q.end[g]; ++v, ++u) {
                p.unit[u] = d.unit[W][v], p.pair[u] = -1, p.thr[u] = -1;
                if (q.diag[g]) {
                    p.slot[u] = u % p.D;
                } else {
                    p.kind[u] = 1, p.slot[u] = nreg++ % p.NS;
                    p.base[u] = p.unit[u] * 1024 / kStripeBaseSpan * kStripeBaseSpan + kStripeBaseBias;
                    p.imm[u] = p.unit[u] * 1024 - p.base[u];
                }
            }
        }
        p.gend[g] = u;
        for (int v = p.gbeg[g]; v < u; ++v) p.group[v] = g;
    }
    p.n = u;
    p.pro = stripe_min(p.A, p.n);
    int issued = p.pro;
    for (int g = 0; g < p.ng; ++g) {
        p.gpre[g] = stripe_max(issued, p.gend[g]);
        p.gwait[g] = p.gpre[g] - p.gend[g];
        p.gpost[g] = stripe_max(p.gpre[g], stripe_min(p.n, p.gend[g] + p.A));
        issued = p.gpost[g];
    }
    return p;
}

// The replay.  The wave's order of events (stripe_device.hpp: stripe_plan_ahead): the prologue's leading loads, its burst [0, pro),
// vmcnt(pro); then per group g: issue [.., gpre), vmcnt(gwait), issue [gpre, gpost).  The requests in front of g's wait go out before the
// multiply-adds of g - 1 where g is an LDS-DMA group -- whose LDS reads follow its wait, in front of those multiply-adds -- and behind
// them where g is a register group.  For a plan that holds an LDS-DMA request the replay lets every group's requests in front of its wait
// reuse only the register slots of the groups up to g - 2.  0: every claim holds, otherwise the claim that fails:
//   1  the groups are not the deal's, do not tile the requests in order, mix kinds, or a part by register load is not eight requests,
//      pair by pair
//   2  a wait does not leave exactly the requests issued behind the group's last one
//   3  64 or more operations outstanding (the leading loads included)
//   4  a position issued twice, out of order or beyond the list
//   5  an immediate outside -4096 .. 4095, a negative base, or an every-lane request that does not address its unit of the deal
//   6  a register slot requested again before its group was multiplied
//   7  a ring slot requested again before its group was read, or not u mod D
//   8  a request never issued, or a register group exceeds the ring
//   9  a request with a lane threshold: a valid lane (l > 2 pl) does not address the 16 bytes the ring read addresses -- lane
//      fc_diag_start(R, LC, p) + l - (2 pl + 1) of the part --, they leave the part, or a zero lane does not address the zero unit with a
//      non-negative offset
constexpr int stripe_plan_check(const StripePlan& p, int R, int S, int W)
{
    const StripeDeal d = stripe_deal(R, S);
    const StripeGroups q = stripe_groups(d, R, W);
    const int CPB = fc_cpb(R), CP = fc_cp(R), total = fc_total_units(R), zero = total * 1024;
    if (p.n < 1 || p.n > kStripeMaxReq || p.ng < 1 || p.ng != q.n || p.gbeg[0] != 0 || p.gend[p.ng - 1] != p.n) return 1;
    if (p.NS < 1 || p.NS > kStripeRegRing) return 8;
    bool dma = false;                                      // the plan holds an LDS-DMA request
    for (int g = 0; g < p.ng; ++g) {
        if (p.gend[g] <= p.gbeg[g] || (g > 0 && p.gbeg[g] != p.gend[g - 1])) return 1;
        const int kind = p.kind[p.gbeg[g]], size = p.gend[g] - p.gbeg[g];
        const bool part = kind == 1 && p.gdiag[g];         // a part by register load
        if (kind == 1 && size > p.NS) return 8;
        if (p.gci[g] != q.ci[g] || p.gdiag[g] != q.diag[g] || size != (part ? CP : q.end[g] - q.beg[g])) return 1;
        if (kind == 0 && !p.gdiag[g]) return 1;
        dma = dma || kind == 0;
        for (int u = p.gbeg[g]; u < p.gend[g]; ++u) {
            if (p.group[u] != g || p.kind[u] != kind) return 1;
            if (part ? p.pair[u] != u - p.gbeg[g] || p.thr[u] < 0 : p.pair[u] != -1 || p.thr[u] != -1) return 1;
        }
    }
    for (int u = 0; u < p.n; ++u) {
        const int g = p.group[u], ci = p.gci[g], lc = ci % CPB;
        if (p.kind[u] == 0) {
            if (p.D < 1 || p.D > 128 || p.slot[u] != u % p.D) return 7;
            if (p.unit[u] != d.unit[W][q.beg[g] + u - p.gbeg[g]]) return 1;
            continue;
        }
        if (p.imm[u] < -4096 || p.imm[u] > 4095 || p.base[u] < 0) return 5;
        if (p.slot[u] < 0 || p.slot[u] >= p.NS) return 6;
        if (p.unit[u] < 0 || p.unit[u] >= total) return 5;
        if (p.thr[u] < 0) {
            if (p.base[u] + p.imm[u] != p.unit[u] * 1024 || p.unit[u] != d.unit[W][q.beg[g] + u - p.gbeg[g]]) return 5;
            continue;
        }
        const int c = p.pair[u], pl = lc * CP + c;
        if (d.diag_pos[W][ci] < 0 || p.unit[u] != fc_chunk_base(R, ci) || p.thr[u] != 2 * pl) return 9;
        const int part = p.unit[u] * 1024, bytes = fc_diag_units(R, lc) * 1024, first = fc_diag_start(R, lc, c) - (2 * pl + 1);
        if (p.zoff[u] < 0) return 9;
        for (int l = 0; l < 64; ++l) {
            const long long at = (long long)p.base[u] + p.imm[u] + (long long)stripe_lane_voff(p, u, l);
            if (l > p.thr[u]) {
                if (at != part + 16 * (first + l) || at < part || at + 16 > part + bytes) return 9;
            } else if (at != zero) return 9;
        }
    }
    int reg_owner[kStripeRegRing] = {}, ring_owner[128] = {};
    for (int i = 0; i < kStripeRegRing; ++i) reg_owner[i] = -1;
    for (int i = 0; i < 128; ++i) ring_owner[i] = -1;
    int issued = 0, landed = 0, fail = 0;
    // requests [issued, upto) go out; `applied`: the last group multiplied, `read`: the last group read out of the ring
    auto issue = [&](int upto, int applied, int read) {
        if (upto < issued || upto > p.n) fail = fail ? fail : 4;
        for (int u = issued; u < upto && !fail; ++u) {
            int& owner = p.kind[u] == 1 ? reg_owner[p.slot[u]] : ring_owner[p.slot[u]];
            if (owner >= 0 && owner > (p.kind[u] == 1 ? applied : read)) fail = p.kind[u] == 1 ? 6 : 7;
            owner = p.group[u];
        }
        issued = upto;
    };
    issue(p.pro, -1, -1);
    if (p.lead + issued >= 64) return 3;                   // (the leading loads are out until the prologue's vmcnt(pro))
    for (int g = 0; g < p.ng && !fail; ++g) {
        issue(p.gpre[g], dma ? g - 2 : g - 1, g - 1);
        if (issued - landed >= 64) return 3;
        if (issued < p.gend[g] || p.gwait[g] != issued - p.gend[g] || p.gwait[g] > 63) return 2;
        landed = p.gend[g];
        issue(p.gpost[g], g - 1, g);
        if (issued - landed >= 64) return 3;
    }
    if (fail) return fail;
    return issued == p.n ? 0 : 8;
}

// every off-diagonal unit of Fw is requested exactly once by the S waves' plans, and every diagonal part either unit by unit or pair by
// pair, at the addresses the plans state
constexpr bool stripe_plans_cover(int R, int S, int A, bool diag_by_reg = false)
{
    int seen[256] = {}, seen_pair[16][8] = {};
    for (int w = 0; w < S; ++w) {
        const StripePlan p = stripe_plan(R, S, w, A, diag_by_reg);
        if (stripe_plan_check(p, R, S, w) != 0) return false;
        for (int u = 0; u < p.n; ++u) {
            if (p.thr[u] < 0) {
                if (seen[p.unit[u]]++) return false;
            } else if (seen_pair[p.gci[p.group[u]]][p.pair[u]]++) return false;
        }
    }
    for (int ci = 0; ci < fc_nchunk(R); ++ci) {
        const int b = fc_chunk_base(R, ci), du = fc_diag_units(R, ci % fc_cpb(R)), by_pair = seen_pair[ci][0];
        for (int c = 0; c < fc_cp(R); ++c)
            if (seen_pair[ci][c] != by_pair) return false;
        for (int i = 0; i < fc_chunk_units(R, ci); ++i)
            if (seen[b + i] != (i < du ? 1 - by_pair : 1)) return false;
    }
    return true;
}

// The form a launch of the stripe kernel takes (k_logpdf.hip: launch_stripe; the hooks mcd_stripe_schedule_selftest_,
// mcd_stripe_finish_selftest_, mcd_stripe_diag_batch_selftest_) for R row blocks, a sweep over ncols columns and `batch` chains.
// prologue, sched, finish, diag: the values of MCD_STRIPE_PROLOGUE, MCD_STRIPE_SCHED, MCD_STRIPE_FINISH and MCD_STRIPE_DIAG as opt_get
// returns them, kStripeUnset (options.h: MCD_OPT_UNSET) for an option that is not set.
//   * The private prologue has round 14's loop only (schedule 0).
//   * Schedule 2 takes whole sweeps only -- no chunk cut, the last chunk starts in front of ncols --; a sweep that stops early runs
//     schedule 1.
//   * Only schedule 2 has the per-chain finish (each chain of the workgroup finished by a wave of its own, k_logpdf_stripe_fin; 0: wave 0
//     finishes both, k_logpdf_stripe), and only the per-chain finish has the diagonal parts by register load (k_logpdf_stripe_reg; 0:
//     the parts through the LDS ring).  Everywhere else the two options have no effect.
//   * The default of MCD_STRIPE_DIAG depends on the batch (profiles/r20_stripe_regdiag_ab.txt; N = 256, us per launch against the ring's
//     kernel): 512 chains -0.17, 384 chains level, 256 chains +0.06, 129 chains +0.07.  The register loads save instruction issue, which
//     binds where all 256 CUs pull on the L2 together; with half the CUs idle the ring's kernel is the faster one, because a part costs
//     the CU's load path eight 1-KiB requests instead of its 7, 5, 3 or 1 units.  So: register loads from kStripeDiagFrom chains on.
enum StripeForm { kStripePrivate0, kStripeShared0, kStripeShared1, kStripeShared2, kStripeFin, kStripeReg };
constexpr int kStripeUnset = -2147483647 - 1;
constexpr int kStripePrologueDefault = 1;                  // MCD_STRIPE_PROLOGUE unset: the shared prologue
constexpr int kStripeSchedDefault = 2;                     // MCD_STRIPE_SCHED unset: the schedule with register loads
constexpr int kStripeFinishDefault = 1;                    // MCD_STRIPE_FINISH unset: a finishing wave per chain
constexpr int kStripeDiagFrom = 385;                       // MCD_STRIPE_DIAG unset: register loads for a batch of at least this many chains
constexpr bool stripe_sched_whole(int R, int ncols) { return ncols > 16 * (fc_nchunk(R) - 1); }
constexpr StripeForm stripe_form(int prologue, int sched, int finish, int diag, long long batch, int R, int ncols)
{
    if ((prologue == kStripeUnset ? kStripePrologueDefault : prologue) == 0) return kStripePrivate0;
    if (sched == kStripeUnset) sched = kStripeSchedDefault;
    if (sched == 0) return kStripeShared0;
    if (sched != 2 || !stripe_sched_whole(R, ncols)) return kStripeShared1;
    if ((finish == kStripeUnset ? kStripeFinishDefault : finish) == 0) return kStripeShared2;
    return (diag == kStripeUnset ? batch >= kStripeDiagFrom : diag != 0) ? kStripeReg : kStripeFin;
}

}  // namespace mcd
