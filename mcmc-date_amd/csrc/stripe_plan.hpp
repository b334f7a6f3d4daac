// stripe_plan.hpp -- the issue plan of one stripe wave under the register-load schedule of the inverse-stream kernel
// (stripe_device.hpp: SC = 2); plain constexpr C++, shared by the host (sweep_launch.cpp: mcd_stripe_plan_selftest_,
// tests/cpp/test_stripe_plan.cpp) and the device.
//
// A wave requests the units of its list (stripe_deal.hpp) in list order, each in one of two ways:
//   * a unit of a chunk's diagonal part by LDS-DMA into slot u mod D of the wave's ring, as under every other schedule: its column
//     pairs straddle units and are read back with a lane shift;
//   * an off-diagonal unit by one global_load_dwordx4 straight into the registers that multiply it: lane l's 16 bytes are the two
//     entries of row l.  The address is a scalar base, the lane's 16 l as the vector offset and a 13-bit immediate: one base (Fw +
//     8192 k + 4096) serves the eight units 8 k .. 8 k + 7.  The destination is slot (number of register loads before it) mod
//     kStripeRegSlots of a register ring.
// Both kinds count on vmcnt in issue order, so a wait is a count over the mixed sequence.  The plan lists every position's kind, slot,
// base and immediate, and for every group (a chunk's diagonal part or the wave's off-diagonal pairs of a chunk, in list order) what is
// issued in front of its wait (pre), the vmcnt of the wait, and what is issued behind it (post: up to A units behind the group).
// stripe_plan_check replays the sequence and proves what the device code relies on; the device static_asserts it.
#pragma once

#include "stripe_deal.hpp"

namespace mcd {

constexpr int kStripeRegSlots = 24;                       // 16-byte-per-lane registers of the ring: the lookahead + the largest group
constexpr int kStripeMaxGroups = 32;
constexpr int kStripeBaseSpan = 8192, kStripeBaseBias = 4096;   // bytes of Fw one scalar base covers; the base sits in their middle

struct StripePlan {
    int n, lead, pro, D, A;                               // units; leading loads of the shared prologue; its burst; ring units; lookahead
    int kind[kStripeMaxUnits];                            // 0: LDS-DMA, 1: register load
    int slot[kStripeMaxUnits];                            // ring slot (u mod D) or register slot
    int base[kStripeMaxUnits];                            // register loads: the scalar base's byte offset from Fw ...
    int imm[kStripeMaxUnits];                             // ... and the immediate: base + imm = 1024 unit
    int group[kStripeMaxUnits];                           // the group that reads the position
    int ng;
    int gci[kStripeMaxGroups], gdiag[kStripeMaxGroups];   // chunk; 1: the diagonal part
    int gbeg[kStripeMaxGroups], gend[kStripeMaxGroups];   // list positions [beg, end)
    int gpre[kStripeMaxGroups];                           // positions issued once the group's wait is reached
    int gwait[kStripeMaxGroups];                          // the vmcnt of that wait
    int gpost[kStripeMaxGroups];                          // positions issued behind the group's reads
};

// Which kernel a launch of the stripe kernel takes (k_logpdf.hip: launch_stripe; mcd_stripe_schedule_selftest_): prologue and sched are
// the values of MCD_STRIPE_PROLOGUE and MCD_STRIPE_SCHED or their defaults.  -1: the private prologue (which has round 14's loop only);
// 0, 1, 2: the shared prologue with that schedule.  Schedule 2 takes whole sweeps only -- no chunk cut, the last chunk starts in
// front of ncols --; a sweep that stops early runs schedule 1.
constexpr int kStripePrologueDefault = 1;                  // MCD_STRIPE_PROLOGUE unset: the shared prologue
constexpr int kStripeSchedDefault = 2;                     // MCD_STRIPE_SCHED unset: the schedule with register loads
constexpr bool stripe_sched_whole(int R, int ncols) { return ncols > 16 * (fc_nchunk(R) - 1); }
constexpr int stripe_schedule(int prologue, int sched, int R, int ncols)
{
    if (prologue == 0) return -1;
    if (sched == 2) return stripe_sched_whole(R, ncols) ? 2 : 1;
    return sched != 0 ? 1 : 0;
}
// Which finish a launch takes (mcd_stripe_finish_selftest_): finish is the value of MCD_STRIPE_FINISH or its default.  1: each chain of
// the workgroup finished by a wave of its own (k_logpdf_stripe_fin); 0: wave 0 finishes both (k_logpdf_stripe).  Only
// schedule 2's kernel has the per-chain finish; everywhere else the option has no effect.
constexpr int kStripeFinishDefault = 1;                    // MCD_STRIPE_FINISH unset: a finishing wave per chain
constexpr int stripe_finish(int prologue, int sched, int finish, int R, int ncols)
{
    return stripe_schedule(prologue, sched, R, ncols) == 2 && finish != 0 ? 1 : 0;
}

constexpr int stripe_plan_min(int a, int b) { return a < b ? a : b; }
constexpr int stripe_plan_max(int a, int b) { return a > b ? a : b; }

// A: the lookahead in units, both kinds together (at most the ring)
constexpr StripePlan stripe_plan(int R, int S, int W, int A)
{
    StripePlan p{};
    const StripeDeal d = stripe_deal(R, S);
    p.D = 128 / S;
    p.A = stripe_plan_min(A, p.D);
    p.n = d.n[W];
    p.lead = W < R ? 4 * ((R - W + S - 1) / S) : 0;
    p.pro = stripe_plan_min(p.A, p.n);
    for (int ci = 0; ci < fc_nchunk(R); ++ci) {
        const int nko = R - 1 - ci / fc_cpb(R);
        if (d.diag_pos[W][ci] >= 0) {
            const int g = p.ng++;
            p.gci[g] = ci, p.gdiag[g] = 1;
            p.gbeg[g] = d.diag_pos[W][ci], p.gend[g] = p.gbeg[g] + fc_diag_units(R, ci % fc_cpb(R));
        }
        int beg = -1, end = -1;
        for (int q = 0; q < fc_cp(R); ++q)
            if (d.pair_pos[W][ci][q] >= 0) {
                if (beg < 0) beg = d.pair_pos[W][ci][q];
                end = d.pair_pos[W][ci][q] + nko;
            }
        if (end >= 0) {
            const int g = p.ng++;
            p.gci[g] = ci, p.gdiag[g] = 0;
            p.gbeg[g] = beg, p.gend[g] = end;
        }
    }
    int nreg = 0, issued = p.pro;
    for (int g = 0; g < p.ng; ++g) {
        for (int u = p.gbeg[g]; u < p.gend[g]; ++u) {
            p.group[u] = g;
            p.kind[u] = p.gdiag[g] ? 0 : 1;
            if (p.gdiag[g]) {
                p.slot[u] = u % p.D;
            } else {
                p.slot[u] = nreg++ % kStripeRegSlots;
                p.base[u] = d.unit[W][u] * 1024 / kStripeBaseSpan * kStripeBaseSpan + kStripeBaseBias;
                p.imm[u] = d.unit[W][u] * 1024 - p.base[u];
            }
        }
        p.gpre[g] = stripe_plan_max(issued, p.gend[g]);
        p.gwait[g] = p.gpre[g] - p.gend[g];
        p.gpost[g] = stripe_plan_max(p.gpre[g], stripe_plan_min(p.n, p.gend[g] + p.A));
        issued = p.gpost[g];
    }
    return p;
}

// The replay.  The wave's order of events (stripe_device.hpp): the prologue's leading loads, its burst [0, pro), vmcnt(pro); then per
// group g: issue [.., gpre) -- groups up to g - 2 have been multiplied and groups up to g - 1 read out of LDS by then --, vmcnt(gwait),
// group g's LDS reads or register pins, the multiply-adds of g - 1, issue [gpre, gpost).  0: every claim holds, otherwise the claim
// that fails:
//   1  the groups do not tile the list in order          5  an immediate outside -4096 .. 4095, or base + imm is not the unit
//   2  a wait does not leave exactly the operations      6  a register slot requested again before its group was multiplied
//      issued behind the group's last unit               7  a ring slot requested again before its group was read, or not u mod D
//   3  64 or more operations outstanding                 8  a unit never requested, or a group's registers exceed the ring
//   4  a position issued twice, out of order or beyond the list
constexpr int stripe_plan_check(const StripePlan& p, int R, int S, int W)
{
    const StripeDeal d = stripe_deal(R, S);
    if (p.n != d.n[W] || p.ng < 1 || p.ng > kStripeMaxGroups || p.gbeg[0] != 0 || p.gend[p.ng - 1] != p.n) return 1;
    for (int g = 0; g < p.ng; ++g) {
        if (p.gend[g] <= p.gbeg[g] || (g > 0 && p.gbeg[g] != p.gend[g - 1])) return 1;
        if (!p.gdiag[g] && p.gend[g] - p.gbeg[g] > kStripeRegSlots) return 8;
        for (int u = p.gbeg[g]; u < p.gend[g]; ++u)
            if (p.group[u] != g || p.kind[u] != (p.gdiag[g] ? 0 : 1)) return 1;
    }
    for (int u = 0; u < p.n; ++u) {
        if (p.kind[u] == 0) continue;
        if (p.imm[u] < -4096 || p.imm[u] > 4095 || p.base[u] < 0 || p.base[u] + p.imm[u] != d.unit[W][u] * 1024) return 5;
        if (p.slot[u] < 0 || p.slot[u] >= kStripeRegSlots) return 6;
    }
    int reg_owner[kStripeRegSlots] = {}, ring_owner[128] = {};
    for (int i = 0; i < kStripeRegSlots; ++i) reg_owner[i] = -1;
    for (int i = 0; i < 128; ++i) ring_owner[i] = -1;
    int issued = 0, landed = 0, fail = 0;
    // positions [issued, upto) go out; `applied`: the last group multiplied, `read`: the last group read out of the ring
    auto issue = [&](int upto, int applied, int read) {
        if (upto < issued || upto > p.n) fail = fail ? fail : 4;
        for (int u = issued; u < upto && !fail; ++u) {
            if (p.kind[u] == 1) {
                if (reg_owner[p.slot[u]] >= 0 && reg_owner[p.slot[u]] > applied) fail = 6;
                reg_owner[p.slot[u]] = p.group[u];
            } else {
                if (p.slot[u] != u % p.D || (ring_owner[p.slot[u]] >= 0 && ring_owner[p.slot[u]] > read)) fail = 7;
                ring_owner[p.slot[u]] = p.group[u];
            }
        }
        issued = upto;
    };
    issue(p.pro, -1, -1);
    if (p.lead + issued >= 64) return 3;                   // (the leading loads are out until the prologue's vmcnt(pro))
    for (int g = 0; g < p.ng && !fail; ++g) {
        issue(p.gpre[g], g - 2, g - 1);
        if (issued - landed >= 64) return 3;
        if (issued < p.gend[g] || p.gwait[g] != issued - p.gend[g] || p.gwait[g] > 63) return 2;
        landed = p.gend[g];
        issue(p.gpost[g], g - 1, g);
        if (issued - landed >= 64) return 3;
    }
    if (fail) return fail;
    return issued == p.n ? 0 : 8;
}

// every unit of Fw is requested exactly once by the S waves' plans, at the address the plan states
constexpr bool stripe_plans_cover(int R, int S, int A)
{
    int seen[256] = {};
    const StripeDeal d = stripe_deal(R, S);
    for (int w = 0; w < S; ++w) {
        const StripePlan p = stripe_plan(R, S, w, A);
        if (stripe_plan_check(p, R, S, w) != 0) return false;
        for (int u = 0; u < p.n; ++u) {
            const int unit = p.kind[u] ? (p.base[u] + p.imm[u]) / 1024 : d.unit[w][u];
            if (unit < 0 || unit >= fc_total_units(R) || seen[unit]++) return false;
        }
    }
    for (int i = 0; i < fc_total_units(R); ++i)
        if (seen[i] != 1) return false;
    return true;
}

// ---- the plan of k_logpdf_stripe_reg: the diagonal parts by register load too (MCD_STRIPE_DIAG = 1) ----
// A list position is a REQUEST, one global_load_dwordx4 into a slot of the register ring.  An off-diagonal unit is one request, as above.
// A chunk's diagonal part is eight, one per column pair: pair pl = 8 LC + p keeps the lanes 2 pl + 1 .. 63 of its diagonal unit, back to
// back from lane fc_diag_start(R, LC, p) of the part on, so lane l > 2 pl finds its 16 bytes at
//     part + 16 (fc_diag_start(R, LC, p) - (2 pl + 1)) + 16 l  =  base + imm + 16 l
// -- the element the lane-shifted ring read picks -- and a lane l <= 2 pl, whose entries are zeros the stream does not store, reads a
// unit of zeros that stands behind the stream on the device (fc_total_units(R) x 1024 bytes from Fw on): its vector offset is
// zoff = (that address) - (base + imm) instead of 16 l: every zero lane reads the unit's first 16 bytes.
// One scalar base per part: the eight offsets span less than the 13 signed bits of the immediate.
// The wave's order of events (stripe_device.hpp: stripe_reg_ahead): the prologue's leading loads, its burst [0, pro), vmcnt(pro); then
// per group g: the multiply-adds of g - 1, issue [.., gpre), vmcnt(gwait), issue [gpre, gpost).
constexpr int kStripeRegRing = 32;                        // register slots of this kernel: the lookahead + the largest group (a part's 8) + a group
constexpr int kStripeRegMaxReq = 96;                      // requests of one wave (R = 4, S = 4: 48 + 4 x 8 = 80)
#ifndef MCD_STRIPE_REG_AHEAD
#define MCD_STRIPE_REG_AHEAD 12
#endif
constexpr int kStripeRegAhead = MCD_STRIPE_REG_AHEAD;     // the lookahead of this kernel, in requests (measured 10 .. 16)
struct StripeRegPlan {
    int n, lead, pro, A, NS;                              // requests; leading loads; the burst; lookahead; register slots
    int slot[kStripeRegMaxReq];
    int base[kStripeRegMaxReq], imm[kStripeRegMaxReq];    // lane l of a request reads Fw + base + imm + 16 l, unless l <= thr
    int thr[kStripeRegMaxReq];                            // -1: every lane (an off-diagonal unit); 2 pl: lanes 0 .. 2 pl read zeros
    int zoff[kStripeRegMaxReq];                           // the vector offset of those lanes: base + imm + zoff = the zero unit
    int unit[kStripeRegMaxReq], pair[kStripeRegMaxReq];   // the unit in Fw (a part: its first), the pair 0 .. 7 of a part or -1
    int group[kStripeRegMaxReq];
    int ng;
    int gci[kStripeMaxGroups], gdiag[kStripeMaxGroups];
    int gbeg[kStripeMaxGroups], gend[kStripeMaxGroups];
    int gpre[kStripeMaxGroups], gwait[kStripeMaxGroups], gpost[kStripeMaxGroups];
};

constexpr int stripe_reg_zero(int R) { return fc_total_units(R) * 1024; }   // the zero unit's byte offset from Fw
constexpr int stripe_reg_pair_off(int R, int lc, int p) { return 16 * (fc_diag_start(R, lc, p) - (2 * (lc * fc_cp(R) + p) + 1)); }

// the vector offset lane l of request u forms: the device's arithmetic (stripe_device.hpp: stripe_reg_issue), in its unsigned 32 bits
constexpr unsigned stripe_reg_lane_voff(const StripeRegPlan& p, int u, int l)
{
    return l > p.thr[u] ? 16u * (unsigned)l : (unsigned)p.zoff[u];
}

constexpr StripeRegPlan stripe_reg_plan(int R, int S, int W, int A)
{
    StripeRegPlan p{};
    const StripeDeal d = stripe_deal(R, S);
    const int CPB = fc_cpb(R), CP = fc_cp(R);
    p.NS = kStripeRegRing;
    p.lead = W < R ? 4 * ((R - W + S - 1) / S) : 0;
    int u = 0;
    for (int ci = 0; ci < fc_nchunk(R); ++ci) {
        const int lc = ci % CPB, nko = R - 1 - ci / CPB;
        if (d.diag_pos[W][ci] >= 0) {
            const int g = p.ng++, part = d.unit[W][d.diag_pos[W][ci]] * 1024;
            int lo = stripe_reg_pair_off(R, lc, 0), hi = lo;   // what the part's immediates have to span
            for (int q = 1; q < CP; ++q) {
                lo = stripe_plan_min(lo, stripe_reg_pair_off(R, lc, q));
                hi = stripe_plan_max(hi, stripe_reg_pair_off(R, lc, q));
            }
            const int bias = stripe_plan_max(0, (lo + hi) / 2 / 16 * 16);
            p.gci[g] = ci, p.gdiag[g] = 1, p.gbeg[g] = u;
            for (int q = 0; q < CP; ++q, ++u) {
                p.group[u] = g, p.unit[u] = part / 1024, p.pair[u] = q;
                p.thr[u] = 2 * (lc * CP + q);
                p.base[u] = part + bias;
                p.imm[u] = stripe_reg_pair_off(R, lc, q) - bias;
                p.zoff[u] = stripe_reg_zero(R) - (p.base[u] + p.imm[u]);
            }
            p.gend[g] = u;
        }
        int g = -1;
        for (int q = 0; q < CP; ++q)
            if (d.pair_pos[W][ci][q] >= 0) {
                if (g < 0) {
                    g = p.ng++;
                    p.gci[g] = ci, p.gdiag[g] = 0, p.gbeg[g] = u;
                }
                for (int k = 0; k < nko; ++k, ++u) {
                    const int unit = d.unit[W][d.pair_pos[W][ci][q] + k];
                    p.group[u] = g, p.unit[u] = unit, p.pair[u] = -1, p.thr[u] = -1, p.zoff[u] = 0;
                    p.base[u] = unit * 1024 / kStripeBaseSpan * kStripeBaseSpan + kStripeBaseBias;
                    p.imm[u] = unit * 1024 - p.base[u];
                }
                p.gend[g] = u;
            }
    }
    p.n = u;
    p.A = stripe_plan_min(A, p.NS);
    p.pro = stripe_plan_min(p.A, p.n);
    for (int i = 0; i < p.n; ++i) p.slot[i] = i % p.NS;
    int issued = p.pro;
    for (int g = 0; g < p.ng; ++g) {
        p.gpre[g] = stripe_plan_max(issued, p.gend[g]);
        p.gwait[g] = p.gpre[g] - p.gend[g];
        p.gpost[g] = stripe_plan_max(p.gpre[g], stripe_plan_min(p.n, p.gend[g] + p.A));
        issued = p.gpost[g];
    }
    return p;
}

// The replay.  0: every claim holds, otherwise the claim that fails (the numbers of stripe_plan_check where they apply):
//   1  the groups do not tile the list in order, or a part is not eight requests, pair by pair
//   2  a wait does not leave exactly the requests issued behind the group's last one
//   3  64 or more operations outstanding (the leading loads included)
//   4  a position issued twice, out of order or beyond the list
//   5  an immediate outside -4096 .. 4095, a negative base, or an off-diagonal request that does not address its unit
//   6  a register slot requested again before its group was multiplied
//   8  a request never issued, or a group's registers exceed the ring
//   9  a diagonal request: a valid lane (l > 2 pl) does not address the 16 bytes the ring read addresses -- lane fc_diag_start(R, LC, p)
//      + l - (2 pl + 1) of the part --, they leave the part, or a zero lane does not address the zero unit with a non-negative offset
constexpr int stripe_reg_plan_check(const StripeRegPlan& p, int R, int S, int W)
{
    const StripeDeal d = stripe_deal(R, S);
    const int CPB = fc_cpb(R), CP = fc_cp(R), total = fc_total_units(R), zero = total * 1024;
    if (p.n < 1 || p.n > kStripeRegMaxReq || p.ng < 1 || p.ng > kStripeMaxGroups || p.gbeg[0] != 0 || p.gend[p.ng - 1] != p.n) return 1;
    if (p.NS < 1 || p.NS > kStripeRegRing) return 8;
    for (int g = 0; g < p.ng; ++g) {
        if (p.gend[g] <= p.gbeg[g] || (g > 0 && p.gbeg[g] != p.gend[g - 1])) return 1;
        if (p.gend[g] - p.gbeg[g] > p.NS) return 8;
        if (p.gdiag[g] && p.gend[g] - p.gbeg[g] != CP) return 1;
        for (int u = p.gbeg[g]; u < p.gend[g]; ++u) {
            if (p.group[u] != g) return 1;
            if (p.gdiag[g] ? p.pair[u] != u - p.gbeg[g] || p.thr[u] < 0 : p.pair[u] != -1 || p.thr[u] != -1) return 1;
        }
    }
    for (int u = 0; u < p.n; ++u) {
        if (p.imm[u] < -4096 || p.imm[u] > 4095 || p.base[u] < 0) return 5;
        if (p.slot[u] < 0 || p.slot[u] >= p.NS) return 6;
        if (p.unit[u] < 0 || p.unit[u] >= total) return 5;
        if (p.thr[u] < 0) {
            if (p.base[u] + p.imm[u] != p.unit[u] * 1024) return 5;
            continue;
        }
        const int ci = p.gci[p.group[u]], lc = ci % CPB, q = p.pair[u], pl = lc * CP + q;
        if (d.diag_pos[W][ci] < 0 || p.unit[u] != fc_chunk_base(R, ci) || p.thr[u] != 2 * pl) return 9;
        const int part = p.unit[u] * 1024, bytes = fc_diag_units(R, lc) * 1024, first = fc_diag_start(R, lc, q) - (2 * pl + 1);
        if (p.zoff[u] < 0) return 9;
        for (int l = 0; l < 64; ++l) {
            const long long at = (long long)p.base[u] + p.imm[u] + (long long)stripe_reg_lane_voff(p, u, l);
            if (l > p.thr[u]) {
                if (at != part + 16 * (first + l) || at < part || at + 16 > part + bytes) return 9;
            } else if (at != zero) return 9;
        }
    }
    int owner[kStripeRegRing] = {};
    for (int i = 0; i < kStripeRegRing; ++i) owner[i] = -1;
    int issued = 0, landed = 0, fail = 0;
    auto issue = [&](int upto, int applied) {              // `applied`: the last group multiplied
        if (upto < issued || upto > p.n) fail = fail ? fail : 4;
        for (int u = issued; u < upto && !fail; ++u) {
            if (owner[p.slot[u]] >= 0 && owner[p.slot[u]] > applied) fail = 6;
            owner[p.slot[u]] = p.group[u];
        }
        issued = upto;
    };
    issue(p.pro, -1);
    if (p.lead + issued >= 64) return 3;
    for (int g = 0; g < p.ng && !fail; ++g) {
        issue(p.gpre[g], g - 1);
        if (issued - landed >= 64) return 3;
        if (issued < p.gend[g] || p.gwait[g] != issued - p.gend[g] || p.gwait[g] > 63) return 2;
        landed = p.gend[g];
        issue(p.gpost[g], g - 1);
        if (issued - landed >= 64) return 3;
    }
    if (fail) return fail;
    return issued == p.n ? 0 : 8;
}

// every off-diagonal unit of Fw, and every (diagonal part, pair), is requested exactly once by the S waves' plans
constexpr bool stripe_reg_plans_cover(int R, int S, int A)
{
    int seen[256] = {}, seen_pair[16][8] = {};
    for (int w = 0; w < S; ++w) {
        const StripeRegPlan p = stripe_reg_plan(R, S, w, A);
        if (stripe_reg_plan_check(p, R, S, w) != 0) return false;
        for (int u = 0; u < p.n; ++u) {
            if (p.thr[u] < 0) {
                if (seen[p.unit[u]]++) return false;
            } else if (seen_pair[p.gci[p.group[u]]][p.pair[u]]++) return false;
        }
    }
    for (int ci = 0; ci < fc_nchunk(R); ++ci) {
        const int b = fc_chunk_base(R, ci), du = fc_diag_units(R, ci % fc_cpb(R));
        for (int q = 0; q < fc_cp(R); ++q)
            if (seen_pair[ci][q] != 1) return false;
        for (int i = 0; i < fc_chunk_units(R, ci); ++i)
            if (seen[b + i] != (i < du ? 0 : 1)) return false;
    }
    return true;
}

// Which kernel takes the diagonal parts (mcd_stripe_diag_selftest_): diag is the value of MCD_STRIPE_DIAG or its default.  1: every unit by
// register load (k_logpdf_stripe_reg); 0: the parts through the LDS ring (k_logpdf_stripe_fin).  Only where the per-chain finish runs;
// everywhere else the option has no effect.
// The default depends on the batch (profiles/r20_stripe_regdiag_ab.txt; N = 256, us per launch against the ring's kernel): 512 chains
// -0.17, 384 chains level, 256 chains +0.06, 129 chains +0.07.  The register loads save instruction issue, which binds where all 256
// CUs pull on the L2 together; with half the CUs idle the ring's kernel is the faster one, because a part costs the CU's load path
// eight 1-KiB requests instead of its 7, 5, 3 or 1 units.  So: register loads from kStripeDiagFrom chains on.
constexpr int kStripeDiagFrom = 385;                       // MCD_STRIPE_DIAG unset: register loads for a batch of at least this many chains
constexpr int stripe_diag_default(long long batch) { return batch >= kStripeDiagFrom ? 1 : 0; }
constexpr int stripe_diag(int prologue, int sched, int finish, int diag, int R, int ncols)
{
    return stripe_finish(prologue, sched, finish, R, ncols) == 1 && diag != 0 ? 1 : 0;
}

}  // namespace mcd
