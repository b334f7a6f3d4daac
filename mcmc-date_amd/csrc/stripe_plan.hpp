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

}  // namespace mcd
