// Stand-alone host check of csrc/stripe_plan.hpp's plan for k_logpdf_stripe_reg (no GPU, no library): every stripe wave at R = 3, 4,
// S = 4, 8 and the lookaheads that are measured, replayed here a second time with a queue that retires in issue order; every diagonal
// request's 64 lane addresses against the layout (fc_layout.hpp) and the deal; and plans damaged on purpose, which the check must refuse.
// Meant for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/test_stripe_plan_reg.cpp -o test_stripe_plan_reg
#include <cstdio>
#include <deque>
#include <vector>

#include "../../mcmc-date_amd/csrc/stripe_plan.hpp"

static_assert(mcd::stripe_plans_cover(4, 4, mcd::kStripeRegAhead, true) && mcd::stripe_plans_cover(3, 4, mcd::kStripeRegAhead, true), "the shipped plans");

// the queue of one wave: -1 a leading load, otherwise the request; vmcnt(n) retires from the front until n are left
static int replay(const mcd::StripePlan& p)
{
    std::deque<int> q;
    std::vector<char> landed(p.n, 0), applied_g(p.ng, 0);
    std::vector<int> reg(p.NS, -1);
    int issued = 0;
    size_t most = 0;
    auto wait = [&](int n) {
        while ((int)q.size() > n) {
            if (q.front() >= 0) landed[q.front()] = 1;
            q.pop_front();
        }
    };
    auto issue = [&](int upto) -> int {
        for (; issued < upto; ++issued) {
            const int u = issued;
            if (u >= p.n) return 4;
            const int old = reg.at(p.slot[u]);
            if (old >= 0 && !applied_g[p.group[old]]) return 6;
            reg[p.slot[u]] = u;
            if (p.imm[u] < -4096 || p.imm[u] > 4095) return 5;
            q.push_back(u);
            most = q.size() > most ? q.size() : most;
        }
        return 0;
    };
    for (int i = 0; i < p.lead; ++i) q.push_back(-1);
    if (int e = issue(p.pro)) return e;
    wait(p.pro);
    for (int x : q)
        if (x < 0) return 2;                               // the leading loads have returned
    for (int g = 0; g < p.ng; ++g) {
        if (g > 0) applied_g[g - 1] = 1;                   // the multiply-adds of the group before, then the group's missing requests
        if (int e = issue(p.gpre[g])) return e;
        wait(p.gwait[g]);
        for (int u = p.gbeg[g]; u < p.gend[g]; ++u)
            if (!landed[u]) return 2;
        if ((int)q.size() != p.gwait[g] || (!q.empty() && q.front() != p.gend[g])) return 2;
        if (int e = issue(p.gpost[g])) return e;
    }
    if (most >= 64) return 3;
    return issued == p.n ? 0 : 8;
}

// the bytes of Fw every lane of every request reads, against the layout and the deal: 0, or the request that is wrong + 1
static int addresses(const mcd::StripePlan& p, int R, int S, int w, std::vector<int>& units, std::vector<int>& pairs)
{
    const mcd::StripeDeal d = mcd::stripe_deal(R, S);
    const long long zero = 1024LL * mcd::fc_total_units(R);
    for (int u = 0; u < p.n; ++u) {
        const int ci = p.gci[p.group[u]], lc = ci % mcd::fc_cpb(R);
        for (int l = 0; l < 64; ++l) {
            const long long at = (long long)p.base[u] + p.imm[u] + (long long)mcd::stripe_lane_voff(p, u, l);
            if (!p.gdiag[p.group[u]]) {
                if (at != 1024LL * p.unit[u] + 16 * l) return u + 1;
                continue;
            }
            const int pl = lc * mcd::fc_cp(R) + p.pair[u];
            const long long part = 1024LL * mcd::fc_chunk_base(R, ci);
            if (d.diag_owner[ci] != w || p.thr[u] != 2 * pl) return u + 1;
            if (l > 2 * pl) {
                // lane l of the pair's diagonal unit: lane fc_diag_start + l - (2 pl + 1) of the part, where the ring read finds it
                if (at != part + 16LL * (mcd::fc_diag_start(R, lc, p.pair[u]) + l - (2 * pl + 1))) return u + 1;
                if (at < part || at + 16 > part + 1024LL * mcd::fc_diag_units(R, lc)) return u + 1;
            } else if (at != zero) {
                return u + 1;
            }
        }
        if (p.gdiag[p.group[u]]) ++pairs.at(ci * 8 + p.pair[u]);
        else ++units.at(p.unit[u]);
    }
    return 0;
}

int main()
{
    int plans = 0;
    {   // a lookahead the register ring cannot hold: both replays say so
        const mcd::StripePlan p = mcd::stripe_plan(4, 4, 0, 28, true);
        if (mcd::stripe_plan_check(p, 4, 4, 0) != 6 || replay(p) != 6) return std::printf("A = 28 passes\n"), 1;
    }
    for (int R = 3; R <= 4; ++R)
        for (int S = 4; S <= 8; S += 4)
            for (int A : {1, 7, 10, 11, 12, 13, 14, 15, 16}) {
                std::vector<int> units(mcd::fc_total_units(R), 0), pairs(mcd::fc_nchunk(R) * 8, 0);
                for (int w = 0; w < S; ++w, ++plans) {
                    const mcd::StripePlan p = mcd::stripe_plan(R, S, w, A, true);
                    const int c = mcd::stripe_plan_check(p, R, S, w), r = replay(p), a = addresses(p, R, S, w, units, pairs);
                    if (c != 0 || r != 0 || a != 0) return std::printf("R %d S %d A %d wave %d: check %d, replay %d, addresses %d\n", R, S, A, w, c, r, a), 1;
                    // damaged plans: a wait one short, a slot taken a ring too early, a wide immediate, a pair one lane off, a zero
                    // offset that misses the zero unit
                    mcd::StripePlan bad = p;
                    bad.gwait[p.ng / 2] += 1;
                    if (mcd::stripe_plan_check(bad, R, S, w) != 2) return std::printf("R %d S %d A %d wave %d: a short wait passes\n", R, S, A, w), 1;
                    bad = p;
                    if (p.pro < p.n) {
                        bad.slot[p.pro] = p.slot[p.pro - 1];
                        if (mcd::stripe_plan_check(bad, R, S, w) != 6) return std::printf("R %d S %d A %d wave %d: a live slot is reused\n", R, S, A, w), 1;
                    }
                    bad = p;
                    bad.base[0] -= 8192, bad.imm[0] += 8192;
                    if (mcd::stripe_plan_check(bad, R, S, w) != 5) return std::printf("R %d S %d A %d wave %d: a wide immediate passes\n", R, S, A, w), 1;
                    for (int u = 0; u < p.n; ++u)
                        if (p.thr[u] >= 0) {
                            bad = p;
                            bad.imm[u] += 16, bad.zoff[u] -= 16;
                            if (mcd::stripe_plan_check(bad, R, S, w) != 9) return std::printf("R %d S %d A %d wave %d: a shifted pair passes\n", R, S, A, w), 1;
                            bad = p;
                            bad.zoff[u] += 16;
                            if (mcd::stripe_plan_check(bad, R, S, w) != 9) return std::printf("R %d S %d A %d wave %d: a missed zero unit passes\n", R, S, A, w), 1;
                            break;
                        }
                }
                for (int ci = 0; ci < mcd::fc_nchunk(R); ++ci) {
                    const int b = mcd::fc_chunk_base(R, ci), du = mcd::fc_diag_units(R, ci % mcd::fc_cpb(R));
                    for (int i = 0; i < mcd::fc_chunk_units(R, ci); ++i)
                        if (units[b + i] != (i < du ? 0 : 1)) return std::printf("R %d S %d A %d: unit %d requested %d times\n", R, S, A, b + i, units[b + i]), 1;
                    for (int q = 0; q < 8; ++q)
                        if (pairs[ci * 8 + q] != 1) return std::printf("R %d S %d A %d: chunk %d pair %d requested %d times\n", R, S, A, ci, q, pairs[ci * 8 + q]), 1;
                }
                if (!mcd::stripe_plans_cover(R, S, A, true)) return std::printf("R %d S %d A %d: stripe_plans_cover\n", R, S, A), 1;
            }
    std::printf("ok: %d plans\n", plans);
    return 0;
}
