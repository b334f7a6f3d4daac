// Stand-alone host check of csrc/stripe_plan.hpp (no GPU, no library): the issue plan of every stripe wave at R = 3, 4, S = 4, 8 and the
// lookaheads that are measured, replayed here a second time, operation by operation with a queue that retires in issue order, instead
// of by the counts stripe_plan_check keeps; and plans damaged on purpose, which the check must refuse.
// Meant for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/test_stripe_plan.cpp -o test_stripe_plan
#include <cstdio>
#include <deque>
#include <vector>

#include "../../mcmc-date_amd/csrc/stripe_plan.hpp"

static_assert(mcd::stripe_plans_cover(4, 4, 12) && mcd::stripe_plans_cover(3, 4, 12), "the shipped plans");

// the queue of one wave: -1 a leading load, otherwise the list position; vmcnt(n) retires from the front until n are left
static int replay(const mcd::StripePlan& p, int R, int S, int w, std::vector<int>& requested)
{
    const mcd::StripeDeal d = mcd::stripe_deal(R, S);
    std::deque<int> q;
    std::vector<char> landed(p.n, 0), applied_g(p.ng, 0), read_g(p.ng, 0);
    std::vector<int> reg(mcd::kStripeRegSlots, -1), ring(p.D, -1);
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
            if (p.kind[u] == 1) {
                const int old = reg.at(p.slot[u]);
                if (old >= 0 && !applied_g[p.group[old]]) return 6;
                reg[p.slot[u]] = u;
                if (p.imm[u] < -4096 || p.imm[u] > 4095 || (p.base[u] + p.imm[u]) % 1024 != 0) return 5;
                requested.push_back((p.base[u] + p.imm[u]) / 1024);
            } else {
                const int old = ring.at(p.slot[u]);
                if (p.slot[u] != u % p.D || (old >= 0 && !read_g[p.group[old]])) return 7;
                ring[p.slot[u]] = u;
                requested.push_back(d.unit[w][u]);
            }
            if (requested.back() != d.unit[w][u]) return 5;
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
        if (int e = issue(p.gpre[g])) return e;
        wait(p.gwait[g]);
        for (int u = p.gbeg[g]; u < p.gend[g]; ++u)
            if (!landed[u]) return 2;                      // the group's units are there ...
        if ((int)q.size() != p.gwait[g] || (!q.empty() && q.front() != p.gend[g])) return 2;   // ... and nothing behind them was waited for
        read_g[g] = 1;                                     // its LDS reads (a diagonal part) go out in front of ...
        if (g > 0) applied_g[g - 1] = 1;                   // ... the multiply-adds of the group before
        if (int e = issue(p.gpost[g])) return e;
    }
    if (most >= 64) return 3;
    return issued == p.n ? 0 : 8;
}

int main()
{
    int plans = 0;
    {   // a lookahead the register ring cannot hold: both replays say so
        const mcd::StripePlan p = mcd::stripe_plan(4, 4, 0, 32);
        std::vector<int> requested;
        if (mcd::stripe_plan_check(p, 4, 4, 0) != 6 || replay(p, 4, 4, 0, requested) != 6) return std::printf("A = 32 passes\n"), 1;
    }
    for (int R = 3; R <= 4; ++R)
        for (int S = 4; S <= 8; S += 4)
            for (int A : {1, 7, 10, 12, 14, 16}) {
                std::vector<int> seen(mcd::fc_total_units(R), 0);
                for (int w = 0; w < S; ++w, ++plans) {
                    const mcd::StripePlan p = mcd::stripe_plan(R, S, w, A);
                    std::vector<int> requested;
                    const int c = mcd::stripe_plan_check(p, R, S, w), r = replay(p, R, S, w, requested);
                    if (c != 0 || r != 0) return std::printf("R %d S %d A %d wave %d: check %d, replay %d\n", R, S, A, w, c, r), 1;
                    for (int unit : requested) ++seen.at(unit);
                    // damaged plans: a wait one short, a register slot taken a ring too early, an immediate out of range
                    mcd::StripePlan bad = p;
                    bad.gwait[p.ng / 2] += 1;
                    if (mcd::stripe_plan_check(bad, R, S, w) != 2) return std::printf("R %d S %d A %d wave %d: a short wait passes\n", R, S, A, w), 1;
                    bad = p;
                    int moved = 0;
                    for (int u = 0; u < p.n && !moved; ++u)
                        if (p.kind[u] == 1 && u >= p.pro) {
                            for (int v = u - 1; v >= 0 && !moved; --v)
                                if (p.kind[v] == 1) bad.slot[u] = p.slot[v], moved = 1;   // the slot of the unit requested just before
                        }
                    if (moved && mcd::stripe_plan_check(bad, R, S, w) != 6) return std::printf("R %d S %d A %d wave %d: a live slot is reused\n", R, S, A, w), 1;
                    bad = p;
                    for (int u = 0; u < p.n; ++u)
                        if (p.kind[u] == 1) {
                            bad.base[u] -= 8192, bad.imm[u] += 8192;
                            break;
                        }
                    if (mcd::stripe_plan_check(bad, R, S, w) != 5) return std::printf("R %d S %d A %d wave %d: a wide immediate passes\n", R, S, A, w), 1;
                }
                for (size_t i = 0; i < seen.size(); ++i)
                    if (seen[i] != 1) return std::printf("R %d S %d A %d: unit %zu requested %d times\n", R, S, A, i, seen[i]), 1;
                if (!mcd::stripe_plans_cover(R, S, A)) return std::printf("R %d S %d A %d: stripe_plans_cover\n", R, S, A), 1;
            }
    std::printf("ok: %d plans\n", plans);
    return 0;
}
