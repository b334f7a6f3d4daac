// sweep_launch.cpp -- the choice of form (host code): which of the column sweep, the row split (k_split.hip) and the multiply forms
// (k_wide*.hip) serves a likelihood or gradient call, the process-wide form policy, and the public launch_logpdf / launch_grad /
// launch_tree_logpdf / launch_tree_grad / launch_tree_logpdf_with_prior, which hand a sweep to the entry of the handle's R group
// (sweep_groups.hpp).
#include "sweep_groups.hpp"
#include "stripe_deal.hpp"
#include "stripe_plan.hpp"
#include <stdlib.h>
#include <atomic>

namespace mcd {

int sweep_chunk_columns(int R)
{
    // columns per chunk (Cfg<R>::CCOLS): the swept column count is rounded up to it (extra columns
    // are zero padding).
    return 2 * ((R == 1) ? 32 : (R == 2) ? 16 : (R <= 4) ? 8 : 4);
}

int wide_chain_tiles(int64_t batch)
{
    const int force = opt_or(OPT_WIDE_CT, 0);
    if (force == 1 || force == 2 || force == 4) return force;
    // 16 chains per workgroup while that leaves every CU at most one workgroup; 32 above (two workgroups then share a CU:
    // one stages while the other multiplies).  64 (MCD_WIDE_CT=4) measured slower at every size: its LDS chunk fills the CU.
    return batch <= 256 * 16 ? 1 : 2;
}

static std::atomic<int> g_form{getenv("MCD_WIDE") ? (atoi(getenv("MCD_WIDE")) ? 2 : 1) : 0};   // MCD_FORM_*: the process default

int set_logpdf_form(int form) { return g_form.exchange(form); }

// the form in force for a handle: its own choice (mcd_mvn_set_form) or, if it has none, the process default
int effective_form(const MvnDev& M)
{
    const int own = M.form ? __atomic_load_n(M.form, __ATOMIC_RELAXED) : 0;
    return own != 0 ? own : g_form.load(std::memory_order_relaxed);
}

MvnFacts::MvnFacts(const MvnDev& M)
    : n(M.n), R(M.R), form(effective_form(M)), split(M.split != nullptr), wide(M.Wt != nullptr), cols(M.Wc != nullptr),
      wide_bwd(M.Wtb != nullptr) {}

bool use_wide(const MvnFacts& M, int64_t batch)
{
    if (!M.wide || M.form == 1) return false;
    if (M.form == 2) return true;
    // measured crossovers (tools/bench_forms.py, profiles/r01_form_crossover.jsonl): at 1024 chains the sweep still wins
    // or ties for every N, at 2048 the multiply form wins from N = 127 up; small N only pays at 8192 chains
    return (M.n >= 96 && batch >= 2048) || (M.n >= 32 && batch >= 8192);
}

bool use_split(const MvnFacts& M, int64_t batch)
{
    // measured window (tools/gpu/window.sh, window2.sh; profiles/r02_split_window.jsonl, r02_split_window_240.jsonl; raw x and
    // tree states alike): above N = 256 -- five or more 64-row blocks in the sweep's dependent chain -- the row split wins for every
    // batch from 1 to 1024 chains, by 1.6x at N = 384 to 6.5x at N = 1024; at 240 < N <= 256 up to 128 chains (6.95-7.25 against
    // 7.4-7.5 us); from 256 chains the sweep's single launch-to-result path is shorter (7.7 against 7.9 us at 512 chains: the split
    // pays about two memory round trips for handing the partial sums over); at N = 200 and 224 (13 / 14 row blocks over 8 groups:
    // uneven) and below the sweep wins everywhere; from 2048 chains k_wide takes over
    const int force = opt_or(OPT_SPLIT, -1);               // tests and tuning (mcd_set_option "MCD_SPLIT"): 1 = wherever possible, 0 = never
    if (M.form != 0 || !M.split || batch < 1 || batch > kSplitMaxBatch || force == 0) return false;
    if (force == 1) return true;
    if (M.n > 256) return true;
    return M.n > 240 && batch <= 128;
}

bool logpdf_inverse_window(const MvnFacts& M, int64_t batch)
{
    // Where raw-x launch_logpdf, once it is on the column sweep, streams W = L^-1 (k_logpdf_stripe, FS = 3) instead of substituting: form auto
    // only -- form "sweep" stays the substitution sweep, bit for bit -- and the headline sizes only, 240 < N <= 256 at 129 .. 512
    // chains (measured: profiles/r12_inverse_stream_ab.txt).  Elsewhere auto keeps the substitution sweep's bits, which the gradient
    // sweep's ll shares; inside the window the gradient takes the row split anyway.  Tree states, the prior variant and the samplers'
    // kernels keep substitution.
    return M.form == 0 && M.n > 240 && M.n <= 256 && batch > 128 && batch <= 512;
}

bool use_split_grad(const MvnFacts& M, int64_t batch)
{
    // the gradient on the row-split schedule: two (tree states: three) launches over 8 row groups x batch / 16 workgroups, where
    // the sweep walks a chain of N / 64 dependent blocks twice and k_wide_grad_mc fills batch / 16 CUs.  MCD_SPLIT as above.
    const int force = opt_or(OPT_SPLIT, -1);
    if (M.form != 0 || !M.split || batch < 1 || batch > kSplitMaxBatch || force == 0) return false;
    if (force == 1) return true;
    return M.n > 256 || (M.n > 240 && batch <= 512);      // (measured: tools/gpu/grad_prof.sh; at N = 224 the sweeps are level or ahead)
}

bool use_wide_grad(const MvnFacts& M, int64_t batch)
{
    // N <= 256: z and y stay in one LDS chunk (k_wide_grad.hip); above they pass through the output buffer (k_wide_grad_mc.hip)
    return M.wide_bwd && use_wide(M, batch);
}

int padded_blocks(int n)
{
    const int r = (n + 63) / 64;
    const int allowed[] = {1, 2, 3, 4, 6, 8, 12, 16};
    for (int a : allowed)
        if (r <= a) return a;
    return -1;
}

// the sweep serves this launch, and the slices of the ring the prior waves use fit it
bool tree_logpdf_can_carry_prior(const MvnFacts& M, int64_t batch, int n_nodes)
{
    if (batch <= 0 || use_split(M, batch) || use_wide(M, batch)) return false;
    const Geometry g = sweep_geometry(M.R, batch);
    return (size_t)(g.cw + sweep_loader_waves(M.R)) * 2 * (size_t)n_nodes * sizeof(double) <= (size_t)2 * sweep_slot_units(M.R) * 64 * 16;
}

// ---- what an entry does with a call: the sweep of R group 0 .. 3, or one of these ----
enum Take { TAKE_REFUSE = -1, TAKE_SPLIT = 4, TAKE_WIDE = 5, TAKE_WIDE_MC = 6, TAKE_SPLIT_PIECES = 7, TAKE_NOTHING = 8 };

static int logpdf_take(const MvnFacts& M, int64_t batch)   // raw x and tree states alike
{
    if (batch <= 0) return TAKE_NOTHING;
    if (use_split(M, batch)) return TAKE_SPLIT;
    if (use_wide(M, batch)) return TAKE_WIDE;
    return sweep_group(M.R);
}

static int grad_take(const MvnFacts& M, int64_t batch, bool in_place /* G == X */)
{
    if (batch <= 0) return TAKE_NOTHING;
    if (use_split_grad(M, batch)) return TAKE_SPLIT;
    if (use_wide_grad(M, batch)) {
        if (M.n <= 256) return TAKE_WIDE;
        // above 256 the gradient rows double as scratch for z: an in-place call (G == X) keeps the sweep, which reads a chain's
        // x completely before it writes
        if (!in_place) return TAKE_WIDE_MC;
    }
    // N > 768: no sweep form of the gradient (16 row blocks of both sweeps' staging do not fit two waves per SIMD: 260 .. 1 200 spilled
    // registers; it was the fallback only -- 207 us at N = 1024 x 512 chains against the row split's 42): whatever the batch and
    // the form asked for, the row split in pieces of at most 1024 chains (in place is fine: its first pass has read every x)
    if (M.R == 16) return M.split ? TAKE_SPLIT_PIECES : TAKE_REFUSE;
    return sweep_group(M.R);
}

static int tree_grad_take(const MvnFacts& M, int64_t batch, bool gH_is_H, bool gH_is_Rt, bool gR_is_H)
{
    if (batch <= 0) return TAKE_NOTHING;
    const bool crossed = gH_is_Rt || gR_is_H;              // (either output may be its own input, not the other's)
    if (use_split_grad(M, batch) && !crossed) return TAKE_SPLIT;
    if (use_wide_grad(M, batch)) {
        if (M.n <= 256) return TAKE_WIDE;
        if (!gH_is_H && !gH_is_Rt) return TAKE_WIDE_MC;    // (the height-gradient rows double as scratch above 256)
    }
    // N > 768: no sweep form of the tree gradient (grad_take has the reason): the row split in pieces of at most 1024 chains, whatever
    // the batch and the form asked for.  Its one restriction: an output that aliases the OTHER input array (the height gradient over the
    // rates or the reverse) is refused -- include/mcmcdate_mvn.h says so.
    if (M.R == 16) return (M.split && !crossed) ? TAKE_SPLIT_PIECES : TAKE_REFUSE;
    return sweep_group(M.R);
}

static SweepLogpdfFn* const kLogpdfGroup[kSweepGroups] = {launch_logpdf_g0, launch_logpdf_g1, launch_logpdf_g2, launch_logpdf_g3};
static SweepTreeLogpdfFn* const kTreeLogpdfGroup[kSweepGroups] = {launch_tree_logpdf_g0, launch_tree_logpdf_g1, launch_tree_logpdf_g2,
                                                                 launch_tree_logpdf_g3};
static SweepTreeLogpdfPriorFn* const kTreeLogpdfPriorGroup[kSweepGroups] = {launch_tree_logpdf_prior_g0, launch_tree_logpdf_prior_g1,
                                                                          launch_tree_logpdf_prior_g2, launch_tree_logpdf_prior_g3};
static SweepGradFn* const kGradGroup[kSweepGroups] = {launch_grad_g0, launch_grad_g1, launch_grad_g2, nullptr};
static SweepTreeGradFn* const kTreeGradGroup[kSweepGroups] = {launch_tree_grad_g0, launch_tree_grad_g1, launch_tree_grad_g2, nullptr};

hipError_t launch_logpdf(const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, hipStream_t st)
{
    switch (const int take = logpdf_take(M, batch)) {
    case TAKE_NOTHING: return hipSuccess;
    case TAKE_SPLIT: return launch_logpdf_split(M, X, ldx, batch, ll, st);
    case TAKE_WIDE: return launch_logpdf_wide(M, X, ldx, batch, ll, st);
    case TAKE_REFUSE: return hipErrorInvalidValue;
    default: return kLogpdfGroup[take](M, X, ldx, batch, ll, st);
    }
}

hipError_t launch_tree_logpdf(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds,
                              const double* tH, const double* rMu, int64_t batch, double* ll, double* logjac,
                              hipStream_t st)
{
    switch (const int take = logpdf_take(M, batch)) {
    case TAKE_NOTHING: return hipSuccess;
    case TAKE_SPLIT: return launch_tree_logpdf_split(M, T, H, Rt, lds, tH, rMu, batch, ll, logjac, st);
    case TAKE_WIDE: return launch_tree_logpdf_wide(M, T, H, Rt, lds, tH, rMu, batch, ll, logjac, st);
    case TAKE_REFUSE: return hipErrorInvalidValue;
    default: return kTreeLogpdfGroup[take](M, T, H, Rt, lds, tH, rMu, batch, ll, logjac, st);
    }
}

// ---- the same launch with the prior role in front (Metropolis-Hastings, two-launch path) ----
hipError_t launch_tree_logpdf_with_prior(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds, const double* tH,
                                         const double* rMu, int64_t batch, double* ll, double* logjac, const MhDev& J, const PriorDev& JP,
                                         hipStream_t st)
{
    if (!tree_logpdf_can_carry_prior(M, batch, J.n_nodes) || J.batch != batch || sweep_group(M.R) < 0) return hipErrorInvalidValue;
    return kTreeLogpdfPriorGroup[sweep_group(M.R)](M, T, H, Rt, lds, tH, rMu, batch, ll, logjac, J, JP, st);
}

hipError_t launch_grad(const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, double* G, int64_t ldg,
                       hipStream_t st)
{
    switch (const int take = grad_take(M, batch, (const double*)G == X)) {
    case TAKE_NOTHING: return hipSuccess;
    case TAKE_SPLIT: return launch_grad_split(M, X, ldx, batch, ll, G, ldg, st);
    case TAKE_WIDE: return launch_grad_wide(M, X, ldx, batch, ll, G, ldg, st);
    case TAKE_WIDE_MC: return launch_grad_wide_mc(M, X, ldx, batch, ll, G, ldg, st);
    case TAKE_SPLIT_PIECES:
        for (int64_t c0 = 0; c0 < batch; c0 += kSplitMaxBatch) {
            const int64_t cnt = (batch - c0 < kSplitMaxBatch) ? batch - c0 : kSplitMaxBatch;
            if (hipError_t e = launch_grad_split(M, X + c0 * ldx, ldx, cnt, ll + c0, G + c0 * ldg, ldg, st)) return e;
        }
        return hipSuccess;
    case TAKE_REFUSE: return hipErrorInvalidValue;
    default: return kGradGroup[take](M, X, ldx, batch, ll, G, ldg, st);
    }
}

hipError_t launch_tree_grad(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds,
                            const double* tH, const double* rMu, int64_t batch, double* ll, double* gH, double* gR,
                            double* gtH, double* grMu, hipStream_t st)
{
    switch (const int take = tree_grad_take(M, batch, (const double*)gH == H, (const double*)gH == Rt, (const double*)gR == H)) {
    case TAKE_NOTHING: return hipSuccess;
    case TAKE_SPLIT: return launch_tree_grad_split(M, T, H, Rt, lds, tH, rMu, batch, ll, gH, gR, gtH, grMu, st);
    case TAKE_WIDE: return launch_tree_grad_wide(M, T, H, Rt, lds, tH, rMu, batch, ll, gH, gR, gtH, grMu, st);
    case TAKE_WIDE_MC: return launch_tree_grad_wide_mc(M, T, H, Rt, lds, tH, rMu, batch, ll, gH, gR, gtH, grMu, st);
    case TAKE_SPLIT_PIECES:
        for (int64_t c0 = 0; c0 < batch; c0 += kSplitMaxBatch) {
            const int64_t cnt = (batch - c0 < kSplitMaxBatch) ? batch - c0 : kSplitMaxBatch;
            if (hipError_t e = launch_tree_grad_split(M, T, H + c0 * lds, Rt + c0 * lds, lds, tH + c0, rMu + c0, cnt, ll + c0, gH + c0 * lds, gR + c0 * lds,
                                                      gtH + c0, grMu + c0, st))
                return e;
        }
        return hipSuccess;
    case TAKE_REFUSE: return hipErrorInvalidValue;
    default: return kTreeGradGroup[take](M, T, H, Rt, lds, tH, rMu, batch, ll, gH, gR, gtH, grMu, st);
    }
}

}  // namespace mcd

// Test hook (tests/test_host.py; no device, no handle): what an entry would do with a call under the knobs as they stand, for a handle of
// these facts.  entry 0 launch_logpdf, 1 launch_grad, 2 launch_tree_logpdf, 3 launch_tree_grad, 4 launch_tree_logpdf_with_prior on a tree of
// n + 2 nodes; alias: bit 0 the (height) gradient is written over x (the heights), bit 1 the height gradient over the rates, bit 2 the rate
// gradient over the heights.  Returns the R group whose sweep runs (0 .. 3), 4 row split, 5 multiply form, 6 its form above 256 dimensions,
// 7 row split in pieces, 8 nothing to do, -1 refused.
extern "C" int mcd_form_selftest_(int entry, int n, int R, int form, int split, int wide, int wide_bwd, int cols, int64_t batch, int alias)
{
    mcd::MvnFacts M;
    M.n = n;
    M.R = R;
    M.form = form;
    M.split = split != 0;
    M.wide = wide != 0;
    M.wide_bwd = wide_bwd != 0;
    M.cols = cols != 0;
    switch (entry) {
    case 0:
    case 2: return mcd::logpdf_take(M, batch);
    case 1: return mcd::grad_take(M, batch, alias & 1);
    case 3: return mcd::tree_grad_take(M, batch, alias & 1, alias & 2, alias & 4);
    case 4: return mcd::tree_logpdf_can_carry_prior(M, batch, n + 2) ? mcd::sweep_group(R) : -1;
    default: return -2;
    }
}

// Test hook (tests/test_inverse_stream_host.py; no device, no handle): the forward factor stream a raw-x launch_logpdf takes under the
// knobs as they stand for a handle of these facts (0 padded, 1 compact, 2 compact by LDS-DMA, 3 inverse: sweep_groups.hpp
// sweep_fwd_stream), -1 where the column sweep does not serve the call.
extern "C" int mcd_stream_selftest_(int n, int R, int form, int split, int wide, int64_t batch)
{
    mcd::MvnFacts M;
    M.n = n;
    M.R = R;
    M.form = form;
    M.split = split != 0;
    M.wide = wide != 0;
    M.wide_bwd = false;
    M.cols = false;
    const int take = mcd::logpdf_take(M, batch);
    if (take < 0 || take >= mcd::kSweepGroups) return -1;
    const mcd::Geometry g = mcd::sweep_geometry(R, batch);
    const bool inv = g.cw == 2 && g.bt == 1;
    return mcd::sweep_fwd_stream(R, g.cw, inv, inv && mcd::logpdf_inverse_window(M, batch));
}

// Test hook (tests/test_stripe_deal_host.py; no device): the list of stripe wave w of S for R row blocks (stripe_deal.hpp), cut as a
// sweep over ncols columns cuts it (the chunks with 16 CI < ncols stay).  piece[i] = {chunk, pair in the chunk or -1 for the chunk's
// diagonal part, first unit in Fw, units, position in the wave's list}.  Returns the pieces kept, -1 for a deal that does not exist,
// -2 if `cap` pieces are too few.
extern "C" int mcd_stripe_deal_selftest_(int R, int S, int w, int ncols, int* piece, int cap)
{
    if ((R != 3 && R != 4) || (S != 4 && S != 8) || w < 0 || w >= S) return -1;
    const mcd::StripeDeal d = mcd::stripe_deal(R, S);
    int np = 0;
    auto put = [&](int ci, int p, int pos, int units) {
        if (np < cap) {
            int* q = piece + 5 * np;
            q[0] = ci, q[1] = p, q[2] = d.unit[w][pos], q[3] = units, q[4] = pos;
        }
        ++np;
    };
    for (int ci = 0; ci < mcd::fc_nchunk(R) && 16 * ci < ncols; ++ci) {
        if (d.diag_pos[w][ci] >= 0) put(ci, -1, d.diag_pos[w][ci], mcd::fc_diag_units(R, ci % mcd::fc_cpb(R)));
        for (int p = 0; p < mcd::fc_cp(R); ++p)
            if (d.pair_pos[w][ci][p] >= 0) put(ci, p, d.pair_pos[w][ci][p], R - 1 - ci / mcd::fc_cpb(R));
    }
    return np <= cap ? np : -2;
}

// Test hooks (no device): the form a launch of the stripe kernel takes for R row blocks, a sweep over ncols columns and `batch` chains
// under the options as they stand (stripe_plan.hpp: stripe_form, the function launch_stripe calls), seen three ways.
static int stripe_form_now(int R, int ncols, long long batch)
{
    static_assert(mcd::kStripeUnset == mcd::MCD_OPT_UNSET, "stripe_form's unset option");
    if (R != 3 && R != 4) return -2;
    return mcd::stripe_form(mcd::opt_get(mcd::OPT_STRIPE_PROLOGUE), mcd::opt_get(mcd::OPT_STRIPE_SCHED), mcd::opt_get(mcd::OPT_STRIPE_FINISH),
                            mcd::opt_get(mcd::OPT_STRIPE_DIAG), batch, R, ncols);
}
// (tests/test_stripe_plan_host.py) -1: the private prologue; 0, 1, 2: the shared prologue with that schedule
extern "C" int mcd_stripe_schedule_selftest_(int R, int ncols)
{
    const int f = stripe_form_now(R, ncols, 512);
    return f < 0 ? f : f == mcd::kStripePrivate0 ? -1 : f == mcd::kStripeShared0 ? 0 : f == mcd::kStripeShared1 ? 1 : 2;
}
// (tests/test_stripe_finish_codegen_host.py, tests/test_gpu_stripe_finish.py) 1: a finishing wave per chain, 0: wave 0 alone
extern "C" int mcd_stripe_finish_selftest_(int R, int ncols)
{
    const int f = stripe_form_now(R, ncols, 512);
    return f < 0 ? f : f >= mcd::kStripeFin ? 1 : 0;
}
// (tests/test_stripe_regdiag_plan_host.py, tests/test_gpu_stripe_regdiag.py) where the diagonal parts of the stream come from: 1 register
// loads (k_logpdf_stripe_reg), 0 the LDS ring.  With MCD_STRIPE_DIAG unset the batch decides.
extern "C" int mcd_stripe_diag_batch_selftest_(int R, int ncols, long long batch)
{
    const int f = stripe_form_now(R, ncols, batch);
    return f < 0 ? f : f == mcd::kStripeReg ? 1 : 0;
}
// ... and for the headline batch, 512 chains, the largest the stripe kernel takes
extern "C" int mcd_stripe_diag_selftest_(int R, int ncols) { return mcd_stripe_diag_batch_selftest_(R, ncols, 512); }

// Test hooks (tests/test_stripe_regdiag_plan_host.py, tests/test_stripe_plan_host.py; no device): the plan of stripe wave w with lookahead A
// (stripe_plan.hpp: stripe_plan) and stripe_plan_check's verdict on it (0: every claim holds); -1 for a plan that does not exist, -2 if the
// arrays are too small.  grp[g] = {chunk, diagonal, first request, end, issued at the wait, vmcnt of the wait, issued behind the wait}.
static int stripe_plan_out(const mcd::StripePlan& p, int R, int S, int w, int cap_pos, int* grp, int cap_grp)
{
    if (p.n > cap_pos || p.ng > cap_grp) return -2;
    for (int g = 0; g < p.ng; ++g) {
        int* q = grp + 7 * g;
        q[0] = p.gci[g], q[1] = p.gdiag[g], q[2] = p.gbeg[g], q[3] = p.gend[g], q[4] = p.gpre[g], q[5] = p.gwait[g], q[6] = p.gpost[g];
    }
    return mcd::stripe_plan_check(p, R, S, w);
}
// k_logpdf_stripe_reg's plan, the diagonal parts by register load (A = 0: the lookahead the library is built with).  head = {requests,
// groups, leading loads, burst, register slots, lookahead, the zero unit's byte offset}; pos[u] = {slot, base, immediate, lane threshold,
// zero offset, unit in Fw, pair, group}; lanes (NULL or [requests][64]): every lane's vector offset.
extern "C" int mcd_stripe_regplan_selftest_(int R, int S, int w, int A, int* head, int* pos, int cap_pos, int* grp, int cap_grp, unsigned* lanes)
{
    if ((R != 3 && R != 4) || (S != 4 && S != 8) || w < 0 || w >= S || A < 0) return -1;
    const mcd::StripePlan p = mcd::stripe_plan(R, S, w, A ? A : mcd::kStripeRegAhead, true);
    const int verdict = stripe_plan_out(p, R, S, w, cap_pos, grp, cap_grp);
    if (verdict == -2) return -2;
    head[0] = p.n, head[1] = p.ng, head[2] = p.lead, head[3] = p.pro, head[4] = p.NS, head[5] = p.A, head[6] = mcd::stripe_zero(R);
    for (int u = 0; u < p.n; ++u) {
        int* q = pos + 8 * u;
        q[0] = p.slot[u], q[1] = p.base[u], q[2] = p.imm[u], q[3] = p.thr[u], q[4] = p.zoff[u], q[5] = p.unit[u], q[6] = p.pair[u], q[7] = p.group[u];
        for (int l = 0; lanes && l < 64; ++l) lanes[64 * u + l] = mcd::stripe_lane_voff(p, u, l);
    }
    return verdict;
}
// The plan with the diagonal parts through the LDS ring.  head = {units, groups, leading loads, burst, ring units, register slots};
// pos[u] = {kind, slot, base, immediate, unit in Fw, group}.
extern "C" int mcd_stripe_plan_selftest_(int R, int S, int w, int A, int* head, int* pos, int cap_pos, int* grp, int cap_grp)
{
    if ((R != 3 && R != 4) || (S != 4 && S != 8) || w < 0 || w >= S || A < 1) return -1;
    const mcd::StripePlan p = mcd::stripe_plan(R, S, w, A);
    const int verdict = stripe_plan_out(p, R, S, w, cap_pos, grp, cap_grp);
    if (verdict == -2) return -2;
    head[0] = p.n, head[1] = p.ng, head[2] = p.lead, head[3] = p.pro, head[4] = p.D, head[5] = p.NS;
    for (int u = 0; u < p.n; ++u) {
        int* q = pos + 6 * u;
        q[0] = p.kind[u], q[1] = p.slot[u], q[2] = p.base[u], q[3] = p.imm[u], q[4] = p.unit[u], q[5] = p.group[u];
    }
    return verdict;
}
