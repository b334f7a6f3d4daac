// k_mc3_summary.hip -- the recorder's ring under Metropolis-coupled MCMC (k_mc3.hip): the temperatures move between the chains of a group
// and the states stay, so the samples of ONE temperature lie in a different chain's record from sample to sample.  Two kernels read the
// reciprocal temperature that every record carries (word 2 ld + 8, mh_rec_tail) and compare it with the ladder BIT FOR BIT: the swap kernel
// stores ladder[rank] itself, so equality is exact.
//   k_mc3_gather   the rung-r sequence of every group as a plain trace [n][G][ldq] in the quantity order of mcd_mh_record_quantities -- what
//                  launch_summary (k_summary.hip) takes as a plain SumSrc -- plus holder [n][G], the local chain that carried the rung
//   k_mc3_flow     per chain the samples spent at every rung and the completed cold -> hottest -> cold passages; integers only
// Both are pure functions of the window: plain vector stores, no atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mvn_kernels.h"

namespace mcd {

namespace {

__device__ __forceinline__ int64_t win_slot(const Mc3Win& W, int64_t k) { return (W.first + k) % W.cap; }
__device__ __forceinline__ const double* win_rec(const Mc3Win& W, int64_t slot, int64_t b) { return W.ring + (slot * W.batch + b) * W.stride; }

// One wave per (sample k, group g), four per workgroup: a row of a 23-node tree is under 1 KB.  Lanes 0 .. C - 1 look at the temperatures
// of the group's chains, a ballot names the holder, and from there on the record's address is wave-uniform (SGPRs); the 64 lanes stride
// over the quantities, each load and store one contiguous run of 512 bytes.  The arithmetic is sum_load's (k_summary.hip): an age is
// rec[2 ld + 2] * h, ln posterior (lp + ll) + lj, and the build contracts no multiply-add.
__global__ __launch_bounds__(256) void k_mc3_gather(Mc3Win W, int rung, int64_t G, int64_t Q, int64_t ldq, double* __restrict__ trace,
                                                     int32_t* __restrict__ holder, unsigned long long* __restrict__ err)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (p >= W.n * G) return;
    const int64_t k = p / G, g = p - k * G;
    const int C = W.n_chains;
    const double* grp = win_rec(W, win_slot(W, k), g * C);
    const double want = W.ladder[rung];
    const bool mine = lane < C && grp[(int64_t)lane * W.stride + 2 * W.ld + 8] == want;
    const unsigned long long who = __ballot(mine);
    const int count = __builtin_amdgcn_readfirstlane(__popcll(who));
    if (count != 1) {
        // a sample from before mcd_mh_mc3_init (every beta is 1) or after a mcd_mh_set_temperatures: nothing of the row is written; one
        // 8-byte store names the offender (any one is enough): bit 63, the pair's number p < 2^32, the count <= 16
        if (lane == 0) *err = 0x8000000000000000ull | (unsigned long long)p << 8 | (unsigned long long)count;
        return;
    }
    const int h = __builtin_amdgcn_readfirstlane(__ffsll(who) - 1);
    const double* rec = grp + (int64_t)h * W.stride;
    const double tH = rec[2 * W.ld + 2];
    const int64_t nn = W.n_nodes;
    double* row = trace + p * ldq;
    for (int64_t q = lane; q < ldq; q += 64) {
        double v = 0.0;                                       // the padding behind Q: defined, never read
        if (q < nn) v = tH * rec[q];
        else if (q < 2 * nn) v = rec[W.ld + (q - nn)];
        else if (q < 2 * nn + 8) v = rec[2 * W.ld + (q - 2 * nn)];
        else if (q < Q) v = (rec[2 * W.ld + 5] + rec[2 * W.ld + 6]) + rec[2 * W.ld + 7];
        row[q] = v;
    }
    if (lane == 0) holder[p] = h;
}

// One lane per local chain walks the window's temperatures.  visits [batch][C] are counted in LDS, a column [C] per lane (lane-contiguous:
// no bank conflict), so that no runtime-indexed array leaves the registers for scratch.  A passage is armed at rung 0, marked at rung
// C - 1 and counted at the next return to rung 0.  A temperature that is not on the ladder counts nowhere and moves nothing.
constexpr int kFlowLanes = 64;
constexpr int kFlowMaxChains = 16;                           // mcd_mh_mc3_init: n_chains <= 16

__global__ __launch_bounds__(kFlowLanes) void k_mc3_flow(Mc3Win W, long long* __restrict__ visits, long long* __restrict__ round_trips)
{
    __shared__ long long cnt[kFlowMaxChains][kFlowLanes];
    __shared__ double lad[kFlowMaxChains];
    const int lane = threadIdx.x, C = W.n_chains;
    if (lane < C) lad[lane] = W.ladder[lane];
    for (int r = 0; r < C; ++r) cnt[r][lane] = 0;
    __syncthreads();
    const int64_t b = (int64_t)blockIdx.x * kFlowLanes + lane;
    if (b >= W.batch) return;
    int64_t slot = win_slot(W, 0);
    int state = 0;                                            // 0: idle, 1: armed at the cold rung, 2: has reached the hottest
    long long trips = 0;
    for (int64_t k = 0; k < W.n; ++k) {
        const double beta = win_rec(W, slot, b)[2 * W.ld + 8];
        slot = slot + 1 == W.cap ? 0 : slot + 1;
        int r = -1;
        for (int i = 0; i < C; ++i) r = lad[i] == beta ? i : r;
        if (r < 0) continue;
        cnt[r][lane] += 1;
        if (r == 0) {
            trips += state == 2;
            state = 1;
        } else if (r == C - 1 && state == 1) state = 2;
    }
    for (int r = 0; r < C; ++r) visits[b * C + r] = cnt[r][lane];
    round_trips[b] = trips;
}

}  // namespace

hipError_t launch_mc3_gather(const Mc3Win& W, int rung, int64_t Q, int64_t ldq, double* trace, int32_t* holder, unsigned long long* err,
                             hipStream_t st)
{
    const int64_t G = W.batch / W.n_chains, pairs = W.n * G;
    if (W.n_chains < 2 || W.n_chains > kFlowMaxChains || W.batch % W.n_chains != 0 || rung < 0 || rung >= W.n_chains || ldq < Q || pairs < 1 ||
        (pairs + 3) / 4 > 0x7fffffffLL)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mc3_gather, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, st, W, rung, G, Q, ldq, trace, holder, err);
    return hipGetLastError();
}

hipError_t launch_mc3_flow(const Mc3Win& W, int64_t* visits, int64_t* round_trips, hipStream_t st)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "");
    if (W.n_chains < 2 || W.n_chains > kFlowMaxChains || W.batch < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mc3_flow, dim3((unsigned)((W.batch + kFlowLanes - 1) / kFlowLanes)), dim3(kFlowLanes), 0, st, W, (long long*)visits,
                       (long long*)round_trips);
    return hipGetLastError();
}

}  // namespace mcd
