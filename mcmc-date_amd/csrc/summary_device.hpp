// summary_device.hpp -- posterior summaries and convergence diagnostics of a trace on the device (k_summary.hip, summary_capi.cpp).
// A trace is n samples x B chains x Q quantities, read IN PLACE through one of two front ends:
//   plain   X[n][B][ldq] doubles, quantity q of (sample k, chain b) at X[(k B + b) ldq + q];
//   ring    the waiting samples of the Metropolis-Hastings driver's recorder (MhRec, mvn_kernels.h): sample k of the window is the record
//           of slot (first + k) mod capacity, chain b; Q = 2 n_nodes + 9 quantities in the fixed order ages tH h_v [n_nodes] (one fp64
//           multiply, as monitor.Trace.ages), rates [n_nodes], birth, death, tH, rMu, rVar, ln prior, ln likelihood, ln
//           jacobianRootBranch, ln posterior = (ln prior + ln likelihood) + ln jacobianRootBranch.
// Everywhere lanes = 64 consecutive quantities, so a wave's load of one (sample, chain) is one contiguous row of a record.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mcd {

struct SumSrc {
    const double* base;
    int64_t n, B, Q;
    int64_t ldq;                      // plain: leading dimension of a (sample, chain) row
    int32_t ring;                     // 1: the recorder's ring
    int32_t n_nodes;                  // ring: nodes of the tree
    int64_t first, cap, stride, ld;   // ring: slot of sample 0, slots, doubles per record (mh_rec_stride(ld)), leading dimension of the state
};

constexpr int kSumCols = 9;           // MCD_SUMMARY_COLS
constexpr int kSumMaxLag = 255;       // MCD_SUMMARY_MAX_LAG: four waves of kAcovLags lags each share one window
constexpr int kAcovLags = 64;         // lags per wave of k_sum_acov (its accumulators: 128 registers)
constexpr int kAcovTile = 32;         // samples staged per barrier pair
constexpr int kAcovRows = kSumMaxLag + 1 + kAcovTile;   // rows of the sliding window in LDS: [rows][64 lanes] doubles = 144 KiB
constexpr int kSelWaves = 16;         // waves of k_sum_select's one workgroup per 64 quantities

// Doubles of workspace for a trace of these sizes with n_lags = max_lag + 1 lags (0: no effective sample size), and the number of chunks
// the 2 B split sequences are cut into for the autocovariance sums (a function of the sizes alone: the combination order is fixed).
int64_t summary_chunks(int64_t B, int64_t Q);
size_t summary_workspace_doubles(int64_t B, int64_t Q, int n_lags);
// All launches of one summary on `st`: d_pooled [Q][9], d_per_chain [B][Q][4] or null (device memory).  The caller has checked the
// arguments (n >= 1, B >= 1, Q >= 1, n B in [2, 2^32), max_lag 0 or odd in [1, min(kSumMaxLag, n / 2 - 1)]).
hipError_t launch_summary(const SumSrc& S, int max_lag, double* work, double* d_pooled, double* d_per_chain, hipStream_t st);

}  // namespace mcd
