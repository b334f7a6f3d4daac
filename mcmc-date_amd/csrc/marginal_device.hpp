// marginal_device.hpp -- the marginal likelihood from the ln likelihoods of power-posterior chains (k_marginal.hip, marginal_capi.cpp).
// K path points with the exponents betas[K] (0 = betas[0] < ... < betas[K - 1] = 1); the chain with the global number g runs at point g mod K
// and is replicate g / K, so B = K C chains hold C replicates of the whole path.  The n ln likelihoods of a chain are read IN PLACE
// through one of two front ends (as SumSrc, summary_device.hpp):
//   plain   ll[n][B] doubles;
//   ring    a window of the Metropolis-Hastings driver's recorder (MhRec, mvn_kernels.h): sample k is the record of slot (first + k) mod
//           cap, ln likelihood its word 2 ld + 6, and the exponent the chain ran at its word 2 ld + 8 -- which must equal betas[g mod K]
//           bit for bit in every record of the window.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mcd {

struct MlSrc {
    const double* base;
    int64_t n, B;
    int32_t ring;                     // 1: the recorder's ring
    int32_t K;                        // path points
    int64_t first, cap, stride, ld;   // ring: slot of sample 0, slots, doubles per record (mh_rec_stride(ld)), leading dimension of the state
};

constexpr int kMlCols = 5;            // MCD_ML_COLS
constexpr int kMlMaxPoints = 4096;
constexpr int kMlPart = 5;            // per chain: mean, M2, maximum, minimum, S

// doubles of workspace: the chains' partials [B][kMlPart]
inline size_t marginal_workspace_doubles(int64_t B) { return (size_t)B * kMlPart; }
// All launches of one estimate on `st`.  d_betas [K]; d_point [K][kMlCols], d_replicate [B / K][2], d_out [4] (device memory, all written);
// *d_err (zeroed by the caller): a record of the ring whose exponent is not its point's sets it to 1 << 63 | (k B + b).  The caller has
// checked the arguments (2 <= K <= kMlMaxPoints, B a multiple of K, n >= 1, n B / K in [2, 2^32)).
hipError_t launch_marginal(const MlSrc& S, const double* d_betas, double* work, double* d_point, double* d_replicate, double* d_out,
                           unsigned long long* d_err, hipStream_t st);

}  // namespace mcd
