// glasso_device.hpp -- what glasso_capi.cpp and k_glasso.hip share: the packed layout of the independent graphical-lasso problems and the
// launches.  One problem = one connected component of the screening graph (glasso_capi.cpp), dimension 2 .. kGlassoMaxDim.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mcd {

constexpr int kGlassoMaxDim = 2048;      // per problem: the sparse sampler's own limit of 2048 nodes
constexpr int kGlassoThreads = 256;      // one workgroup per problem; thread t owns the coordinates t, t + 256, ... (the lane stride)
constexpr int kGlassoMaxStrides = kGlassoMaxDim / kGlassoThreads;

struct GlassoDev {
    int n_problems = 0;
    const int32_t* dim = nullptr;        // [n_problems] p
    const int64_t* off = nullptr;        // [n_problems] first element of the problem's p x p blocks in S, W, W_old, B, Theta
    const double* S = nullptr;           // packed, every block row-major and symmetric
    double* W = nullptr;                 // W = Theta^-1, kept symmetric
    const double* W_old = nullptr;       // W as it was when the pass began (the stopping rule compares against it)
    double* B = nullptr;                 // row j: the lasso coefficients of column j (entry j is 0)
    double* Theta = nullptr;
    double* theta_diag = nullptr;        // [sum of p]; problem q's part begins at doff[q]
    const int64_t* doff = nullptr;
    double* change = nullptr;            // [n_problems] largest |W - W_old| of the pass
    unsigned long long* updates = nullptr;   // [n_problems] coordinate updates of the pass
    int32_t* capped = nullptr;           // [n_problems] 1: some column's descent stopped at max_iter sweeps
};

// One outer pass over the columns of every problem (grid = n_problems, no communication between workgroups).
hipError_t launch_glasso_pass(const GlassoDev& G, double rho, double tol, int max_iter, hipStream_t st);
// Theta from W and the coefficient rows: the diagonal first, then the symmetrised columns.
hipError_t launch_glasso_theta(const GlassoDev& G, int max_dim, hipStream_t st);

}  // namespace mcd
