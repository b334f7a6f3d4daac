// k_glasso.hip -- the graphical lasso of `prepare` (app/Main.hs:257-276; Friedman, Hastie, Tibshirani 2008) on the device.
//
// The algorithm is prepare.graphical_lasso's: block coordinate descent over the columns of W = Theta^-1, the lasso sub-problem of a column
// by cyclic coordinate descent, warm starts from the previous pass.  It is restated so that a column step costs what it changes:
//   * v = W11 beta is kept as a vector (thread t holds the coordinates t, t + 256, ... in registers, with beta, the column of S and the
//     diagonal of W), so a coordinate's residual is r_k = S_kj - v_k + W_kk beta_k, evaluated for all coordinates at once;
//   * only a coordinate whose new beta_k differs from the old one does work: v += d W[k][.] (W is symmetric: the row is the column and the
//     load is contiguous);
//   * the cyclic order is kept exactly: every lane tests its coordinates against the current v, the workgroup takes the smallest index
//     after the current one that would change, updates it and repeats.  The skipped coordinates were tested against the v they would have
//     seen at their turn, because v only changes at an update;
//   * v is recomputed from the non-zero beta, in index order, at the start of every sweep (nothing drifts from sweep to sweep).
// One workgroup owns one problem (a connected component of the screening graph, glasso_capi.cpp).  Workgroups never communicate, nothing
// waits on memory; the only barriers are __syncthreads().  Every loop is bounded: a sweep makes at most p updates, a column at most max_iter
// sweeps, a launch is one pass over the columns, and the host decides between launches whether another pass follows.  Every sum is in index
// order and there are no atomics: the same input gives the same bits.
#include <hip/hip_runtime.h>

#include <climits>

#include "glasso_device.hpp"

namespace mcd {
namespace {

constexpr int T = kGlassoThreads;
constexpr int MAXS = kGlassoMaxStrides;
constexpr int WAVES = T / 64;

__global__ __launch_bounds__(T) void k_glasso_pass(GlassoDev G, double rho, double tol, int max_iter)
{
    const int q = blockIdx.x;
    const int p = G.dim[q];
    const int64_t off = G.off[q];
    const double* __restrict__ S = G.S + off;
    double* W = G.W + off;
    const double* __restrict__ Wo = G.W_old + off;
    double* B = G.B + off;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ns = (p + T - 1) / T;                      // strides in use, <= MAXS (the host refuses p > kGlassoMaxDim)

    __shared__ int s_cnt[MAXS * WAVES];
    __shared__ int s_nzk[kGlassoMaxDim];                 // the non-zero coefficients of the column at the start of a sweep, in index order
    __shared__ double s_nzb[kGlassoMaxDim];
    __shared__ int s_key[2][WAVES];                      // per wave: its first coordinate that would change, and by how much
    __shared__ double s_d[2][WAVES];
    __shared__ double s_red[WAVES];

    double wkk[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        const int k = t + s * T;
        wkk[s] = (s < ns && k < p) ? W[(int64_t)k * p + k] : 1.0;
    }
    double chg = 0.0;
    unsigned long long n_upd = 0;
    int capped = 0, par = 0;

    for (int j = 0; j < p; ++j) {
        double s12[MAXS], beta[MAXS], v[MAXS], nb[MAXS];
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
            const int k = t + s * T;
            const bool in = s < ns && k < p;
            s12[s] = in ? S[(int64_t)j * p + k] : 0.0;
            beta[s] = in ? B[(int64_t)j * p + k] : 0.0;   // B[j][j] is never written: 0
            v[s] = 0.0;
            nb[s] = 0.0;
        }
        bool done = false;
        for (int sweep = 0; sweep < max_iter && !done; ++sweep) {
            // --- the non-zero coefficients in index order: coordinate t + 256 s = lane + 64 wave + 256 s is ordered by (s, wave, lane)
            unsigned long long nzm[MAXS];
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {
                nzm[s] = 0;
                if (s < ns) {
                    nzm[s] = __ballot(beta[s] != 0.0);
                    if (lane == 0) s_cnt[s * WAVES + wave] = __popcll(nzm[s]);
                }
            }
            __syncthreads();
            int nnz = 0;
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {
                if (s < ns) {
                    int mine = 0;
#pragma unroll
                    for (int w = 0; w < WAVES; ++w) {
                        if (w == wave) mine = nnz;
                        nnz += s_cnt[s * WAVES + w];
                    }
                    if (beta[s] != 0.0) {
                        const int e = mine + __popcll(nzm[s] & ((1ull << lane) - 1ull));
                        s_nzk[e] = t + s * T;             // e < p <= kGlassoMaxDim: one entry per non-zero coordinate
                        s_nzb[e] = beta[s];
                    }
                }
            }
            __syncthreads();
            // --- v = W11 beta from those rows, in index order
#pragma unroll
            for (int s = 0; s < MAXS; ++s) v[s] = 0.0;
            for (int e = 0; e < nnz; ++e) {
                const int k = s_nzk[e];
                const double b = s_nzb[e];
                const double* row = W + (int64_t)k * p;
#pragma unroll
                for (int s = 0; s < MAXS; ++s) {
                    const int i = t + s * T;
                    if (s < ns && i < p) v[s] += b * row[i];
                }
            }
            // --- one sweep: the coordinates that change, in cyclic order (each update moves `cur` up: at most p - 1 of them)
            int cur = -1;
            double delta = 0.0;
            for (int it = 0; it < p; ++it) {
                int sfound = -1;
                unsigned long long m = 0;
                double dsel = 0.0;
#pragma unroll
                for (int s = 0; s < MAXS; ++s) {
                    if (s < ns) {
                        const int k = t + s * T;
                        const double r = s12[s] - v[s] + wkk[s] * beta[s];
                        const double a = fabs(r) - rho;
                        nb[s] = a > 0.0 ? copysign(a, r) / wkk[s] : 0.0;
                        const bool c = k < p && k != j && k > cur && nb[s] != beta[s];
                        const unsigned long long mm = __ballot(c);
                        if (sfound < 0 && mm != 0) {
                            sfound = s;
                            m = mm;
                            dsel = nb[s] - beta[s];
                        }
                    }
                }
                if (sfound >= 0) {
                    if (lane == __ffsll((long long)m) - 1) {
                        s_key[par][wave] = sfound * T + t;
                        s_d[par][wave] = dsel;
                    }
                } else if (lane == 0) {
                    s_key[par][wave] = INT_MAX;
                }
                __syncthreads();                          // (the two parities: a wave may write the next round's slot while another still reads)
                int kmin = INT_MAX;
                double d = 0.0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) {
                    const int kw = s_key[par][w];
                    if (kw < kmin) {
                        kmin = kw;
                        d = s_d[par][w];
                    }
                }
                par ^= 1;
                kmin = __builtin_amdgcn_readfirstlane(kmin);
                if (kmin == INT_MAX) break;
                const double* row = W + (int64_t)kmin * p;
#pragma unroll
                for (int s = 0; s < MAXS; ++s) {
                    const int i = t + s * T;
                    if (s < ns && i < p) {
                        if (i == kmin) beta[s] = nb[s];
                        v[s] += d * row[i];
                    }
                }
                delta = fmax(delta, fabs(d));
                cur = kmin;
                ++n_upd;
            }
            done = delta <= tol;
        }
        if (!done) capped = 1;
        // --- w12 = v into row j and column j of W; the largest change against the pass's start counts where this is the element's last
        // write of the pass (k < j: the element (j, k) was written at step k before and is not written again)
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
            const int k = t + s * T;
            if (s < ns && k < p && k != j) {
                W[(int64_t)j * p + k] = v[s];
                W[(int64_t)k * p + j] = v[s];
                B[(int64_t)j * p + k] = beta[s];
                if (k < j) chg = fmax(chg, fabs(v[s] - Wo[(int64_t)j * p + k]));
            }
        }
        __syncthreads();                                  // the next column reads these rows
    }
    // the pass's largest change: a maximum, so any order gives the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) chg = fmax(chg, __shfl_xor(chg, o));
    if (lane == 0) s_red[wave] = chg;
    __syncthreads();
    if (t == 0) {
        double c = s_red[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) c = fmax(c, s_red[w]);
        G.change[q] = c;
        G.updates[q] = n_upd;
        G.capped[q] = capped;
    }
}

// theta_jj = 1 / (W_jj - w12 . beta), one thread per column, the sum in index order (B[j][j] = 0: the term of k = j is an exact zero)
__global__ __launch_bounds__(64) void k_glasso_theta_diag(GlassoDev G)
{
    const int q = blockIdx.x;
    const int p = G.dim[q];
    const int j = blockIdx.y * 64 + threadIdx.x;
    if (j >= p) return;
    const double* __restrict__ w = G.W + G.off[q] + (int64_t)j * p;
    const double* __restrict__ b = G.B + G.off[q] + (int64_t)j * p;
    double acc = 0.0;
    for (int k = 0; k < p; ++k)
        if (k != j) acc += w[k] * b[k];
    G.theta_diag[G.doff[q] + j] = 1.0 / (w[j] - acc);
}

// column j of Theta is -beta_j theta_jj; symmetrised, entries below 1e-14 set to 0 (as prepare.graphical_lasso does)
__global__ __launch_bounds__(T) void k_glasso_theta(GlassoDev G)
{
    const int q = blockIdx.x;
    const int p = G.dim[q];
    const int i = blockIdx.y;
    const int j = blockIdx.z * T + threadIdx.x;
    if (i >= p || j >= p) return;
    const double* __restrict__ B = G.B + G.off[q];
    const double* __restrict__ td = G.theta_diag + G.doff[q];
    double x;
    if (i == j) {
        x = td[i];
    } else {
        const double a = -B[(int64_t)j * p + i] * td[j];      // Theta[i][j] of column j
        const double b = -B[(int64_t)i * p + j] * td[i];      // Theta[j][i] of column i
        x = 0.5 * (a + b);
    }
    if (fabs(x) < 1e-14) x = 0.0;
    G.Theta[G.off[q] + (int64_t)i * p + j] = x;
}

}  // namespace

hipError_t launch_glasso_pass(const GlassoDev& G, double rho, double tol, int max_iter, hipStream_t st)
{
    if (G.n_problems <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_glasso_pass, dim3((unsigned)G.n_problems), dim3(T), 0, st, G, rho, tol, max_iter);
    return hipGetLastError();
}

hipError_t launch_glasso_theta(const GlassoDev& G, int max_dim, hipStream_t st)
{
    if (G.n_problems <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_glasso_theta_diag, dim3((unsigned)G.n_problems, (unsigned)((max_dim + 63) / 64)), dim3(64), 0, st, G);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_glasso_theta, dim3((unsigned)G.n_problems, (unsigned)max_dim, (unsigned)((max_dim + T - 1) / T)), dim3(T), 0, st, G);
    return hipGetLastError();
}

}  // namespace mcd
