// k_metric_gemm.hip -- the dense metric's products for all lock-step chains at once (gfx950): Y = X A on the fp64 matrix cores.
//
//     Y[r][k] = sum_j X[r][j] A[j dim + k],    r < rows, k < dim
//
// X and Y are [rows][dim] row-major (the layout of D.q, D.p, N.* and of the right-hand-side workspace of the across-chains form), A is
// [dim][dim] row-major: the stored inverse mass matrix C (exactly symmetric, so Y's rows are C x) or the stored lower-triangular U^-1
// (Y's rows are U^-T z).  metric_device.hpp computes the same sums for one chain per workgroup; here every chain is a row of one product,
// so A is read once per 64 chains and not once per chain.
//
// Tiling: a workgroup of 256 threads (4 waves) owns 64 rows x 64 columns of Y.  It walks j in chunks of 32: the X tile [64][32] and the
// A tile [32][64] of the chunk go through registers (loaded while the previous chunk is multiplied) into LDS, zero-filled outside
// rows x dim and dim x dim; wave w multiplies rows 16 w .. 16 w + 15 with the four 16-column blocks: 8 k steps x 4 blocks of
// v_mfma_f64_16x16x4_f64 per chunk, four accumulators.  Operand layout (wide_device.hpp, k_split.hip): lane l carries
// X[row l & 15][k l >> 4] and A[k l >> 4][column l & 15]; result register i of lane l is row (l >> 4) + 4 i, column l & 15.
//
// Order of the sum: one accumulator per output, j ascending from 0 (lower: from the first row of A that is not zero in the
// workgroup's columns, 64 (k / 64); the terms skipped are exact zeros added to an accumulator that starts at zero) in steps of four,
// the padding terms j >= dim being 0 x 0.  It is a function of dim (and k) alone: no split of the sum, no atomics, and a row of Y depends
// on the same row of X only -- not on rows, the grid, or what the other rows hold (NaN and Inf included).
//
// Rows through an index list (the chains of a NUTS transition that are still building their trees): with `list`, row r of the product is
// row (r / n_list) stride + list[r % n_list] of X and of Y -- slot r / n_list of chain list[r % n_list] in the workspace's layout -- and the
// rows of the other chains are neither read nor written.  Where a row sits in the launch changes nothing of its sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvn_kernels.h"

namespace mcd {

typedef double mg_d4 __attribute__((ext_vector_type(4)));

constexpr int MG_TM = 64;           // rows of Y per workgroup
constexpr int MG_TN = 64;           // columns of Y per workgroup
constexpr int MG_KC = 32;           // terms of the sum per staged chunk
constexpr int MG_LDX = MG_KC + 4;   // LDS row stride of the X tile in doubles: 72 dwords = 8 (mod 64 banks)
constexpr int MG_LDA = MG_TN + 8;   // LDS row stride of the A tile
constexpr int MG_PER = MG_TM * MG_KC / 256;   // elements of each tile per thread

__global__ __launch_bounds__(256) void k_metric_gemm(const double* __restrict__ X, const double* __restrict__ A, double* __restrict__ Y, int64_t rows,
                                                     int dim, int lower, const int* __restrict__ list, int n_list, int64_t stride)
{
    __shared__ double xs[MG_TM * MG_LDX];
    __shared__ double as[MG_KC * MG_LDA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * MG_TM;
    const int n0 = (int)blockIdx.y * MG_TN;
    // this thread's elements of the two tiles: X (row xr + 8 e, term xk), A (term ak + 4 e, column ac)
    const int xr = tid >> 5, xk = tid & 31;
    const int ak = tid >> 6, ac = tid & 63;
    double xv[MG_PER], av[MG_PER];
    // row r of the product in memory: r itself, or through the list; -1 past the end
    auto mem_row = [&](int64_t r) -> int64_t {
        if (r >= rows) return -1;
        return list ? (r / n_list) * stride + list[r % n_list] : r;
    };
    int64_t xrow[MG_PER];
#pragma unroll
    for (int e = 0; e < MG_PER; ++e) xrow[e] = mem_row(r0 + xr + 8 * e);
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < MG_PER; ++e) {
            const int k = k0 + xk;
            xv[e] = (xrow[e] >= 0 && k < dim) ? X[(size_t)xrow[e] * dim + k] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < MG_PER; ++e) {
            const int k = k0 + ak + 4 * e, c = n0 + ac;
            av[e] = (k < dim && c < dim) ? A[(size_t)k * dim + c] : 0.0;
        }
    };
    mg_d4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = mg_d4{0.0, 0.0, 0.0, 0.0};
    const int k_begin = lower ? n0 : 0;                 // rows of a lower-triangular A above the tile's first column hold zeros in all its columns
    fetch(k_begin);
    const double* xa = xs + (16 * wave + (lane & 15)) * MG_LDX + (lane >> 4);
    const double* ab = as + (lane >> 4) * MG_LDA + (lane & 15);
    for (int k0 = k_begin; k0 < dim; k0 += MG_KC) {
        __syncthreads();                                // the previous chunk's readers are done
#pragma unroll
        for (int e = 0; e < MG_PER; ++e) {
            xs[(xr + 8 * e) * MG_LDX + xk] = xv[e];
            as[(ak + 4 * e) * MG_LDA + ac] = av[e];
        }
        __syncthreads();
        if (k0 + MG_KC < dim) fetch(k0 + MG_KC);        // in flight while this chunk is multiplied
#pragma unroll
        for (int kk = 0; kk < MG_KC / 4; ++kk) {
            const double a = xa[4 * kk];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ab[4 * kk * MG_LDA + 16 * nt], acc[nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t r = mem_row(r0 + 16 * wave + (lane >> 4) + 4 * i);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int c = n0 + 16 * nt + (lane & 15);
            if (r >= 0 && c < dim) Y[(size_t)r * dim + c] = acc[nt][i];
        }
    }
}

hipError_t launch_metric_gemm(const double* X, const double* A, double* Y, int64_t rows, int dim, bool lower, hipStream_t st)
{
    return launch_metric_gemm_rows(X, A, Y, rows, dim, lower, nullptr, 0, 0, st);
}

// `slots` x n_list rows through the list (above); list == nullptr: the rows 0 .. slots n_list - 1 themselves
hipError_t launch_metric_gemm_rows(const double* X, const double* A, double* Y, int64_t rows, int dim, bool lower, const int* list, int n_list,
                                   int64_t stride, hipStream_t st)
{
    if (rows <= 0 || dim <= 0) return hipSuccess;
    const dim3 grid((unsigned)((rows + MG_TM - 1) / MG_TM), (unsigned)((dim + MG_TN - 1) / MG_TN));
    hipLaunchKernelGGL(k_metric_gemm, grid, dim3(256), 0, st, X, A, Y, rows, dim, lower ? 1 : 0, list, n_list, stride);
    return hipGetLastError();
}

}  // namespace mcd
