// k_metric_factor.hip -- the dense metric's factors on the device (gfx950): from C [dim][dim] (row-major, on the device) the stored
// symmetric matrix S, its lower Cholesky factor U (U U^T = S) and W = U^-1 in the layout metric_device.hpp, k_metric_gemm.hip and
// k_nuts_across.hip read (full [dim][dim], +0.0 above the diagonal).  What mcd::cholesky_lower / mcd::invert_factor (host_factor.cpp)
// compute on the host, entry by entry the same definitions -- only the order of the sums differs:
//
//     U_ij = (S_ij - sum_{k<j} U_ik U_jk) / U_jj      U_jj = sqrt(S_jj - sum_{k<j} U_jk^2)
//     W_ij = (    - sum_{k=j}^{i-1} U_ik W_kj) / U_ii  W_ii = 1 / U_ii
//
// Every entry is one sum, then one IEEE division or square root: no inverse of a diagonal block is multiplied into anything and no
// entry is multiplied by a reciprocal, so the textbook componentwise backward-error bounds of Cholesky and of forward substitution hold.
//
// Blocked, left-looking, 64 x 64 tiles (a tile is one workgroup's four 16-row bands of v_mfma_f64_16x16x4_f64 accumulators, and a diagonal
// tile fits LDS beside a panel tile).  Block column J takes two launches on one stream:
//
//   k_mf_diag (one workgroup)   T = S_JJ - sum_{K<J} U_JK U_JK^T on the matrix cores, then the tile's own Cholesky factor in LDS.
//   k_mf_rest (NB - 1 - J + J + 1 workgroups)
//       panel tile I > J:       T = S_IJ - sum_{K<J} U_IK U_JK^T, then row i of T substituted against U_JJ in LDS (one lane per row);
//       row J of the inverse:   tile (J, Jc), Jc <= J: T = [J == Jc] I - sum_{K=Jc}^{J-1} U_JK W_K,Jc, then column j of T substituted
//                               against U_JJ (one lane per column).  It needs rows < J of W (earlier launches) and row J of U, which
//                               k_mf_diag(J) completed: the inverse costs no launch of its own.
//
// Order of every sum: one accumulator per entry that starts at the S (or identity) entry; the terms of the earlier block columns in
// ascending k, four at a time, through the matrix cores (operand layout of k_metric_gemm.hip; the products are fused there); then the
// tile's own terms in ascending k, each a rounded product and a rounded subtraction.  A function of dim and the entry's indices alone:
// the same bits on every call.  The steps are ordered by the launches; a workgroup reads what earlier launches or itself wrote; no spin
// barrier, no flag, no floating-point atomic.
//
// Status: one 64-bit word.  The pre-pass takes an atomic minimum of the row-major index of every non-finite entry; k_mf_diag of
// kMfPivot + the global index of every pivot whose sum is not > 0 or not finite (host_factor.cpp's rule).  kMfOk = ~0 is neither.  Every
// kernel after the pre-pass returns at once when the word is not kMfOk: a failed factorisation leaves U and W unfinished, and the caller
// must not use them.  No loop depends on the data: nothing can hang, whatever C holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lds_optin.hpp"
#include "mvn_kernels.h"

namespace mcd {

typedef double mf_d4 __attribute__((ext_vector_type(4)));

constexpr int MF_B = 64;            // tile
constexpr int MF_KC = 32;           // terms per staged chunk
constexpr int MF_LDX = MF_KC + 4;   // row stride of a [64 rows][32 terms] operand tile in LDS (k_metric_gemm.hip's X tile)
constexpr int MF_LDA = MF_B + 8;    // row stride of a [32 terms][64 columns] operand tile (k_metric_gemm.hip's A tile)
constexpr int MF_LDT = MF_B + 1;    // row stride of the accumulated tile: rows and columns both conflict-free
constexpr int MF_STAGE = 2 * MF_B * MF_LDX;                          // doubles of the two staged operands (>= MF_KC * MF_LDA + MF_B * MF_LDX)
constexpr int MF_TILE = MF_B * MF_LDT;
constexpr int MF_UNION = MF_STAGE > MF_TILE ? MF_STAGE : MF_TILE;    // the accumulated tile takes the staging area's place
constexpr int MF_REST_LDS = (MF_UNION + MF_B * MF_B) * (int)sizeof(double);

// acc (wave w: rows 16 w .. 16 w + 15 of the tile, four 16-column blocks) -= sum_{k = k_begin}^{k_end - 1} A[a0 + row][k] B(k, col).
//   BT:  B(k, col) = Bm[(b0 + col) dim + k]   (rows of U: the product U U^T)
//   !BT: B(k, col) = Bm[k dim + b0 + col]     (rows of W)
// k_begin and k_end are multiples of 64 and k_end <= dim; rows and columns past dim are staged as zeros.  All 256 threads.
template <bool BT>
__device__ __forceinline__ void mf_accumulate(const double* A, int a0, const double* Bm, int b0, int dim, int k_begin, int k_end, double* stage,
                                              mf_d4 (&acc)[4])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* xs = stage;
    double* bs = stage + MF_B * MF_LDX;
    const int xr = tid >> 5, xk = tid & 31;
    const int ak = tid >> 6, ac = tid & 63;
    constexpr int PER = MF_B * MF_KC / 256;
    double xv[PER], bv[PER];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int r = a0 + xr + 8 * e, k = k0 + xk;
            xv[e] = (r < dim && k < k_end) ? A[(size_t)r * dim + k] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            if (BT) {
                const int r = b0 + xr + 8 * e, k = k0 + xk;
                bv[e] = (r < dim && k < k_end) ? Bm[(size_t)r * dim + k] : 0.0;
            } else {
                const int k = k0 + ak + 4 * e, c = b0 + ac;
                bv[e] = (k < k_end && c < dim) ? Bm[(size_t)k * dim + c] : 0.0;
            }
        }
    };
    if (k_begin >= k_end) return;
    fetch(k_begin);
    const double* xa = xs + (16 * wave + (lane & 15)) * MF_LDX + (lane >> 4);
    const double* bb = BT ? bs + (lane & 15) * MF_LDX + (lane >> 4) : bs + (lane >> 4) * MF_LDA + (lane & 15);
    for (int k0 = k_begin; k0 < k_end; k0 += MF_KC) {
        __syncthreads();                                // the previous chunk's readers are done
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            xs[(xr + 8 * e) * MF_LDX + xk] = xv[e];
            if (BT)
                bs[(xr + 8 * e) * MF_LDX + xk] = bv[e];
            else
                bs[(ak + 4 * e) * MF_LDA + ac] = bv[e];
        }
        __syncthreads();
        if (k0 + MF_KC < k_end) fetch(k0 + MF_KC);      // in flight while this chunk is multiplied
#pragma unroll
        for (int kk = 0; kk < MF_KC / 4; ++kk) {
            const double a = -xa[4 * kk];               // exact: the accumulator takes S - sum
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const double b = BT ? bb[16 * nt * MF_LDX + 4 * kk] : bb[4 * kk * MF_LDA + 16 * nt];
                acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[nt], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                    // the staging area may be overwritten
}

// the accumulators into T [64][MF_LDT] (transposed: T[col][row]); result register i of lane l is row (l >> 4) + 4 i, column l & 15 of a block
template <bool TRANSPOSED>
__device__ __forceinline__ void mf_store_tile(const mf_d4 (&acc)[4], double* T)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 16 * wave + (lane >> 4) + 4 * i, c = 16 * nt + (lane & 15);
            T[TRANSPOSED ? c * MF_LDT + r : r * MF_LDT + c] = acc[nt][i];
        }
}

// The pre-pass: S = the symmetric part of C (of keep C + floor I with `shrink`, the warm-up's window covariance: one multiplication and
// one addition per entry, as the host writes it), S_ii = C_ii, S_ij = S_ji = 0.5 (C_ij + C_ji); the finite scan of what is symmetrised.
// One workgroup per 32 x 32 tile on or above the diagonal and its mirror image, both read and written along rows.
__global__ __launch_bounds__(256) void k_mf_prepass(const double* __restrict__ C, double* __restrict__ S, int dim, int shrink, double keep, double floor_,
                                                    unsigned long long* status)
{
    __shared__ double t[32][33];
    const int bx = blockIdx.x, by = blockIdx.y;         // tile rows 32 by, columns 32 bx
    if (bx < by) return;
    const int ty = threadIdx.x >> 5, tx = threadIdx.x & 31;
    auto value = [&](int i, int j) {
        const double c = C[(size_t)i * dim + j];
        return shrink ? keep * c + (i == j ? floor_ : 0.0) : c;
    };
#pragma unroll
    for (int e = 0; e < 4; ++e) {                       // the mirror tile: rows 32 bx, columns 32 by
        const int r = ty + 8 * e, gi = 32 * bx + r, gj = 32 * by + tx;
        t[r][tx] = (gi < dim && gj < dim) ? value(gi, gj) : 0.0;
    }
    __syncthreads();
    double s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = ty + 8 * e, gi = 32 * by + r, gj = 32 * bx + tx;
        s[e] = 0.0;
        if (gi < dim && gj < dim) {
            const double a = value(gi, gj), b = t[tx][r];
            if (!isfinite(a)) atomicMin(status, (unsigned long long)gi * (unsigned long long)dim + (unsigned long long)gj);
            if (!isfinite(b)) atomicMin(status, (unsigned long long)gj * (unsigned long long)dim + (unsigned long long)gi);
            s[e] = gi == gj ? a : 0.5 * (a + b);
            S[(size_t)gi * dim + gj] = s[e];
        }
    }
    if (bx == by) return;                               // the diagonal tile is its own mirror image
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) t[ty + 8 * e][tx] = s[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = ty + 8 * e, gi = 32 * bx + r, gj = 32 * by + tx;
        if (gi < dim && gj < dim) S[(size_t)gi * dim + gj] = t[tx][r];
    }
}

// Diagonal tile J: the sums over the earlier block columns, then the tile's factor, right-looking inside the tile (every subtraction is
// the next term of its entry's sum, k ascending).  Rows and columns past dim are an identity block: they change no other entry.
__global__ __launch_bounds__(256) void k_mf_diag(const double* __restrict__ S, double* U, int dim, int J, unsigned long long* status)
{
    __shared__ double lds[MF_UNION];
    __shared__ double dg[MF_B];
    if (*status != kMfOk) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = MF_B * J;
    mf_d4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 16 * wave + (lane >> 4) + 4 * i, c = 16 * nt + (lane & 15);
            acc[nt][i] = (j0 + r < dim && j0 + c < dim) ? S[(size_t)(j0 + r) * dim + j0 + c] : (r == c ? 1.0 : 0.0);
        }
    mf_accumulate<true>(U, j0, U, j0, dim, 0, j0, lds, acc);
    double* T = lds;
    mf_store_tile<false>(acc, T);
    for (int j = 0; j < MF_B; ++j) {
        __syncthreads();
        const double s = T[j * MF_LDT + j];
        if (tid == 0) {
            if (!(s > 0.0) || !isfinite(s)) atomicMin(status, kMfPivot + (unsigned long long)(j0 + j));
            dg[j] = __dsqrt_rn(s);
        }
        const double d = __dsqrt_rn(s);
        if (tid > j && tid < MF_B) T[tid * MF_LDT + j] = __ddiv_rn(T[tid * MF_LDT + j], d);
        __syncthreads();
        for (int idx = (j + 1) * MF_B + tid; idx < MF_B * MF_B; idx += 256) {
            const int i = idx >> 6, k = idx & 63;
            if (k > j && k <= i) T[i * MF_LDT + k] = T[i * MF_LDT + k] - T[i * MF_LDT + j] * T[k * MF_LDT + j];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < MF_B * MF_B; idx += 256) {
        const int i = idx >> 6, k = idx & 63;
        if (k <= i && j0 + i < dim) U[(size_t)(j0 + i) * dim + j0 + k] = k == i ? dg[i] : T[i * MF_LDT + k];
    }
}

// The rest of block column J (header): workgroups 0 .. n_panel - 1 the panel tiles I = J + 1 + b of U, the others the tiles (J, Jc) of W.
__global__ __launch_bounds__(256) void k_mf_rest(const double* __restrict__ S, double* U, double* W, int dim, int J, int n_panel,
                                                 const unsigned long long* status)
{
    extern __shared__ double lds_dyn[];
    if (*status != kMfOk) return;
    double* T = lds_dyn;                                // the staging area first
    double* D = lds_dyn + MF_UNION;                     // U_JJ [64][64]: every lane reads the same entry
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = MF_B * J;
    for (int idx = tid; idx < MF_B * MF_B; idx += 256) {
        const int i = idx >> 6, k = idx & 63;
        D[idx] = (j0 + i < dim && k <= i) ? U[(size_t)(j0 + i) * dim + j0 + k] : (i == k ? 1.0 : 0.0);
    }
    mf_d4 acc[4];
    if ((int)blockIdx.x < n_panel) {
        const int i0 = MF_B * (J + 1 + (int)blockIdx.x);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = i0 + 16 * wave + (lane >> 4) + 4 * i, c = j0 + 16 * nt + (lane & 15);
                acc[nt][i] = r < dim ? S[(size_t)r * dim + c] : 0.0;
            }
        mf_accumulate<true>(U, i0, U, j0, dim, 0, j0, T, acc);
        mf_store_tile<true>(acc, T);                    // T[column][row]: the lanes of the substitution are the rows
        __syncthreads();
        if (wave == 0) {
            double* t = T + lane;                       // row `lane` of the tile; nobody else touches it
            for (int j = 0; j < MF_B; ++j) {
                double s = t[j * MF_LDT];
                for (int k = 0; k < j; ++k) s = s - t[k * MF_LDT] * D[j * MF_B + k];
                t[j * MF_LDT] = __ddiv_rn(s, D[j * MF_B + j]);
            }
        }
        __syncthreads();
        for (int idx = tid; idx < MF_B * MF_B; idx += 256) {
            const int i = idx >> 6, j = idx & 63;
            if (i0 + i < dim) U[(size_t)(i0 + i) * dim + j0 + j] = T[j * MF_LDT + i];
        }
    } else {
        const int Jc = (int)blockIdx.x - n_panel, c0 = MF_B * Jc;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 16 * wave + (lane >> 4) + 4 * i, c = 16 * nt + (lane & 15);
                acc[nt][i] = (Jc == J && r == c) ? 1.0 : 0.0;
            }
        mf_accumulate<false>(U, j0, W, c0, dim, c0, j0, T, acc);
        mf_store_tile<false>(acc, T);
        __syncthreads();
        if (wave == 0) {
            double* t = T + lane;                       // column `lane` of the tile
            for (int i = 0; i < MF_B; ++i) {
                double s = t[i * MF_LDT];
                for (int k = 0; k < i; ++k) s = s - D[i * MF_B + k] * t[k * MF_LDT];
                t[i * MF_LDT] = __ddiv_rn(s, D[i * MF_B + i]);
            }
        }
        __syncthreads();
        for (int idx = tid; idx < MF_B * MF_B; idx += 256) {
            const int i = idx >> 6, j = idx & 63;
            if (j0 + i < dim && c0 + j < dim && (Jc < J || j <= i)) W[(size_t)(j0 + i) * dim + c0 + j] = T[i * MF_LDT + j];
        }
    }
}

hipError_t launch_metric_factor(const double* C, int dim, bool shrink, double keep, double floor_, double* S, double* U, double* W,
                                unsigned long long* status, hipStream_t st)
{
    if (dim <= 0) return hipErrorInvalidValue;
    const size_t bytes = sizeof(double) * (size_t)dim * (size_t)dim;
    if (hipError_t e = allow_dynamic_lds<k_mf_rest>(MF_REST_LDS)) return e;
    static_assert(kMfOk == ~0ull, "the status word is reset by bytes");
    if (hipError_t e = hipMemsetAsync(status, 0xFF, sizeof(unsigned long long), st)) return e;
    if (hipError_t e = hipMemsetAsync(U, 0, bytes, st)) return e;   // +0.0 above the diagonal
    if (hipError_t e = hipMemsetAsync(W, 0, bytes, st)) return e;
    const unsigned nb32 = (unsigned)((dim + 31) / 32);
    hipLaunchKernelGGL(k_mf_prepass, dim3(nb32, nb32), dim3(256), 0, st, C, S, dim, shrink ? 1 : 0, keep, floor_, status);
    const int NB = (dim + MF_B - 1) / MF_B;
    for (int J = 0; J < NB; ++J) {
        hipLaunchKernelGGL(k_mf_diag, dim3(1), dim3(256), 0, st, (const double*)S, U, dim, J, status);
        const int n_panel = NB - 1 - J;
        hipLaunchKernelGGL(k_mf_rest, dim3((unsigned)(n_panel + J + 1)), dim3(256), MF_REST_LDS, st, (const double*)S, U, W, dim, J, n_panel,
                           (const unsigned long long*)status);
    }
    return hipGetLastError();
}

}  // namespace mcd
