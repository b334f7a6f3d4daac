// k_summary.hip -- posterior summaries and convergence diagnostics of a trace of n samples x B chains x Q quantities (summary_device.hpp):
// per quantity the pooled mean and maximum-likelihood variance, minimum, maximum, the two order statistics of the 95 % interval (exact:
// elements of the input), split R-hat and the effective sample size with Geyer's initial monotone sequence; per chain and quantity mean,
// unbiased variance, minimum, maximum.  Every output is a pure function of the samples: no floating-point atomics, every sum in a fixed
// order, so two calls on the same data return the same bits.  Five ordinary launches on one stream:
//   k_sum_pass1    per (chain, quantity): sums of the two halves (the oldest sample apart when n is odd), min, max, NaN flag
//   k_sum_pass2    ... sums of squared deviations about the halves' means and about the chain's mean (two passes, never sum x^2)
//   k_sum_select   the two order statistics by a most-significant-digit radix select on order-preserving 64-bit keys
//   k_sum_acov     sums over the split sequences of the lagged products of the centred values, lags 0 .. max_lag
//   k_sum_final    combines all of it per quantity
// Lanes = 64 consecutive quantities everywhere: a wave's load of one (sample, chain) is one contiguous 512-byte row.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <limits>

#include "lds_optin.hpp"
#include "mvn_kernels.h"
#include "summary_device.hpp"

namespace mcd {

namespace {

// what a lane reads of a record: the double at `off`; mode 1: times the record's tH (an age), mode 2: (off + off[1]) + off[2] (ln posterior)
struct SumCol {
    int64_t off;
    int mode;
    bool on;
};

__device__ __forceinline__ SumCol sum_col(const SumSrc& S, int64_t q)
{
    SumCol c{q, 0, q < S.Q};
    if (!S.ring || !c.on) return c;
    const int64_t nn = S.n_nodes;
    if (q < nn) c.mode = 1;
    else if (q < 2 * nn) c.off = S.ld + (q - nn);
    else if (q < 2 * nn + 8) c.off = 2 * S.ld + (q - 2 * nn);
    else {
        c.off = 2 * S.ld + 5;
        c.mode = 2;
    }
    return c;
}
// rows: sample k of the window lives in row k (plain) or slot (first + k) mod capacity (ring); walked with row_next, one modulo per walk
__device__ __forceinline__ int64_t sum_row(const SumSrc& S, int64_t k) { return S.ring ? (S.first + k) % S.cap : k; }
__device__ __forceinline__ int64_t row_next(const SumSrc& S, int64_t row)
{
    ++row;
    return (S.ring && row == S.cap) ? 0 : row;
}
__device__ __forceinline__ const double* sum_rec(const SumSrc& S, int64_t row, int64_t b)
{
    return S.base + (row * S.B + b) * (S.ring ? S.stride : S.ldq);
}
__device__ __forceinline__ double sum_load(const SumSrc& S, const double* rec, const SumCol& c)
{
    if (!c.on) return 0.0;
    double v = rec[c.off];
    if (c.mode == 1) v = rec[2 * S.ld + 2] * v;
    else if (c.mode == 2) v = (v + rec[c.off + 1]) + rec[c.off + 2];
    return v;
}

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// workspace (doubles; Qp = 64 * quantity groups): the arrays every kernel below shares
struct SumWork {
    int64_t Qp;
    double *seq_mean, *seq_m2;                 // [2 B][Qp]  sequence m = 2 b + half
    double *c_sum, *c_m2, *c_min, *c_max, *c_nan;   // [B][Qp]
    double* ord;                               // [2][Qp]
    double* part;                              // [chunks][n_lags][Qp]
};

// ---- pass 1 and 2: a wave = one chain x 64 quantities, walking the samples ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sum_pass1(SumSrc S, SumWork W)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.y * 4 + wave_id();
    if (b >= S.B) return;
    const int64_t q = (int64_t)blockIdx.x * 64 + lane;
    const SumCol c = sum_col(S, q);
    const int64_t nh = S.n / 2, d = S.n - 2 * nh;
    double s[3] = {0.0, 0.0, 0.0};             // the oldest sample of an odd n, first half, second half
    double mn = std::numeric_limits<double>::infinity(), mx = -mn;
    bool nan = false;
    int64_t row = sum_row(S, 0);
    const int64_t end[3] = {d, d + nh, S.n};
    int64_t k = 0;
    for (int part = 0; part < 3; ++part) {
        double a = 0.0;
#pragma unroll 4
        for (; k < end[part]; ++k) {
            const double v = sum_load(S, sum_rec(S, row, b), c);
            row = row_next(S, row);
            a += v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
            nan = nan || v != v;
        }
        s[part] = a;
    }
    const int64_t o = b * W.Qp + q;
    W.seq_mean[2 * o - q] = s[1] / (double)nh;                 // [(2 b) Qp + q]
    W.seq_mean[2 * o - q + W.Qp] = s[2] / (double)nh;
    W.c_sum[o] = (s[0] + s[1]) + s[2];
    W.c_min[o] = mn;
    W.c_max[o] = mx;
    W.c_nan[o] = nan ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void k_sum_pass2(SumSrc S, SumWork W)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.y * 4 + wave_id();
    if (b >= S.B) return;
    const int64_t q = (int64_t)blockIdx.x * 64 + lane;
    const SumCol c = sum_col(S, q);
    const int64_t nh = S.n / 2, d = S.n - 2 * nh;
    const int64_t o = b * W.Qp + q;
    const double mc = W.c_sum[o] / (double)S.n;
    const double mh[3] = {0.0, W.seq_mean[2 * o - q], W.seq_mean[2 * o - q + W.Qp]};
    double m2c = 0.0, m2h[3] = {0.0, 0.0, 0.0};
    int64_t row = sum_row(S, 0);
    const int64_t end[3] = {d, d + nh, S.n};
    int64_t k = 0;
    // a constant sequence has the variance 0 exactly, whatever the rounding of its mean (a quantity no proposal moved, a leaf's age)
    const bool flat = W.c_min[o] == W.c_max[o];
    for (int part = 0; part < 3; ++part) {
        double a = 0.0, first = 0.0;
        bool same = true;
        const double m = mh[part];
        const int64_t k0 = k;
#pragma unroll 4
        for (; k < end[part]; ++k) {
            const double v = sum_load(S, sum_rec(S, row, b), c);
            row = row_next(S, row);
            first = (k == k0) ? v : first;
            same = same && v == first;
            const double e = v - mc, f = v - m;
            m2c += e * e;
            a += f * f;
        }
        m2h[part] = same ? 0.0 : a;
    }
    W.c_m2[o] = flat ? 0.0 : m2c;
    W.seq_m2[2 * o - q] = m2h[1];
    W.seq_m2[2 * o - q + W.Qp] = m2h[2];
}

// ---- the two order statistics: radix select, 8 passes of 8 bits, one workgroup per 64 quantities --------------------------------------------
// Keys: the double's bits with the sign flipped (positive) or all bits flipped (negative): unsigned order = numeric order, -0 below +0.
// Each pass counts, per quantity, the byte below the prefix resolved so far in a histogram [256][64] of uint32 per rank (lane j owns column
// j: the 32 lanes of an LDS access group hit 32 different banks); the waves split the (sample, chain) pairs and add with LDS integer adds.
__device__ __forceinline__ uint64_t sel_key(double v)
{
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double sel_value(uint64_t k)
{
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

__global__ __launch_bounds__(64 * kSelWaves) void k_sum_select(SumSrc S, SumWork W, uint32_t rank0, uint32_t rank1)
{
    extern __shared__ uint32_t sel_hist[];                     // [2][256][64]
    __shared__ uint64_t pre[2][64];
    __shared__ uint32_t rem[2][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int64_t q = (int64_t)blockIdx.x * 64 + lane;
    const SumCol c = sum_col(S, q);
    if (tid < 128) {
        pre[tid >> 6][lane] = 0;
        rem[tid >> 6][lane] = (tid >> 6) ? rank1 : rank0;
    }
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int i = tid; i < 2 * 256 * 64; i += 64 * kSelWaves) sel_hist[i] = 0;
        __syncthreads();
        // the bits above this pass's byte (pass 0: none -- a shift by 64 is not defined, so two shifts)
        const uint64_t p0 = pre[0][lane] >> shift >> 8, p1 = pre[1][lane] >> shift >> 8;
        int64_t k = wave / S.B, b = wave - k * S.B, row = sum_row(S, k);
#pragma unroll 2
        while (k < S.n) {
            const uint64_t key = sel_key(sum_load(S, sum_rec(S, row, b), c));
            const uint64_t hi = key >> shift >> 8;
            const uint32_t digit = (uint32_t)(key >> shift) & 255u;
            if (hi == p0) atomicAdd(&sel_hist[digit * 64 + lane], 1u);
            if (hi == p1) atomicAdd(&sel_hist[(256 + digit) * 64 + lane], 1u);
            b += kSelWaves;
            while (b >= S.B) {
                b -= S.B;
                ++k;
                row = row_next(S, row);
            }
        }
        __syncthreads();
        if (tid < 128) {                                       // two waves: one per rank, a lane walks its column
            const int h = tid >> 6;
            uint32_t r = rem[h][lane];
            int dsel = 255;
            for (int dgt = 0; dgt < 256; ++dgt) {
                const uint32_t cnt = sel_hist[(h * 256 + dgt) * 64 + lane];
                if (r < cnt) {
                    dsel = dgt;
                    break;
                }
                r -= cnt;
            }
            pre[h][lane] |= (uint64_t)dsel << shift;
            rem[h][lane] = r;
        }
        __syncthreads();
    }
    if (tid < 128) W.ord[(tid >> 6) * W.Qp + q] = sel_value(pre[tid >> 6][lane]);
}

// ---- autocovariance sums: four waves share a sliding window of the centred values of one split sequence in LDS ---------------------------
// Workgroup = 64 quantities x one chunk of the 2 B split sequences; wave w holds the sums of lags [64 w, 64 w + 64) in registers and keeps
// adding over the chunk's sequences (what the estimate needs is the mean over sequences).  The window is a ring of kAcovRows rows
// [64 lanes]: per tile of kAcovTile samples the waves stage the centred values, then every wave multiplies each new value with the 64 older
// ones of its lags.  Rows of samples before the sequence's start hold zeros, so that no product needs a bounds test.
__global__ __launch_bounds__(256) void k_sum_acov(SumSrc S, SumWork W, int n_lags, int64_t seq_per_chunk)
{
    extern __shared__ double win[];                            // [kAcovRows][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int64_t q = (int64_t)blockIdx.x * 64 + lane;
    const SumCol c = sum_col(S, q);
    const int64_t nh = S.n / 2, d = S.n - 2 * nh, M = 2 * S.B;
    const int t0 = wave * kAcovLags;
    const bool work = t0 < n_lags;
    double acc[kAcovLags];
#pragma unroll
    for (int t = 0; t < kAcovLags; ++t) acc[t] = 0.0;
    const int64_t m0 = (int64_t)blockIdx.y * seq_per_chunk, m1 = (m0 + seq_per_chunk < M) ? m0 + seq_per_chunk : M;
    for (int64_t m = m0; m < m1; ++m) {
        const int64_t b = m >> 1, k0 = d + (m & 1) * nh;
        const double mean = W.seq_mean[m * W.Qp + q];
        for (int i = tid; i < kAcovRows * 64; i += 256) win[i] = 0.0;
        __syncthreads();
        for (int64_t i0 = 0; i0 < nh; i0 += kAcovTile) {
            {                                                  // stage: wave w takes rows i0 + 8 w .. + 8
                const int64_t i = i0 + wave * (kAcovTile / 4);
                int64_t row = sum_row(S, k0 + i);
#pragma unroll
                for (int r = 0; r < kAcovTile / 4; ++r) {
                    double v = 0.0;
                    if (i + r < nh) v = sum_load(S, sum_rec(S, row, b), c) - mean;
                    row = row_next(S, row);
                    win[(int)((i + r) % kAcovRows) * 64 + lane] = v;
                }
            }
            __syncthreads();
            if (work) {
                const int64_t i1 = (i0 + kAcovTile < nh) ? i0 + kAcovTile : nh;
                for (int64_t i = i0; i < i1; ++i) {
                    const double ci = win[(int)(i % kAcovRows) * 64 + lane];
                    int row = (int)((i - t0 + 2 * (int64_t)kAcovRows) % kAcovRows);     // i - t0 >= -192 > -kAcovRows
#pragma unroll
                    for (int t = 0; t < kAcovLags; ++t) {
                        acc[t] += ci * win[row * 64 + lane];
                        row = row ? row - 1 : kAcovRows - 1;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (work) {
#pragma unroll
        for (int t = 0; t < kAcovLags; ++t)
            if (t0 + t < n_lags) W.part[((int64_t)blockIdx.y * n_lags + t0 + t) * W.Qp + q] = acc[t];
    }
}

// ---- the combination: one lane per quantity, every sum in index order ------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sum_final(SumSrc S, SumWork W, int max_lag, int64_t chunks, double* __restrict__ pooled, double* __restrict__ per_chain)
{
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= S.Q) return;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const int64_t B = S.B, n = S.n, nh = n / 2, M = 2 * B, Qp = W.Qp;
    const double l = (double)n * (double)B;
    bool nan = false;
    double sum = 0.0, mn = std::numeric_limits<double>::infinity(), mx = -mn;
    for (int64_t b = 0; b < B; ++b) {
        sum += W.c_sum[b * Qp + q];
        const double a = W.c_min[b * Qp + q], z = W.c_max[b * Qp + q];
        mn = a < mn ? a : mn;
        mx = z > mx ? z : mx;
        nan = nan || W.c_nan[b * Qp + q] != 0.0;
    }
    const double mean = sum / l;
    double m2 = 0.0;
    for (int64_t b = 0; b < B; ++b) {                          // Chan's combination of the chains' two-pass sums
        const double e = W.c_sum[b * Qp + q] / (double)n - mean;
        m2 += W.c_m2[b * Qp + q] + (double)n * (e * e);
    }
    double* out = pooled + q * kSumCols;
    if (per_chain) {
        for (int64_t b = 0; b < B; ++b) {
            double* pc = per_chain + (b * S.Q + q) * 4;
            pc[0] = nan ? qnan : W.c_sum[b * Qp + q] / (double)n;
            pc[1] = (nan || n < 2) ? qnan : W.c_m2[b * Qp + q] / (double)(n - 1);
            pc[2] = nan ? qnan : W.c_min[b * Qp + q];
            pc[3] = nan ? qnan : W.c_max[b * Qp + q];
        }
    }
    if (nan) {
        for (int i = 0; i < kSumCols; ++i) out[i] = qnan;
        return;
    }
    out[0] = mean;
    out[1] = m2 / l;
    out[2] = mn;
    out[3] = mx;
    out[4] = W.ord[q];
    out[5] = W.ord[Qp + q];
    out[6] = out[7] = out[8] = qnan;
    if (nh < 2) return;
    // split R-hat over the M = 2 B sequences of nh samples
    double w = 0.0, mm = 0.0;
    for (int64_t m = 0; m < M; ++m) {
        w += W.seq_m2[m * Qp + q] / (double)(nh - 1);
        mm += W.seq_mean[m * Qp + q];
    }
    w /= (double)M;
    mm /= (double)M;
    double bv = 0.0;
    for (int64_t m = 0; m < M; ++m) {
        const double e = W.seq_mean[m * Qp + q] - mm;
        bv += e * e;
    }
    bv = (double)nh * (bv / (double)(M - 1));
    const double varp = ((double)(nh - 1) / (double)nh) * w + bv / (double)nh;
    if (!(w == w) || !(varp == varp) || w == 0.0 || varp == 0.0 || fabs(w) == std::numeric_limits<double>::infinity() ||
        fabs(varp) == std::numeric_limits<double>::infinity())
        return;
    out[6] = sqrt(varp / w);
    if (max_lag < 1) return;
    // Geyer's initial monotone sequence on rho_t = 1 - (W - mean_m gamma_{m,t}) / var+
    const int n_lags = max_lag + 1;
    const double scale = (double)M * (double)nh;
    double tau = -1.0, prev = std::numeric_limits<double>::infinity(), last = -1.0;
    for (int k = 0; 2 * k + 1 <= max_lag; ++k) {
        double rho[2];
        for (int j = 0; j < 2; ++j) {
            double g = 0.0;
            for (int64_t ch = 0; ch < chunks; ++ch) g += W.part[(ch * n_lags + 2 * k + j) * Qp + q];
            rho[j] = 1.0 - (w - g / scale) / varp;
        }
        double p = rho[0] + rho[1];
        if (!(p > 0.0)) break;
        p = p < prev ? p : prev;
        tau += 2.0 * p;
        prev = p;
        last = (double)(2 * k + 1);
    }
    const double floor_tau = 1.0 / log10(scale);
    tau = tau > floor_tau ? tau : floor_tau;
    out[7] = scale / tau;
    out[8] = last;
}

SumWork carve(const SumSrc& S, int n_lags, double* work)
{
    SumWork W{};
    const int64_t Qp = 64 * ((S.Q + 63) / 64), B = S.B;
    W.Qp = Qp;
    double* p = work;
    auto take = [&](int64_t rows) {
        double* r = p;
        p += rows * Qp;
        return r;
    };
    W.seq_mean = take(2 * B);
    W.seq_m2 = take(2 * B);
    W.c_sum = take(B);
    W.c_m2 = take(B);
    W.c_min = take(B);
    W.c_max = take(B);
    W.c_nan = take(B);
    W.ord = take(2);
    W.part = take(summary_chunks(S.B, S.Q) * n_lags);
    return W;
}

}  // namespace

// enough workgroups for the chip where the quantities alone do not give them (256 compute units; one 144 KiB workgroup each)
int64_t summary_chunks(int64_t B, int64_t Q)
{
    const int64_t G = (Q + 63) / 64, M = 2 * B;
    const int64_t want = (512 + G - 1) / G;
    return want < M ? want : M;
}

size_t summary_workspace_doubles(int64_t B, int64_t Q, int n_lags)
{
    const int64_t Qp = 64 * ((Q + 63) / 64);
    return (size_t)(Qp * (9 * B + 2 + summary_chunks(B, Q) * n_lags));
}

hipError_t launch_summary(const SumSrc& S, int max_lag, double* work, double* d_pooled, double* d_per_chain, hipStream_t st)
{
    const int n_lags = max_lag > 0 ? max_lag + 1 : 0;
    const SumWork W = carve(S, n_lags, work);
    const int64_t G = W.Qp / 64, l = S.n * S.B;
    if (G > 0x7fffffffLL || (S.B + 3) / 4 > 65535 || l < 2 || l >= ((int64_t)1 << 32) || max_lag > kSumMaxLag) return hipErrorInvalidValue;
    const dim3 gc((unsigned)G, (unsigned)((S.B + 3) / 4));
    hipLaunchKernelGGL(k_sum_pass1, gc, dim3(256), 0, st, S, W);
    hipLaunchKernelGGL(k_sum_pass2, gc, dim3(256), 0, st, S, W);
    // summarize_node_ages: sorted[i] and sorted[i + m - 1], i = floor(0.025 l), m = floor(0.95 l), in the same fp64 products
    const double lf = (double)l;
    const int64_t i_ci = (int64_t)floor(lf * 0.025), n_ci = (int64_t)floor(lf * 0.95);
    static const size_t sel_lds = 2 * 256 * 64 * sizeof(uint32_t), acov_lds = (size_t)kAcovRows * 64 * sizeof(double);
    if (hipError_t e = allow_dynamic_lds<k_sum_select>((int)sel_lds)) return e;
    hipLaunchKernelGGL(k_sum_select, dim3((unsigned)G), dim3(64 * kSelWaves), sel_lds, st, S, W, (uint32_t)i_ci, (uint32_t)(i_ci + n_ci - 1));
    const int64_t chunks = summary_chunks(S.B, S.Q);
    if (n_lags > 0 && S.n / 2 >= 2) {
        const int64_t per = (2 * S.B + chunks - 1) / chunks;
        if (hipError_t e = allow_dynamic_lds<k_sum_acov>((int)acov_lds)) return e;
        hipLaunchKernelGGL(k_sum_acov, dim3((unsigned)G, (unsigned)chunks), dim3(256), acov_lds, st, S, W, n_lags, per);
    }
    hipLaunchKernelGGL(k_sum_final, dim3((unsigned)G), dim3(64), 0, st, S, W, (n_lags > 0 && S.n / 2 >= 2) ? max_lag : 0, chunks, d_pooled, d_per_chain);
    return hipGetLastError();
}

}  // namespace mcd
