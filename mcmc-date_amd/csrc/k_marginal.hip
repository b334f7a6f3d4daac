// k_marginal.hip -- ln Z from the ln likelihoods of power-posterior chains (marginal_device.hpp; definitions: include/mcmcdate_mvn.h,
// mcd_ml_estimate): stepping stones (Xie et al. 2011) and the trapezoid of thermodynamic integration, pooled over the replicates and per
// replicate.  Four launches, each a pure function of what the one before wrote:
//   k_ml_chain   one wave per chain, lanes striding over its n samples, two passes: {mean, M2, max, min, S = sum exp(delta (x - max))}
//   k_ml_point   one wave per path point, lanes striding over its C replicates: the pooled columns of the point
//   k_ml_rep     one wave per replicate, lanes striding over the points: the replicate's stepping-stone and trapezoid sums
//   k_ml_total   one wave: the four totals
// Every lane adds its terms in index order and the lanes are combined by the same butterfly (xor 32, 16, ... 1: fp64 addition commutes, so
// every lane ends with the same bits): a fixed order, no atomics, plain vector stores; the build contracts no multiply-add.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "marginal_device.hpp"

namespace mcd {

namespace {

__device__ __forceinline__ int ml_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ double ml_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double ml_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double ml_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
// ln likelihood of (sample k, chain b); ring: the record's word 2 ld + 6, the exponent behind it in word 2 ld + 8
__device__ __forceinline__ const double* ml_at(const MlSrc& S, int64_t k, int64_t b)
{
    if (!S.ring) return S.base + (k * S.B + b);
    return S.base + (((S.first + k) % S.cap) * S.B + b) * S.stride + (2 * S.ld + 6);
}
__device__ __forceinline__ double ml_delta(const double* __restrict__ betas, int K, int p) { return p + 1 < K ? betas[p + 1] - betas[p] : 0.0; }

__global__ __launch_bounds__(256) void k_ml_chain(MlSrc S, const double* __restrict__ betas, double* __restrict__ part,
                                                  unsigned long long* __restrict__ err)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + ml_wave();
    if (b >= S.B) return;                                    // wave-uniform
    const int p = (int)(b % S.K);                            // (the first chain of the source is the first of a group of K)
    const double want = betas[p], delta = ml_delta(betas, S.K, p);
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    double s = 0.0, mx = -inf, mn = inf;
    bool bad = false, stray = false;
    for (int64_t k = lane; k < S.n; k += 64) {
        const double* at = ml_at(S, k, b);
        const double x = at[0];
        if (S.ring && __double_as_longlong(at[2]) != __double_as_longlong(want) && !stray) {
            // recorded before mcd_mh_set_power, or under other exponents: one 8-byte store names the record (any one is enough)
            stray = true;
            *err = 0x8000000000000000ull | (unsigned long long)(k * S.B + b);
        }
        s += x;
        bad |= x != x;
        mx = fmax(mx, x);
        mn = fmin(mn, x);
    }
    if (__ballot(stray) != 0) return;                        // nothing of this chain is written
    s = ml_sum(s);
    mx = ml_max(mx);
    mn = ml_min(mn);
    const bool any_bad = __ballot(bad) != 0;
    const double m = mx == mn ? mx : s / (double)S.n;        // a constant chain: its mean exactly, whatever the rounding of the sum
    double q = 0.0, e = 0.0;
    for (int64_t k = lane; k < S.n; k += 64) {
        const double x = ml_at(S, k, b)[0];
        const double d = x - m;
        q += d * d;
        e += exp(delta * (x - mx));
    }
    q = ml_sum(q);
    e = ml_sum(e);
    if (lane == 0) {
        double* o = part + b * kMlPart;
        o[0] = any_bad ? nan : m;
        o[1] = any_bad ? nan : q;
        o[2] = any_bad ? nan : mx;
        o[3] = any_bad ? nan : mn;
        o[4] = any_bad ? nan : e;
    }
}

// point[p] = mean, unbiased variance, minimum, maximum, ln r_p over the n C values of the point.  All chains hold n values, so the pooled
// mean is the mean of the C means M and the pooled M2 = sum_r M2_r + n sum_r (m_r - M)^2 (Chan's update for equal counts, two passes over
// the means); the chains' S are rescaled from their own maximum to the point's.
__global__ __launch_bounds__(256) void k_ml_point(MlSrc S, const double* __restrict__ betas, const double* __restrict__ part,
                                                  double* __restrict__ point)
{
    const int lane = threadIdx.x & 63;
    const int p = (int)blockIdx.x * 4 + ml_wave();
    if (p >= S.K) return;
    const int64_t C = S.B / S.K;
    const double delta = ml_delta(betas, S.K, p);
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    double sm = 0.0, MX = -inf, MN = inf;
    bool bad = false;
    for (int64_t r = lane; r < C; r += 64) {
        const double* pr = part + (r * S.K + p) * kMlPart;
        sm += pr[0];
        bad |= pr[0] != pr[0];
        MX = fmax(MX, pr[2]);
        MN = fmin(MN, pr[3]);
    }
    sm = ml_sum(sm);
    MX = ml_max(MX);
    MN = ml_min(MN);
    const bool any_bad = __ballot(bad) != 0;
    const double M = MX == MN ? MX : sm / (double)C;
    double q2 = 0.0, qm = 0.0, e = 0.0;
    for (int64_t r = lane; r < C; r += 64) {
        const double* pr = part + (r * S.K + p) * kMlPart;
        const double d = pr[0] - M;
        q2 += pr[1];
        qm += d * d;
        e += pr[4] * exp(delta * (pr[2] - MX));
    }
    q2 = ml_sum(q2);
    qm = ml_sum(qm);
    e = ml_sum(e);
    if (lane == 0) {
        const double l = (double)S.n * (double)C;
        double* o = point + (int64_t)p * kMlCols;
        o[0] = any_bad ? nan : M;
        o[1] = any_bad ? nan : (q2 + (double)S.n * qm) / (l - 1.0);
        o[2] = any_bad ? nan : MN;
        o[3] = any_bad ? nan : MX;
        o[4] = any_bad || p + 1 >= S.K ? nan : delta * MX + log(e / l);
    }
}

// replicate[r] = sum_p [delta_p mx_{p,r} + ln(S_{p,r} / n)],  sum_p delta_p (m_{p,r} + m_{p+1,r}) / 2: the path of replicate r's chains alone
__global__ __launch_bounds__(256) void k_ml_rep(MlSrc S, const double* __restrict__ betas, const double* __restrict__ part,
                                                double* __restrict__ replicate)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + ml_wave();
    if (r >= S.B / S.K) return;
    const double* pr = part + r * S.K * kMlPart;
    double ss = 0.0, ti = 0.0;
    for (int p = lane; p + 1 < S.K; p += 64) {
        const double delta = betas[p + 1] - betas[p];
        const double* a = pr + (int64_t)p * kMlPart;
        ss += delta * a[2] + log(a[4] / (double)S.n);
        ti += delta * (a[0] + a[kMlPart]) / 2.0;
    }
    ss = ml_sum(ss);
    ti = ml_sum(ti);
    if (lane == 0) {
        replicate[2 * r] = ss;
        replicate[2 * r + 1] = ti;
    }
}

// sd(v_r) / sqrt(C) over column c of replicate[C][2], unbiased, two passes; equal values: 0 exactly; C = 1 or a NaN: NaN
__device__ __forceinline__ double ml_se(const double* __restrict__ replicate, int64_t C, int c, int lane)
{
    const double inf = __builtin_inf();
    double s = 0.0, mx = -inf, mn = inf;
    for (int64_t r = lane; r < C; r += 64) {
        const double v = replicate[2 * r + c];
        s += v;
        mx = fmax(mx, v);
        mn = fmin(mn, v);
    }
    s = ml_sum(s);
    mx = ml_max(mx);
    mn = ml_min(mn);
    const double m = s / (double)C;
    double q = 0.0;
    for (int64_t r = lane; r < C; r += 64) {
        const double d = replicate[2 * r + c] - m;
        q += d * d;
    }
    q = ml_sum(q);
    if (C < 2 || s != s) return __builtin_nan("");
    return mx == mn ? 0.0 : sqrt(q / (double)(C - 1)) / sqrt((double)C);
}

__global__ __launch_bounds__(64) void k_ml_total(MlSrc S, const double* __restrict__ betas, const double* __restrict__ point,
                                                 const double* __restrict__ replicate, double* __restrict__ out)
{
    const int lane = threadIdx.x;
    double ss = 0.0, ti = 0.0;
    for (int p = lane; p + 1 < S.K; p += 64) {
        const double delta = betas[p + 1] - betas[p];
        const double* a = point + (int64_t)p * kMlCols;
        ss += a[4];
        ti += delta * (a[0] + a[kMlCols]) / 2.0;
    }
    ss = ml_sum(ss);
    ti = ml_sum(ti);
    const int64_t C = S.B / S.K;
    const double se_ss = ml_se(replicate, C, 0, lane), se_ti = ml_se(replicate, C, 1, lane);
    if (lane == 0) {
        out[0] = ss;
        out[1] = se_ss;
        out[2] = ti;
        out[3] = se_ti;
    }
}

}  // namespace

hipError_t launch_marginal(const MlSrc& S, const double* d_betas, double* work, double* d_point, double* d_replicate, double* d_out,
                           unsigned long long* d_err, hipStream_t st)
{
    if (S.K < 2 || S.K > kMlMaxPoints || S.n < 1 || S.B < S.K || S.B % S.K != 0 || (S.B + 3) / 4 > 0x7fffffffLL ||
        (S.ring && (S.cap < 1 || S.first < 0 || S.first >= S.cap || S.n > S.cap)))
        return hipErrorInvalidValue;
    const int64_t C = S.B / S.K;
    hipLaunchKernelGGL(k_ml_chain, dim3((unsigned)((S.B + 3) / 4)), dim3(256), 0, st, S, d_betas, work, d_err);
    hipLaunchKernelGGL(k_ml_point, dim3((unsigned)((S.K + 3) / 4)), dim3(256), 0, st, S, d_betas, (const double*)work, d_point);
    hipLaunchKernelGGL(k_ml_rep, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, st, S, d_betas, (const double*)work, d_replicate);
    hipLaunchKernelGGL(k_ml_total, dim3(1), dim3(64), 0, st, S, d_betas, (const double*)d_point, (const double*)d_replicate, d_out);
    return hipGetLastError();
}

}  // namespace mcd
