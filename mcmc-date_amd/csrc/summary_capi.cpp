// summary_capi.cpp -- C ABI of the posterior summaries and convergence diagnostics of a trace (include/mcmcdate_mvn.h: mcd_trace_summary;
// mcd_summary_run_ is what mcd_*_record_summary run on the window of the ring that recorder.cpp checked).  Kernels: k_summary.hip.  No CPU path.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/mcmcdate_mvn.h"
#include "mvn_kernels.h"
#include "summary_device.hpp"

extern "C" int mcd_set_last_error_(int code, const char* msg);   // mvn_capi.cpp

static_assert(MCD_SUMMARY_COLS == mcd::kSumCols && MCD_SUMMARY_MAX_LAG == mcd::kSumMaxLag, "the header's constants are the kernels'");

namespace {

int sfail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mcd_set_last_error_(code, buf);
}

}  // namespace

// The checks that both entry points share: nothing is launched or allocated when one fails.
int mcd_summary_check_(const char* who, int64_t n, int64_t batch, int64_t q, int32_t max_lag)
{
    if (n < 1 || batch < 1 || q < 1) return sfail(MCD_ERR_INVALID_ARG, "%s: need n >= 1, batch >= 1, q >= 1 (got %lld, %lld, %lld)", who, (long long)n, (long long)batch, (long long)q);
    if (batch > 262140) return sfail(MCD_ERR_INVALID_ARG, "%s: at most 262140 chains (got %lld)", who, (long long)batch);
    if (n >= ((int64_t)1 << 32) || n * batch >= ((int64_t)1 << 32))
        return sfail(MCD_ERR_INVALID_ARG, "%s: n x batch = %lld x %lld pooled values; the rank counters hold fewer than 2^32", who, (long long)n, (long long)batch);
    if (n * batch < 2) return sfail(MCD_ERR_INVALID_ARG, "%s: the 95 %% interval needs at least 2 pooled values", who);
    if (max_lag != 0) {
        if (max_lag < 0 || max_lag % 2 == 0) return sfail(MCD_ERR_INVALID_ARG, "%s: max_lag must be odd (or 0: no effective sample size), got %d", who, (int)max_lag);
        if (max_lag > MCD_SUMMARY_MAX_LAG) return sfail(MCD_ERR_INVALID_ARG, "%s: max_lag %d is above MCD_SUMMARY_MAX_LAG = %d", who, (int)max_lag, MCD_SUMMARY_MAX_LAG);
        if (max_lag > n / 2 - 1)
            return sfail(MCD_ERR_INVALID_ARG, "%s: max_lag %d needs split sequences of more than %d samples, they have %lld", who, (int)max_lag, (int)max_lag, (long long)(n / 2));
    }
    return MCD_OK;
}

// One summary of a checked source on `st` (the current device is the source's): workspace and outputs are allocated per call.
int mcd_summary_run_(const mcd::SumSrc& S, int32_t max_lag, hipStream_t st, double* pooled, double* per_chain)
{
    const int n_lags = max_lag > 0 ? max_lag + 1 : 0;
    const size_t n_pool = (size_t)S.Q * mcd::kSumCols, n_pc = per_chain ? (size_t)S.B * (size_t)S.Q * 4 : 0;
    double* buf = nullptr;
    hipError_t e = hipMalloc((void**)&buf, sizeof(double) * (mcd::summary_workspace_doubles(S.B, S.Q, n_lags) + n_pool + n_pc));
    if (e != hipSuccess) return sfail(MCD_ERR_HIP, "summary: workspace: %s", hipGetErrorString(e));
    double* d_pool = buf + mcd::summary_workspace_doubles(S.B, S.Q, n_lags);
    double* d_pc = per_chain ? d_pool + n_pool : nullptr;
    e = mcd::launch_summary(S, max_lag, buf, d_pool, d_pc, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pooled, d_pool, sizeof(double) * n_pool, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && per_chain) e = hipMemcpyAsync(per_chain, d_pc, sizeof(double) * n_pc, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) return sfail(MCD_ERR_HIP, "summary: %s", hipGetErrorString(e));
    return MCD_OK;
}

extern "C" int mcd_trace_summary(int64_t n, int64_t batch, int64_t q, int64_t ldq, const double* X, int on_device, int device_id, int32_t max_lag,
                                 double* pooled, double* per_chain)
{
    if (!X || !pooled) return sfail(MCD_ERR_INVALID_ARG, "mcd_trace_summary: NULL argument");
    if (int rc = mcd_summary_check_("mcd_trace_summary", n, batch, q, max_lag)) return rc;
    if (ldq < q) return sfail(MCD_ERR_INVALID_ARG, "mcd_trace_summary: ldq = %lld is below q = %lld", (long long)ldq, (long long)q);
    if (ldq > ((int64_t)1 << 50) / (n * batch)) return sfail(MCD_ERR_INVALID_ARG, "mcd_trace_summary: %lld x %lld rows of %lld doubles", (long long)n, (long long)batch, (long long)ldq);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return sfail(MCD_ERR_NO_DEVICE, "mcd_trace_summary: no HIP device");
    if (device_id < 0 || device_id >= count) return sfail(MCD_ERR_INVALID_ARG, "mcd_trace_summary: device %d of %d", device_id, count);
    hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) return sfail(MCD_ERR_HIP, "mcd_trace_summary: %s", hipGetErrorString(e));
    double* d_X = nullptr;
    if (!on_device) {
        const size_t bytes = sizeof(double) * (size_t)(n * batch * ldq);
        e = hipMalloc((void**)&d_X, bytes);
        if (e == hipSuccess) e = hipMemcpy(d_X, X, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (d_X) (void)hipFree(d_X);
            return sfail(MCD_ERR_HIP, "mcd_trace_summary: copy of the trace: %s", hipGetErrorString(e));
        }
    }
    mcd::SumSrc S{};
    S.base = on_device ? X : d_X;
    S.n = n;
    S.B = batch;
    S.Q = q;
    S.ldq = ldq;
    const int rc = mcd_summary_run_(S, max_lag, nullptr, pooled, per_chain);
    if (d_X) (void)hipFree(d_X);
    return rc;
}
