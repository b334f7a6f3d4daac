// marginal_capi.cpp -- C ABI of the marginal-likelihood estimators (include/mcmcdate_mvn.h: mcd_ml_estimate; mcd_marginal_run_ is what
// mcd_mh_record_marginal runs on the window of the ring that recorder.cpp checked).  Kernels: k_marginal.hip.  No CPU path.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/mcmcdate_mvn.h"
#include "marginal_device.hpp"

extern "C" int mcd_set_last_error_(int code, const char* msg);   // mvn_capi.cpp

static_assert(MCD_ML_COLS == mcd::kMlCols, "the header's constant is the kernels'");

namespace {

int lfail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mcd_set_last_error_(code, buf);
}

}  // namespace

// The checks that both entry points share: nothing is launched or allocated when one fails.  chain0: global number of the source's chain 0.
int mcd_marginal_check_(const char* who, int64_t n, int64_t batch, int64_t chain0, int n_points, const double* betas)
{
    const int K = n_points;
    if (K < 2 || K > mcd::kMlMaxPoints) return lfail(MCD_ERR_INVALID_ARG, "%s: n_points must be 2 .. %d (got %d)", who, mcd::kMlMaxPoints, K);
    if (!(betas[0] == 0.0)) return lfail(MCD_ERR_INVALID_ARG, "%s: betas[0] must be 0 (the prior), got %g", who, betas[0]);
    if (!(betas[K - 1] == 1.0)) return lfail(MCD_ERR_INVALID_ARG, "%s: betas[%d] must be 1 (the posterior), got %g", who, K - 1, betas[K - 1]);
    for (int p = 1; p < K; ++p)
        if (!(betas[p] > betas[p - 1])) return lfail(MCD_ERR_INVALID_ARG, "%s: betas must increase strictly (betas[%d] = %g, betas[%d] = %g)", who, p - 1, betas[p - 1], p, betas[p]);
    if (n < 1 || batch < 1) return lfail(MCD_ERR_INVALID_ARG, "%s: need n >= 1, batch >= 1 (got %lld, %lld)", who, (long long)n, (long long)batch);
    if (batch % K != 0 || chain0 % K != 0)
        return lfail(MCD_ERR_INVALID_ARG, "%s: the chains [%lld, %lld) are not whole groups of n_points = %d (chain g runs at point g mod n_points)", who,
                     (long long)chain0, (long long)(chain0 + batch), K);
    const int64_t C = batch / K;
    if (n >= ((int64_t)1 << 32) || n * C >= ((int64_t)1 << 32) || n * C < 2)
        return lfail(MCD_ERR_INVALID_ARG, "%s: n x replicates = %lld x %lld values per point; need 2 .. 2^32 - 1", who, (long long)n, (long long)C);
    return MCD_OK;
}

// One estimate of a checked source on `st` (the current device is the source's): workspace and outputs are allocated per call.  A record
// of the ring that ran at another exponent than its point's: MCD_ERR_INVALID_ARG naming it, no output written.
int mcd_marginal_run_(const char* who, const mcd::MlSrc& S, const double* betas, hipStream_t st, double* point, double* replicate, double* out)
{
    const int64_t C = S.B / S.K;
    const size_t n_work = mcd::marginal_workspace_doubles(S.B), n_pt = (size_t)S.K * mcd::kMlCols, n_rep = (size_t)C * 2;
    double* buf = nullptr;
    // betas [K], the partials, point, replicate, out [4], the error word
    hipError_t e = hipMalloc((void**)&buf, sizeof(double) * ((size_t)S.K + n_work + n_pt + n_rep + 4 + 1));
    if (e != hipSuccess) return lfail(MCD_ERR_HIP, "%s: workspace: %s", who, hipGetErrorString(e));
    double *d_betas = buf, *d_work = d_betas + S.K, *d_pt = d_work + n_work, *d_rep = d_pt + n_pt, *d_out = d_rep + n_rep;
    unsigned long long* d_err = (unsigned long long*)(d_out + 4);
    unsigned long long err = 0;
    e = hipMemcpyAsync(d_betas, betas, sizeof(double) * (size_t)S.K, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, sizeof err, st);
    if (e == hipSuccess) e = mcd::launch_marginal(S, d_betas, d_work, d_pt, d_rep, d_out, d_err, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && err == 0) {
        if (point) e = hipMemcpyAsync(point, d_pt, sizeof(double) * n_pt, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && replicate) e = hipMemcpyAsync(replicate, d_rep, sizeof(double) * n_rep, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out) e = hipMemcpyAsync(out, d_out, sizeof(double) * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipFree(buf);
    if (e != hipSuccess) return lfail(MCD_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    if (err != 0) {
        const int64_t i = (int64_t)(err & 0x7fffffffffffffffull);
        return lfail(MCD_ERR_INVALID_ARG, "%s: sample %lld of chain %lld was not recorded at betas[%lld] = %g: the window holds samples from before mcd_mh_set_power or from other exponents",
                     who, (long long)(i / S.B), (long long)(i % S.B), (long long)((i % S.B) % S.K), betas[(i % S.B) % S.K]);
    }
    return MCD_OK;
}

extern "C" int mcd_ml_estimate(int64_t n, int64_t batch, const double* ll, int on_device, int device_id, int n_points, const double* betas,
                               double* point, double* replicate, double* out)
{
    const char* who = "mcd_ml_estimate";
    if (!ll || !betas) return lfail(MCD_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (int rc = mcd_marginal_check_(who, n, batch, 0, n_points, betas)) return rc;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return lfail(MCD_ERR_NO_DEVICE, "%s: no HIP device", who);
    if (device_id < 0 || device_id >= count) return lfail(MCD_ERR_INVALID_ARG, "%s: device %d of %d", who, device_id, count);
    hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) return lfail(MCD_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    double* d_ll = nullptr;
    if (!on_device) {
        const size_t bytes = sizeof(double) * (size_t)(n * batch);
        e = hipMalloc((void**)&d_ll, bytes);
        if (e == hipSuccess) e = hipMemcpy(d_ll, ll, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (d_ll) (void)hipFree(d_ll);
            return lfail(MCD_ERR_HIP, "%s: copy of the ln likelihoods: %s", who, hipGetErrorString(e));
        }
    }
    mcd::MlSrc S{};
    S.base = on_device ? ll : d_ll;
    S.n = n;
    S.B = batch;
    S.K = n_points;
    const int rc = mcd_marginal_run_(who, S, betas, nullptr, point, replicate, out);
    if (d_ll) (void)hipFree(d_ll);
    return rc;
}
