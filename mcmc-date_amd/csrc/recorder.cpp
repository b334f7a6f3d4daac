// recorder.cpp -- host side of the sample recorder of both drivers (recorder.hpp): the ring's counts, its two device buffers, the refusal of
// a run that would overflow it, the staged fetch and the window of a summary.  Host code only; the kernels are the drivers' and k_summary.hip's.
#include "recorder.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>

#include "../../include/mcmcdate_mvn.h"

int mcd_summary_check_(const char* who, int64_t n, int64_t batch, int64_t q, int32_t max_lag);   // summary_capi.cpp
extern "C" int mcd_set_last_error_(int code, const char* msg);                                   // mvn_capi.cpp

namespace {

int rfail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mcd_set_last_error_(code, buf);
}

#define RHIP_TRY(expr)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return rfail(MCD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

}  // namespace

namespace mcd {

void Recorder::release()
{
    if (ring_) (void)hipFree(ring_);
    if (stage_) (void)hipFree(stage_);
    ring_ = stage_ = nullptr;
    c_ = RecCounts{};
}

int Recorder::begin(const char* who, const RecOn& on, int32_t period, int64_t capacity, int tail_doubles)
{
    if (active()) return rfail(MCD_ERR_INVALID_ARG, "%s: a recorder is active already (%s_end first)", who, api_);
    if (period < 1) return rfail(MCD_ERR_INVALID_ARG, "%s: period must be >= 1 (got %d)", who, (int)period);
    if (capacity < 1) return rfail(MCD_ERR_INVALID_ARG, "%s: capacity must be >= 1 sample (got %lld)", who, (long long)capacity);
    const MhRecDims& D = on.dims;
    const int64_t per_sample = D.batch * mh_rec_stride(D.ld);                      // doubles of one slot
    if (capacity > ((int64_t)1 << 50) / per_sample)
        return rfail(MCD_ERR_INVALID_ARG, "%s: %lld samples of %lld bytes each", who, (long long)capacity, (long long)per_sample * 8);
    // the fetch unpacks into a staging buffer of at most 64 MiB (at least one sample) and copies from there, piece by piece
    const int64_t out_sample = D.batch * (2 * (int64_t)D.n_nodes + 8 + tail_doubles);
    const int64_t stage = std::max<int64_t>(1, std::min<int64_t>(capacity, ((int64_t)8 << 20) / out_sample));
    RHIP_TRY(hipSetDevice(on.device));
    hipError_t e = hipMalloc((void**)&ring_, sizeof(double) * (size_t)(per_sample * capacity));
    if (e == hipSuccess) e = hipMalloc((void**)&stage_, sizeof(double) * (size_t)(out_sample * stage));
    if (e == hipSuccess) e = hipMemsetAsync(ring_, 0, sizeof(double) * (size_t)(per_sample * capacity), on.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(on.stream);
    if (e != hipSuccess) {
        release();
        return rfail(MCD_ERR_HIP, "%s: %lld samples of %lld bytes each: %s", who, (long long)capacity, (long long)per_sample * 8, hipGetErrorString(e));
    }
    stage_cap_ = stage;
    tail_ = tail_doubles;
    c_ = RecCounts{capacity, period, 0, 0};
    return MCD_OK;
}

int Recorder::room(const char* who, int64_t n) const
{
    if (!active()) return MCD_OK;
    if (c_.adds(n) > c_.free_slots())
        return rfail(MCD_ERR_INVALID_ARG, "%s: the call would record %lld samples, the recorder has %lld free slots (%s_fetch frees them)", who,
                     (long long)c_.adds(n), (long long)c_.free_slots(), api_);
    return MCD_OK;
}

int Recorder::count(const char* who, int64_t* n_samples) const
{
    if (!active()) return rfail(MCD_ERR_INVALID_ARG, "%s: no recorder is active (%s_begin first)", who, api_);
    *n_samples = c_.waiting();
    return MCD_OK;
}

int Recorder::fetch(const char* who, const RecOn& on, int64_t max_samples, int64_t* n_out, int64_t* index, double* scalars, double* heights,
                    double* rates, double* post, double* beta, double* diag)
{
    *n_out = 0;
    if (!active()) return rfail(MCD_ERR_INVALID_ARG, "%s: no recorder is active (%s_begin first)", who, api_);
    if (max_samples < 0) return rfail(MCD_ERR_INVALID_ARG, "%s: max_samples < 0", who);
    const int64_t n = std::min(c_.waiting(), max_samples), B = on.dims.batch, nn = on.dims.n_nodes;
    double* const out[5] = {scalars, heights, rates, post, beta ? beta : diag};
    const int64_t width[5] = {5, nn, nn, 3, tail_};          // doubles per (sample, chain) of the five arrays
    RHIP_TRY(hipSetDevice(on.device));
    for (int64_t done = 0; done < n; done += stage_cap_) {
        const int64_t cnt = std::min(stage_cap_, n - done);
        double* s[5] = {stage_};                             // the staging buffer's five arrays for `cnt` samples, one behind the other
        for (int a = 1; a < 5; ++a) s[a] = s[a - 1] + cnt * B * width[a - 1];
        RHIP_TRY(launch_mh_rec_unpack(on.dims, view(), c_.fetched + done, cnt, out[0] ? s[0] : nullptr, out[1] ? s[1] : nullptr,
                                      out[2] ? s[2] : nullptr, out[3] ? s[3] : nullptr, beta ? s[4] : nullptr, diag ? s[4] : nullptr, on.stream));
        for (int a = 0; a < 5; ++a)
            if (out[a])
                RHIP_TRY(hipMemcpyAsync(out[a] + done * B * width[a], s[a], sizeof(double) * (size_t)(cnt * B * width[a]), hipMemcpyDeviceToHost, on.stream));
        RHIP_TRY(hipStreamSynchronize(on.stream));           // (the next piece reuses the staging buffer)
    }
    if (index)
        for (int64_t i = 0; i < n; ++i) index[i] = (c_.fetched + 1 + i) * c_.period;
    c_.fetched += n;
    *n_out = n;
    return MCD_OK;
}

int Recorder::end(const char* who, const RecOn& on)
{
    if (!active()) return rfail(MCD_ERR_INVALID_ARG, "%s: no recorder is active (%s_begin first)", who, api_);
    RHIP_TRY(hipSetDevice(on.device));
    RHIP_TRY(hipStreamSynchronize(on.stream));
    release();
    return MCD_OK;
}

int Recorder::window(const char* who, const RecOn& on, int64_t skip, int64_t n_samples, int32_t max_lag, SumSrc* S, int64_t* n_used) const
{
    if (!active()) return rfail(MCD_ERR_INVALID_ARG, "%s: no recorder is active (%s_begin first)", who, api_);
    const int64_t waiting = c_.waiting();
    if (skip < 0 || skip >= waiting)
        return rfail(MCD_ERR_INVALID_ARG, "%s: skip = %lld, %lld samples are waiting", who, (long long)skip, (long long)waiting);
    const int64_t n = n_samples < 0 ? waiting - skip : n_samples;
    if (n < 1 || n > waiting - skip)
        return rfail(MCD_ERR_INVALID_ARG, "%s: the window [%lld, %lld) ends past the %lld waiting samples", who, (long long)skip, (long long)(skip + n),
                     (long long)waiting);
    const MhRecDims& D = on.dims;
    const int64_t Q = 2 * (int64_t)D.n_nodes + 9;
    if (int rc = mcd_summary_check_(who, n, D.batch, Q, max_lag)) return rc;
    // base, n, B, Q, ldq (plain traces only), ring, n_nodes, first, cap, stride, ld
    *S = SumSrc{ring_, n, D.batch, Q, 0, 1, D.n_nodes, c_.first_slot(skip), c_.cap, mh_rec_stride(D.ld), D.ld};
    *n_used = n;
    return MCD_OK;
}

}  // namespace mcd

// Test hook (tests/test_hmc_record_host.py; no device, no handle): the counts of a ring in this state -- what `n` more iterations add, the
// free slots, the waiting samples, the slot of waiting sample `skip`.
extern "C" int mcd_record_ring_selftest_(int32_t period, int64_t cap, int64_t iter, int64_t fetched, int64_t n, int64_t skip, int64_t out[4])
{
    if (period < 1 || cap < 1 || !out) return rfail(MCD_ERR_INVALID_ARG, "mcd_record_ring_selftest_: need period >= 1, cap >= 1, out");
    const mcd::RecCounts c{cap, period, iter, fetched};
    out[0] = c.adds(n);
    out[1] = c.free_slots();
    out[2] = c.waiting();
    out[3] = c.first_slot(skip);
    return MCD_OK;
}
