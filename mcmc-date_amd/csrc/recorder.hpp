// recorder.hpp -- host side of the sample recorder that the Metropolis-Hastings and the NUTS driver share (mcd_mh_record_*, mcd_hmc_record_*;
// recorder.cpp).  The device side is the mcd::MhRec ring (mvn_kernels.h): each driver's kernels fill it, launch_mh_rec_unpack and k_summary.hip
// read it.  A handle holds one Recorder; an entry point is its NULL check plus one call here, with its own name `who` in front of every message.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mvn_kernels.h"
#include "summary_device.hpp"

namespace mcd {

// The ring's counts, plain numbers: `iter` iterations (transitions) since begin, so iter / period samples were taken -- sample number k
// (1, 2, ...) lies in slot (k - 1) % cap -- and `fetched` of them were handed out.
struct RecCounts {
    int64_t cap = 0;
    int32_t period = 0;
    int64_t iter = 0, fetched = 0;
    int64_t taken() const { return iter / period; }
    int64_t waiting() const { return taken() - fetched; }
    int64_t adds(int64_t n) const { return (iter + n) / period - taken(); }       // samples that n more iterations take
    int64_t free_slots() const { return cap - waiting(); }
    int64_t first_slot(int64_t skip) const { return (fetched + skip) % cap; }     // slot of waiting sample number `skip`
};

// where a driver's recorder lives and what the ring's readers need of the driver
struct RecOn { int device; hipStream_t stream; MhRecDims dims; };

class Recorder {
public:
    explicit Recorder(const char* api) : api_(api) {}      // "mcd_mh_record" / "mcd_hmc_record": the sibling calls that the messages name
    Recorder(const Recorder&) = delete;
    ~Recorder() { release(); }                             // (a member: runs after the owner's destructor body has made the device current)
    bool active() const { return ring_ != nullptr; }
    const RecCounts& counts() const { return c_; }
    // what a launch takes: the ring with `iter0` iterations counted before the launch (MhRec::iter0); base null while inactive
    MhRec view(int64_t iter0 = 0) const { return MhRec{ring_, iter0, c_.cap, c_.period}; }
    void advance(int64_t n) { if (ring_) c_.iter += n; }
    // a checkpoint's counts (mcd_mh_load): `iter` iterations done and every sample of them handed out, so the period phase continues; the
    // caller has checked that the period is the ring's and that no sample waits on either side
    void restore(int64_t iter, int64_t fetched) { if (ring_) { c_.iter = iter; c_.fetched = fetched; } }
    bool step() { advance(1); return ring_ && c_.iter % c_.period == 0; }      // one more iteration; true: it is to be recorded
    // tail_doubles: what a sample carries behind post, per chain -- 1 (beta) or kHmcRecDiag (the transition's diagnostics)
    int begin(const char* who, const RecOn& on, int32_t period, int64_t capacity, int tail_doubles);
    // the contract of a run: `n` more iterations must fit the free slots, or nothing is launched (inactive: always)
    int room(const char* who, int64_t n) const;
    int count(const char* who, int64_t* n_samples) const;
    // index[i] = the iteration (transition) of sample i, counted from begin; of beta / diag the one the driver does not record is null
    int fetch(const char* who, const RecOn& on, int64_t max_samples, int64_t* n_out, int64_t* index, double* scalars, double* heights, double* rates,
              double* post, double* beta, double* diag);
    int end(const char* who, const RecOn& on);
    // the waiting samples [skip, skip + n_samples) (n_samples < 0: all after skip) as the checked source of a summary; launches nothing
    int window(const char* who, const RecOn& on, int64_t skip, int64_t n_samples, int32_t max_lag, SumSrc* S, int64_t* n) const;

private:
    void release();
    const char* const api_;
    double *ring_ = nullptr, *stage_ = nullptr;            // the fetch unpacks into stage_: stage_cap_ samples of the five output arrays
    int64_t stage_cap_ = 0;
    int tail_ = 0;
    RecCounts c_;
};

}  // namespace mcd
