// ckpt_device.hpp -- what the checkpoint calls (ckpt_capi.cpp: mcd_mh_save, mcd_mh_load) need of the device and of the Metropolis-Hastings
// handle: the job record of the three kernels of k_checkpoint.hip and the few internal calls mh_capi.cpp offers.  The handle's struct stays
// private to its file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ckpt_format.hpp"
#include "mvn_kernels.h"

struct mcd_mh;

namespace mcd {

// how one section's 8-byte words lie in the handle's arrays
enum { CKPT_WORDS = 0,   // n_words contiguous words
       CKPT_ROWS,        // rows of row_len doubles with the leading dimension ld (heights, rates: the pad of a row is neither read nor written)
       CKPT_INT32 };     // row_len int32 values, two per word; an odd count leaves the last word's upper half 0
struct CkptSec {
    void* arr;             // the handle's array (null: the section is only summed, as every section is by k_ckpt_verify)
    uint64_t n_words;      // the section's length in the blob
    uint64_t blob_word;    // its first word in the blob
    int64_t row_len, ld;
    int kind;
    unsigned first_block;  // the launch's workgroups [first_block, first_block of the next section) take this section, kCkptSlab words each
};
constexpr int kCkptSlab = 2048;   // words per workgroup: 256 lanes x 8, consecutive lanes on consecutive words
struct CkptJob {
    uint64_t* blob;               // the staging blob (device)
    unsigned long long* sums;     // section s adds its checksum to sums[s * sum_stride] (zeroed before the launch)
    int sum_stride;
    int n;
    CkptSec s[kCkptMaxSections];
};

// first_block of every section from n_words; the grid in *blocks.  false: more than 2^31 - 1 workgroups
bool ckpt_plan(CkptJob* J, unsigned* blocks);
// blob := the arrays, and every section's checksum (k_ckpt_pack); the checksums of the blob's sections alone (k_ckpt_verify); the arrays :=
// blob (k_ckpt_unpack; sums unused).  One launch each on `st`.
hipError_t launch_ckpt_pack(const CkptJob& J, unsigned blocks, hipStream_t st);
hipError_t launch_ckpt_verify(const CkptJob& J, unsigned blocks, hipStream_t st);
hipError_t launch_ckpt_unpack(const CkptJob& J, unsigned blocks, hipStream_t st);

// a Metropolis-Hastings handle between two runs, as the checkpoint sees it (pointers into the handle; valid until the next call on it)
struct CkptView {
    int device;
    hipStream_t stream;
    MhDev dev;
    bool dense, have_state;
    int dim;                            // the likelihood's dimension
    uint64_t seed, step;
    int64_t n_samples;
    const int32_t* host_parent;         // [n_nodes]
    const MhRow* rows;                  // [n_prop] the proposal table (host)
    const int32_t* dims;                // [n_prop] its dimension column
    bool rec_active;
    int32_t rec_period;
    int64_t rec_iter, rec_fetched;
    Mc3Dev mc3;                         // n_chains 0: not initialised
    const double* mc3_ladder;           // [n_chains] host copy
    uint64_t mc3_seed, mc3_phase;
    bool ham;                           // an attachment
    int ham_depth, ham_dim;
    uint64_t ham_seed, ham_next;
    int64_t ham_counted;
    double *ham_eps, *ham_inv_mass;     // device; inv_mass null: the attached handle's dense metric
    void* ham_sums;                     // [4][batch] words
};

// what a load sets on the host side of the handle once the arrays are written
struct CkptCommit {
    bool full;                          // false: MCD_CKPT_STATE_TUNING -- have_state alone
    uint64_t step;
    int64_t n_samples;
    int32_t lik_only;
    bool rec;                           // restore the recorder's counts
    int64_t rec_iter, rec_fetched;
    uint64_t mc3_phase;
    uint64_t ham_next;
    int64_t ham_counted;
};

}  // namespace mcd

// ---- what mh_capi.cpp offers (no launch, no host wait) --------------------------------------------------------------------------------
int mcd_mh_ckpt_view_(const mcd_mh* m, mcd::CkptView* v);
// the handle's staging blob of at least `bytes` bytes (one of the handle's allocations; grows on demand, never shrinks)
int mcd_mh_ckpt_stage_(mcd_mh* m, size_t bytes, void** p);
int mcd_mh_ckpt_commit_(mcd_mh* m, const mcd::CkptCommit& c);
