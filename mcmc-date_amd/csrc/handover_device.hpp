// handover_device.hpp -- what the Metropolis-Hastings driver (mh_capi.cpp) and the leapfrog / NUTS driver (hmc_capi.cpp) need of each other
// to hand the chains over ON THE DEVICE (mcd_hmc_take_state, mcd_mh_take_state) and to run the Hamiltonian proposal inside mcd_mh_run
// (mcd_mh_attach_hamiltonian): the kernels of k_handover.hip and the few internal calls each side offers the other.  The handles' structs
// stay private to their files.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "mvn_kernels.h"

struct mcd_mh;
struct mcd_hmc;

namespace mcd {

// the state arrays of a driver handle: scalars [5][batch] (birth, death, tH, rMu, rVar), heights / rates [batch][ld]
struct ChainArrays {
    double *sc, *H, *R;
    int64_t ld;
};

// a handle as the other driver sees it: where its chains live and what a hand-over must agree on
struct ChainsView {
    int device;
    hipStream_t stream;
    int n_nodes;
    int64_t batch;
    const int32_t* host_parent;   // [n_nodes], the likelihood handle's host copy of the topology
    bool have_state;
    ChainArrays a;
};

// per-chain sums of the attached transitions' diagnostics (mcd_mh_hamiltonian_stats), all [batch] on the device
struct HamSums {
    double* alpha;
    int64_t *depth, *leaves, *diverged;
};

// dst := src for `batch` chains of n_nodes nodes in ONE launch: the scalars as they lie, the first n_nodes entries of every row of H and
// R (the two handles may have different ld; what lies behind n_nodes in a row of dst is not written)
hipError_t launch_handover(const ChainArrays& dst, const ChainArrays& src, int64_t batch, int n_nodes, hipStream_t st);
// sums += the diagnostics of the transition N holds: alpha / max(n_alpha, 1) (the division mcd_hmc_nuts does), depth, leapfrog steps, diverged
hipError_t launch_ham_stats(const NutsDev& N, const HamSums& S, int64_t batch, hipStream_t st);

// May the chains of `src` become those of `dst`?  false, with the mismatch named in `why`: different device, number of nodes, topology,
// batch, no state on the source.
inline bool handover_allowed(const ChainsView& dst, const ChainsView& src, char* why, size_t len)
{
    if (dst.device != src.device) {
        snprintf(why, len, "the handles live on different GPUs (device %d and device %d)", dst.device, src.device);
        return false;
    }
    if (dst.n_nodes != src.n_nodes) {
        snprintf(why, len, "the handles' trees have different numbers of nodes (%d and %d)", dst.n_nodes, src.n_nodes);
        return false;
    }
    for (int v = 0; v < dst.n_nodes; ++v)
        if (dst.host_parent[v] != src.host_parent[v]) {
            snprintf(why, len, "the handles' trees have different topologies (the parent of node %d is %d and %d)", v, (int)dst.host_parent[v],
                     (int)src.host_parent[v]);
            return false;
        }
    if (dst.batch != src.batch) {
        snprintf(why, len, "the handles hold different numbers of chains (%lld and %lld)", (long long)dst.batch, (long long)src.batch);
        return false;
    }
    if (!src.have_state) {
        snprintf(why, len, "the source handle has no state yet (set_state or take_state first)");
        return false;
    }
    return true;
}

}  // namespace mcd

// ---- what each driver's file offers the other (no host wait in any of them unless said) ----------------------------------------------
// the handle as the other side sees it; mark != null: an event recorded on the handle's stream behind everything enqueued so far
int mcd_mh_chains_(const mcd_mh* m, mcd::ChainsView* v, hipEvent_t* mark);    // mh_capi.cpp
int mcd_hmc_chains_(const mcd_hmc* h, mcd::ChainsView* v, hipEvent_t* mark);  // hmc_capi.cpp
// Before a run with an attachment launches anything: may `h` make the attached transitions?  dense: the attachment names h's dense metric
// (inv_mass == NULL).  Allocates h's NUTS workspace.  MCD_ERR_INVALID_ARG with `who` in front of the message otherwise.
int mcd_hmc_cycle_ready_(mcd_hmc* h, const char* who, bool dense);
// One attached transition: h := the chains at `src` once `ready` has passed (h's stream waits, not the host), one NUTS transition with the
// step sizes d_eps [batch] and inverse masses d_inv_mass [dim] (null: h's dense metric) that lie on the device, its diagnostics added
// to `sums`; *done: an event on h's stream behind all of it.  The host waits where mcd_hmc_nuts waits: once per round of the transition.
int mcd_hmc_cycle_transition_(mcd_hmc* h, const mcd::ChainArrays& src, hipEvent_t ready, const double* d_eps, const double* d_inv_mass, int max_depth,
                              uint64_t seed, int64_t chain0, uint64_t transition, const mcd::HamSums& sums, hipEvent_t* done);
