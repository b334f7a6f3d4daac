// mh_capi.cpp -- C ABI of the lock-step Metropolis-Hastings-Green driver (include/mcmcdate_mvn.h, "mcd_mh_*").
// mcd_mh_run plans every run once (plan_run: one of the nine MCD_MH_PATH_* launch structures and every choice its launches depend on),
// then one runner enqueues its launches on the handle's stream: a whole-schedule kernel (k_mh_chain.hip, k_mh_chain_big.hip), the segment
// loop (k_mh_segment*.hip) or the two-launch step loop (k_mh.hip + a likelihood launch).  The state stays on the device.  No CPU path.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <algorithm>
#include <vector>

#include "../../include/mcmcdate_mvn.h"
#include "ckpt_device.hpp"
#include "handover_device.hpp"
#include "mvn_kernels.h"
#include "nuts_rhs_plan.hpp"
#include "options.h"
#include "recorder.hpp"
#include "summary_device.hpp"
#include "marginal_device.hpp"

int mcd_summary_run_(const mcd::SumSrc& S, int32_t max_lag, hipStream_t st, double* pooled, double* per_chain);   // summary_capi.cpp
int mcd_summary_check_(const char* who, int64_t n, int64_t batch, int64_t q, int32_t max_lag);
int mcd_marginal_check_(const char* who, int64_t n, int64_t batch, int64_t chain0, int n_points, const double* betas);   // marginal_capi.cpp
int mcd_marginal_run_(const char* who, const mcd::MlSrc& S, const double* betas, hipStream_t st, double* point, double* replicate, double* out);
extern "C" int mcd_set_last_error_(int code, const char* msg);   // mvn_capi.cpp
struct mcd_sparse;
struct mcd_sparse_tree;
int mcd_sparse_tree_internal_(const mcd_sparse_tree* t, const mcd_sparse** sp, const mcd::SparseDev** dev, const mcd::SparseTreeDev** tree, int* device,
                              const int32_t** host_parent);   // sparse_capi.cpp
int mcd_sparse_scratch_(const mcd_sparse* h, hipStream_t st, int64_t batch, double** out);

namespace {

int mfail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mcd_set_last_error_(code, buf);
}

#define MHIP_TRY(expr)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return mfail(MCD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

}  // namespace

struct mcd_mh {
    int device = 0;
    const mcd::MvnDev* mvn = nullptr;
    const mcd::TreeDev* tree = nullptr;
    const mcd::PriorDev* prior = nullptr;
    // a likelihood over a SPARSE precision matrix instead (mcd_mh_create_sparse): mvn stays null, tree points at tree_shim (the slot
    // tables the step kernel needs for the distances)
    const mcd_sparse* sp_handle = nullptr;
    const mcd::SparseDev* sp = nullptr;
    const mcd::SparseTreeDev* sp_tree = nullptr;
    mcd::TreeDev tree_shim{};
    mcd::MhDev dev{};
    uint64_t seed = 0, step = 0;
    int64_t n_samples = 0;
    bool have_state = false;
    bool chain_kernel = false;   // n_nodes <= 64: whole schedule in one launch
    double* d_X1 = nullptr;         // [batch][n]: distances of the proposed states (large trees: written by k_mh_step_wg)
    double* d_inc_ll = nullptr;     // [batch] ln likelihood output of the refreshing full products (not used)
    mcd::MhInc inc{};               // incremental likelihood of that path (k_mh_inc.hip): X0, zcur, zprop allocated on first use
    std::vector<mcd::MhRow> rows;   // host copy of the proposal table
    std::vector<int32_t> dims;      // ... and of its dimension column (the checkpoint's fingerprint, ckpt_capi.cpp)
    double* d_psum = nullptr;           // k_mh_step_wg's kept summands of the ln prior (MhDev::psum, psel)
    int32_t* d_psel = nullptr;
    std::vector<int32_t> sparse_rows;   // per row: 1 = moves at most kMhIncSlots distances (the two-launch path's incremental evaluation)
    const double* d_Fp = nullptr;
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    int32_t* d_sched = nullptr;
    size_t sched_cap = 0;
    double* d_trace_alpha = nullptr;
    int8_t* d_trace_accept = nullptr;
    size_t trace_cap = 0;
    int last_path = MCD_MH_PATH_NONE;   // which launch structure the last mcd_mh_run took
    unsigned long long last_lds = 0;    // LDS bytes per workgroup of the persistent kernel that run launched last (0: none)
    bool list_all = false;              // sparse likelihood on a tree whose distance slots all fit the segment kernel's list
    // Metropolis-coupled MCMC (mcd_mh_mc3_*): temperature ranks of all GLOBAL chains, ladder, counters; phase = swap phases done
    mcd::Mc3Dev mc3{};
    uint64_t mc3_seed = 0, mc3_phase = 0;
    std::vector<double> mc3_ladder;           // host copy of the ladder (what a checkpoint's MC3 must agree with)
    void* d_ckpt = nullptr;                   // the checkpoint's staging blob (mcd_mh_save / mcd_mh_load), one of `allocs`
    size_t ckpt_cap = 0;
    mcd::Recorder rec{"mcd_mh_record"};       // the sample recorder (mcd_mh_record_*, recorder.cpp): it counts iterations
    const int32_t* host_parent = nullptr;     // [n_nodes] the likelihood handle's host copy of the topology (hand-overs compare it)
    mutable hipEvent_t mark = nullptr;        // what another handle's stream waits for (mcd_mh_chains_), created on first use
    // the Hamiltonian proposal attached to this handle (mcd_mh_attach_hamiltonian): h null = none.  The step sizes, the inverse masses
    // (null: h's dense metric) and the sums of the transitions' diagnostics live on the device and belong to the attachment.
    struct Hamiltonian {
        mcd_hmc* h = nullptr;
        double *d_eps = nullptr, *d_inv_mass = nullptr;
        int max_depth = 0;
        uint64_t seed = 0, first = 0, done = 0;   // the next transition's number is first + done
        int64_t counted = 0;                      // transitions in the sums
        void* d_sums = nullptr;                   // one block behind `sums`
        mcd::HamSums sums{};
        void release()
        {
            for (void* p : {(void*)d_eps, (void*)d_inv_mass, d_sums})
                if (p) (void)hipFree(p);
            *this = Hamiltonian{};
        }
    } ham;
    mcd::RecOn rec_on() const { return {device, stream, mcd::MhRecDims{dev.batch, dev.ld, dev.n_nodes}}; }

    ~mcd_mh()
    {
        (void)hipSetDevice(device);
        ham.release();
        if (mark) (void)hipEventDestroy(mark);
        for (void* p : allocs) (void)hipFree(p);
        if (d_sched) (void)hipFree(d_sched);
        if (d_trace_alpha) (void)hipFree(d_trace_alpha);
        if (d_trace_accept) (void)hipFree(d_trace_accept);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// why a tempered target and an attached Hamiltonian proposal exclude each other, whichever comes second
const char* const kHamTempered = "a Hamiltonian proposal is attached to this handle (mcd_mh_attach_hamiltonian) and its target is prior x likelihood x "
                                 "jacobianRootBranch at temperature 1: no MC3, no power posterior, no temperature other than 1";

template <class T>
int dev_alloc(mcd_mh* m, T** p, size_t count, bool zero)
{
    *p = nullptr;
    MHIP_TRY(hipMalloc((void**)p, sizeof(T) * (count ? count : 1)));
    m->allocs.push_back(*p);
    if (zero) MHIP_TRY(hipMemset(*p, 0, sizeof(T) * (count ? count : 1)));
    return MCD_OK;
}

template <class T>
int dev_upload(mcd_mh* m, const T** p, const T* src, size_t count)
{
    T* d = nullptr;
    if (int rc = dev_alloc(m, &d, count, false)) return rc;
    if (count) MHIP_TRY(hipMemcpy(d, src, sizeof(T) * count, hipMemcpyHostToDevice));
    *p = d;
    return MCD_OK;
}

// ln prior, ln likelihood and ln jacobianRootBranch of a state batch -> post[3][batch]
int eval_posterior(mcd_mh* m, const double* sc, const double* H, const double* R, double* post)
{
    const mcd::MhDev& D = m->dev;
    const int64_t B = D.batch;
    MHIP_TRY(mcd::launch_prior(*m->prior, sc + 0 * B, sc + 1 * B, sc + 2 * B, H, sc + 3 * B, sc + 4 * B, R, D.ld, B, post, D.pcomp,
                               m->stream));
    if (m->sp) {
        double* scr = nullptr;
        if (int rc = mcd_sparse_scratch_(m->sp_handle, m->stream, B, &scr)) return rc;
        MHIP_TRY(mcd::launch_sparse_tree_logpdf(*m->sp, *m->sp_tree, H, R, D.ld, sc + 2 * B, sc + 3 * B, B, post + B, post + 2 * B, scr, m->stream));
        return MCD_OK;
    }
    MHIP_TRY(mcd::launch_tree_logpdf(*m->mvn, *m->tree, H, R, D.ld, sc + 2 * B, sc + 3 * B, B, post + B, post + 2 * B, m->stream));
    return MCD_OK;
}

}  // namespace

namespace {

// host copies of the topology that the proposal table is checked and classified against
struct HostTree {
    int n;
    const int32_t* parent;
    std::vector<int32_t> size;                     // nodes of every sub tree
    std::vector<int32_t> brace_ptr, brace_nodes;   // the prior's braces (their tables live in device memory)
};

// the proposal table checks: the reference raises `error` for a path to a leaf / an invalid path when the proposal is built
int check_proposals(const HostTree& t, int n_prop, const int32_t* kind, const int32_t* node, const int32_t* dim, const double* p0, const double* p1)
{
    const int n = t.n, n_brace = (int)t.brace_ptr.size() - 1;
    const std::vector<int32_t>& size = t.size;
    const int root_right = 1 + size[1];
    for (int i = 0; i < n_prop; ++i) {
        const int k = kind[i], v = node[i];
        if (!(p0[i] > 0) || !std::isfinite(p0[i])) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: proposal %d: p0 must be positive", i);
        if (dim[i] < 1) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: proposal %d: dimension must be >= 1", i);
        switch (k) {
            case MCD_PROP_SCALE_SCALAR:
                if (v < 0 || v > 4) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: proposal %d: scalar index %d", i, v);
                break;
            case MCD_PROP_SCALE_NORM_TREE:
                if (v != 2 && v != 3) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: proposal %d: norm must be tH (2) or rMu (3)", i);
                break;
            case MCD_PROP_SLIDE_NODE:
            case MCD_PROP_SCALE_SUBTREE_TIME:
                if (v < 1 || v >= n) return mfail(MCD_ERR_INVALID_ARG, "slideNodeAtUltrametric: Path is invalid (proposal %d, node %d).", i, v);
                if (size[v] == 1) return mfail(MCD_ERR_INVALID_ARG, "slideNodeAtUltrametric: Path leads to a leaf (proposal %d, node %d).", i, v);
                break;
            case MCD_PROP_PULLEY:
                if (size[1] == 1) return mfail(MCD_ERR_INVALID_ARG, "pulleyUltrametric: Left sub tree is a leaf.");
                if (size[root_right] == 1) return mfail(MCD_ERR_INVALID_ARG, "pulleyUltrametric: Right sub tree is a leaf.");
                break;
            case MCD_PROP_SCALE_BRANCH_RATE:
            case MCD_PROP_SCALE_SUBTREE_RATE:
                if (v < 1 || v >= n) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: proposal %d: node %d out of range", i, v);
                break;
            case MCD_PROP_SLIDE_NODE_CONTRA:
            case MCD_PROP_SCALE_SUBTREE_CONTRA:
                if (v < 1 || v >= n) return mfail(MCD_ERR_INVALID_ARG, "slideNodesAtContrarily: Path is invalid (proposal %d, node %d).", i, v);
                if (size[v] == 1) return mfail(MCD_ERR_INVALID_ARG, "slideNodesAtContrarily: Path leads to a leaf (proposal %d, node %d).", i, v);
                break;
            case MCD_PROP_SLIDE_BRACE:
            case MCD_PROP_SLIDE_BRACE_CONTRA:
                if (v < 0 || v >= n_brace) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: proposal %d: the prior has no brace %d", i, v);
                for (int j = t.brace_ptr[v]; j < t.brace_ptr[v + 1]; ++j) {
                    const int x = t.brace_nodes[j];
                    if (x == 0) return mfail(MCD_ERR_INVALID_ARG, "slideBracedNodesUltrametric: Braced root node (proposal %d).", i);
                    if (size[x] == 1) return mfail(MCD_ERR_INVALID_ARG, "slideBracedNodesUltrametric: Path of a node leads to a leaf (proposal %d).", i);
                }
                break;
            case MCD_PROP_SLIDE_ROOT_CONTRA:
            case MCD_PROP_SCALE_RATES_TREE_CONTRA:
            case MCD_PROP_SCALE_VAR_TREE:
            case MCD_PROP_SCALE_VAR_TREE_AUTO: break;
            case MCD_PROP_SCALE_CONTRARILY:
                if (!(p1[i] > 0)) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: proposal %d: p1 must be positive", i);
                break;
            default: return mfail(MCD_ERR_UNSUPPORTED, "mcd_mh_create: proposal %d: unknown kind %d", i, k);
        }
    }
    return MCD_OK;
}

// Per proposal: 1 where it moves at most `limit` branch distances, or everywhere (all).  A distance changes where a node's height, its
// parent's height or its rate changes -- for the node kinds below the node itself with its daughters, or its sub tree.  The root's two
// daughters share distance slot 0.  This is a performance hint only: the kernels find the moved distances from the data and are right for
// any number of them.
std::vector<int32_t> moves_few(const HostTree& t, int limit, bool all, int n_prop, const int32_t* kind, const int32_t* node)
{
    std::vector<std::vector<int>> kids((size_t)t.n);
    for (int v = 1; v < t.n; ++v) kids[(size_t)t.parent[v]].push_back(v);
    auto slots_of = [&](const std::vector<int>& nodes) {
        std::vector<int> sl;
        for (int w : nodes) {
            if (w == 0) continue;
            const int key = (t.parent[w] == 0) ? 1 : w;              // both root daughters -> one slot
            if (std::find(sl.begin(), sl.end(), key) == sl.end()) sl.push_back(key);
        }
        return (int)sl.size();
    };
    std::vector<int32_t> out((size_t)n_prop, 0);
    for (int i = 0; i < n_prop; ++i) {
        const int k = kind[i], v = node[i];
        std::vector<int> touched;
        bool known = true;
        switch (k) {
            case MCD_PROP_SLIDE_NODE:
            case MCD_PROP_SLIDE_NODE_CONTRA:
                touched.push_back(v);
                for (int c : kids[(size_t)v]) touched.push_back(c);
                break;
            case MCD_PROP_SCALE_BRANCH_RATE: touched.push_back(v); break;
            case MCD_PROP_SCALE_SUBTREE_TIME:
            case MCD_PROP_SCALE_SUBTREE_RATE:
            case MCD_PROP_SCALE_SUBTREE_CONTRA:
                if (t.size[v] > 2 * limit) { known = false; break; }
                for (int w = v; w < v + t.size[v]; ++w) touched.push_back(w);
                break;
            case MCD_PROP_SLIDE_BRACE:
            case MCD_PROP_SLIDE_BRACE_CONTRA:
                for (int j = t.brace_ptr[v]; j < t.brace_ptr[v + 1]; ++j) {
                    touched.push_back(t.brace_nodes[j]);
                    for (int c : kids[(size_t)t.brace_nodes[j]]) touched.push_back(c);
                }
                break;
            default: known = false; break;                         // scalars, whole-tree scalings, pulley, root slide
        }
        out[(size_t)i] = ((known && slots_of(touched) <= limit) || all) ? 1 : 0;
    }
    return out;
}

// the part of mcd_mh_create / mcd_mh_create_sparse behind the handles: m->mvn / m->tree (dense) or m->sp / m->sp_tree / m->tree
// (= &m->tree_shim, sparse) and m->prior are set, `parent` is the host copy of the topology, host_L the host factor (dense) or null
int mh_create_impl(mcd_mh_t** out, std::unique_ptr<mcd_mh>& m, const mcd_prior_t* prior, int dev_t, int dev_p, const int32_t* parent, const double* host_L,
                   int n_prop, const int32_t* kind, const int32_t* node, const int32_t* n1, const int32_t* n2, const int32_t* jac_root,
                   const int32_t* dim, const double* p0, const double* p1, int64_t batch, uint64_t seed)
{
    // the knobs (mcd_set_option) that creation reads; every run reads the others when it starts (plan_run)
    const int opt_inc_slots = mcd::opt_get(mcd::OPT_MH_INC_SLOTS), opt_sparse_slots = mcd::opt_get(mcd::OPT_MH_SPARSE_SLOTS);
    const bool per_phase = mcd::opt_is(mcd::OPT_MH_PER_PHASE, 1);
    if (dev_t != dev_p) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: tree (device %d) and prior (device %d) live on different GPUs", dev_t, dev_p);
    const int n = m->tree->n_nodes;
    if (m->prior->n_nodes != n) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: tree has %d nodes, prior %d", n, m->prior->n_nodes);
    {   // tree and prior must describe the same topology: compare the prior's parent array (device) with the tree's
        std::vector<int32_t> pp(n);
        MHIP_TRY(hipSetDevice(dev_p));
        MHIP_TRY(hipMemcpy(pp.data(), m->prior->parent, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        for (int v = 0; v < n; ++v)
            if (pp[v] != parent[v]) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: tree and prior have different topologies (node %d)", v);
    }
    HostTree t{n, parent, std::vector<int32_t>(n, 1), {}, {}};
    for (int v = n - 1; v > 0; --v) t.size[parent[v]] += t.size[v];
    const int nbr = m->prior->n_brace;
    t.brace_ptr.assign(nbr + 1, 0);
    if (nbr > 0) {
        int dev_prior = 0;
        const mcd::PriorDev* pd = nullptr;
        (void)mcd_prior_internal_(prior, &pd, &dev_prior);
        MHIP_TRY(hipSetDevice(dev_prior));
        MHIP_TRY(hipMemcpy(t.brace_ptr.data(), pd->brace_ptr, sizeof(int32_t) * (nbr + 1), hipMemcpyDeviceToHost));
        t.brace_nodes.resize(t.brace_ptr[nbr]);
        MHIP_TRY(hipMemcpy(t.brace_nodes.data(), pd->brace_nodes, sizeof(int32_t) * t.brace_nodes.size(), hipMemcpyDeviceToHost));
    }
    if (int rc = check_proposals(t, n_prop, kind, node, dim, p0, p1)) return rc;
    // Which proposals move only a few branch distances: the streaming chain kernel (k_mh_chain_big.hip) evaluates those by columns of L^-1
    // instead of a sweep -- up to 258 nodes its likelihood wave takes the columns four at a time beside the prior: kMhSparseSlots, tuning:
    // MCD_MH_SPARSE_SLOTS, at most 64 (its list, kMhbList).  The two-launch path's incremental evaluation (k_mh_inc.hip) is not bounded by
    // registers: up to kMhIncSlots columns of L^-1 still cost less than a likelihood launch.  Where the segment kernel runs the sparse
    // proposals (k_mh_segment.hip), many more: a likelihood launch there also costs the whole state's way through memory twice; measured at
    // 1025 nodes x 512 chains: 16 -> 22.5, 64 -> 14.2, 128 -> 12.7, 192 -> 12.5 us per lock step.  Over a sparse precision matrix
    // (k_mh_segment_sparse.hip) a listed distance costs a row of the matrix, some 15 entries, where the two launches of a dense proposal
    // cost a full product -- whatever the list holds.  MCD_MH_INC_SLOTS sets the latter three.
    const bool seg_capable = m->mvn != nullptr && mcd::mh_segment_available(*m->mvn, n, batch);
    const bool sseg_capable = m->sp != nullptr && mcd::mh_segment_sparse_available(*m->sp, n, batch);
    const int list_cap = sseg_capable ? mcd::mh_segment_sparse_list() : mcd::kMhSegList;
    const int inc_slots = opt_inc_slots != mcd::MCD_OPT_UNSET ? std::max(1, std::min(list_cap, opt_inc_slots)) : sseg_capable ? list_cap : seg_capable ? mcd::kMhSegSlots : mcd::kMhIncSlots;
    // a tree whose distance slots ALL fit the sparse segment kernel's list: every proposal of the cycle can run inside a segment
    m->list_all = sseg_capable && m->sp->n <= list_cap;
    const int chain_slots = opt_sparse_slots != mcd::MCD_OPT_UNSET ? std::max(1, std::min(64, opt_sparse_slots)) : mcd::kMhSparseSlots;
    const std::vector<int32_t> sparse = moves_few(t, chain_slots, false, n_prop, kind, node);
    m->sparse_rows = moves_few(t, inc_slots, m->list_all, n_prop, kind, node);
    m->device = dev_t;
    m->seed = seed;
    m->host_parent = parent;
    for (int i = 0; i < n_prop; ++i) m->rows.push_back(mcd::MhRow{kind[i], node[i], n1[i], n2[i], jac_root[i], p0[i], p1[i]});
    m->dims.assign(dim, dim + n_prop);
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    mcd::MhDev& D = m->dev;
    D.n_nodes = n;
    D.n_prop = n_prop;
    D.batch = batch;
    D.ld = (n + 7) / 8 * 8;
    D.chain0 = 0;
    D.parent = m->mvn ? m->tree->parent : m->prior->parent;
    D.brace_ptr = m->prior->brace_ptr;
    D.brace_nodes = m->prior->brace_nodes;
    D.n_brace = nbr;
    int rc = MCD_OK;
    const size_t B = (size_t)batch, BL = B * (size_t)D.ld, BP = B * (size_t)n_prop, BN = B * (size_t)n;
    if ((rc = dev_upload(m.get(), &D.size, t.size.data(), (size_t)n)) || (rc = dev_upload(m.get(), &D.kind, kind, (size_t)n_prop)) ||
        (rc = dev_upload(m.get(), &D.node, node, (size_t)n_prop)) || (rc = dev_upload(m.get(), &D.n1, n1, (size_t)n_prop)) ||
        (rc = dev_upload(m.get(), &D.n2, n2, (size_t)n_prop)) || (rc = dev_upload(m.get(), &D.jac_root, jac_root, (size_t)n_prop)) ||
        (rc = dev_upload(m.get(), &D.dim, dim, (size_t)n_prop)) || (rc = dev_upload(m.get(), &D.p0, p0, (size_t)n_prop)) ||
        (rc = dev_upload(m.get(), &D.p1, p1, (size_t)n_prop)) || (rc = dev_alloc(m.get(), &D.sc, 5 * B, true)) ||
        (rc = dev_alloc(m.get(), &D.H, BL, true)) || (rc = dev_alloc(m.get(), &D.R, BL, true)) ||
        (rc = dev_alloc(m.get(), &D.sc1, 5 * B, true)) || (rc = dev_alloc(m.get(), &D.H1, BL, true)) ||
        (rc = dev_alloc(m.get(), &D.R1, BL, true)) || (rc = dev_alloc(m.get(), &D.post, 3 * B, true)) ||
        (rc = dev_alloc(m.get(), &D.post1, 3 * B, true)) || (rc = dev_alloc(m.get(), &D.lnqj, B, true)) || (rc = dev_alloc(m.get(), &D.beta, B, false)) ||
        (rc = dev_alloc(m.get(), &D.tune, BP, false)) || (rc = dev_alloc(m.get(), &D.acc, BP, true)) ||
        (rc = dev_alloc(m.get(), &D.tried, BP, true)) || (rc = dev_alloc(m.get(), &D.age_sum, BN, true)) ||
        (rc = dev_alloc(m.get(), &D.age_sq, BN, true)) || (rc = dev_alloc(m.get(), &D.pcomp, 3 * B, true)) ||
        (rc = dev_alloc(m.get(), &D.pcomp1, 3 * B, true)) || (rc = dev_alloc(m.get(), &D.draws, 64 * 5 * B, true)) ||
        (rc = dev_alloc(m.get(), &D.pflags, B, true)) || (rc = dev_upload(m.get(), &D.sparse, sparse.data(), (size_t)n_prop)))
        return rc;
    // trees of at most 64 nodes: the whole schedule runs in one launch with the factor staged in LDS (k_mh_chain.hip).
    // MCD_MH_PER_PHASE=1 (diagnostic) keeps the two-launches-per-step path that larger trees use.
    const int nd = m->mvn ? m->mvn->n : m->sp->n;
    if (m->mvn && n <= 64 && !per_phase && mcd::mh_chain_lds_bytes(nd, n_prop, 4) + sizeof(double) * mcd::prior_node_tables_doubles(m->prior->n_cal, m->prior->n_con) <= 64 * 1024) {
        std::vector<double> Fp((size_t)nd * 64, 0.0);
        for (int i = 0; i < nd; ++i) {
            const double inv = 1.0 / host_L[(size_t)i * nd + i];
            for (int j = 0; j < i; ++j) Fp[(size_t)j * 64 + i] = host_L[(size_t)i * nd + j] * inv;
        }
        if ((rc = dev_upload(m.get(), &m->d_Fp, Fp.data(), Fp.size()))) return rc;
        m->chain_kernel = true;
    }
    {
        std::vector<double> ones(BP > B ? BP : B, 1.0);
        MHIP_TRY(hipMemcpy(D.tune, ones.data(), sizeof(double) * BP, hipMemcpyHostToDevice));
        MHIP_TRY(hipMemcpy(D.beta, ones.data(), sizeof(double) * B, hipMemcpyHostToDevice));
    }
    *out = m.release();
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_mh_create(mcd_mh_t** out, const mcd_tree_t* tree, const mcd_prior_t* prior, int n_prop, const int32_t* kind,
                  const int32_t* node, const int32_t* n1, const int32_t* n2, const int32_t* jac_root, const int32_t* dim,
                  const double* p0, const double* p1, int64_t batch, uint64_t seed)
{
    if (!out) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: out is NULL");
    *out = nullptr;
    if (!tree || !prior) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: NULL tree or prior handle");
    if (n_prop <= 0 || !kind || !node || !n1 || !n2 || !jac_root || !dim || !p0 || !p1)
        return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: empty or NULL proposal table");
    if (batch <= 0 || batch > (int64_t)1 << 31) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: batch must be in [1, 2^31]");
    std::unique_ptr<mcd_mh> m(new mcd_mh());
    int dev_t = 0, dev_p = 0;
    const int32_t* parent = nullptr;
    const double* host_L = nullptr;
    if (mcd_tree_internal_(tree, &m->mvn, &m->tree, &dev_t, &parent, &host_L) || mcd_prior_internal_(prior, &m->prior, &dev_p))
        return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create: invalid handle");
    return mh_create_impl(out, m, prior, dev_t, dev_p, parent, host_L, n_prop, kind, node, n1, n2, jac_root, dim, p0, p1, batch, seed);
}

// The same driver over a likelihood whose precision matrix stays sparse on the device (mcd_sparse_*): trees beyond the dense kernels'
// 1024 branches.  Two launches per lock step -- the workgroup-per-chain step kernel leaving the proposed distances, the sparse
// product on them (k_sparse.hip).
int mcd_mh_create_sparse(mcd_mh_t** out, const mcd_sparse_tree_t* tree, const mcd_prior_t* prior, int n_prop, const int32_t* kind,
                         const int32_t* node, const int32_t* n1, const int32_t* n2, const int32_t* jac_root, const int32_t* dim,
                         const double* p0, const double* p1, int64_t batch, uint64_t seed)
{
    if (!out) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create_sparse: out is NULL");
    *out = nullptr;
    if (!tree || !prior) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create_sparse: NULL tree or prior handle");
    if (n_prop <= 0 || !kind || !node || !n1 || !n2 || !jac_root || !dim || !p0 || !p1)
        return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create_sparse: empty or NULL proposal table");
    if (batch <= 0 || batch > (int64_t)1 << 31) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create_sparse: batch must be in [1, 2^31]");
    std::unique_ptr<mcd_mh> m(new mcd_mh());
    int dev_t = 0, dev_p = 0;
    const int32_t* parent = nullptr;
    if (mcd_sparse_tree_internal_(tree, &m->sp_handle, &m->sp, &m->sp_tree, &dev_t, &parent) || mcd_prior_internal_(prior, &m->prior, &dev_p))
        return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_create_sparse: invalid handle");
    if (m->sp_tree->n_nodes < 3 || m->sp_tree->n_nodes > 2048)
        return mfail(MCD_ERR_UNSUPPORTED, "mcd_mh_create_sparse: %d nodes (the sparse driver serves trees of 3 .. 2048 nodes)", m->sp_tree->n_nodes);
    m->tree_shim = mcd::TreeDev{m->sp_tree->n_nodes, (m->sp_tree->n_nodes + 63) / 64 * 64, m->sp_tree->root_right, m->prior->parent, m->sp_tree->slot_node,
                                m->sp_tree->slot_parent, nullptr, nullptr};
    m->tree = &m->tree_shim;
    return mh_create_impl(out, m, prior, dev_t, dev_p, parent, nullptr, n_prop, kind, node, n1, n2, jac_root, dim, p0, p1, batch, seed);
}

void mcd_mh_destroy(mcd_mh_t* m) { delete m; }

int mcd_mh_set_chain_offset(mcd_mh_t* m, int64_t first_chain)
{
    if (!m || first_chain < 0 || first_chain + m->dev.batch > ((int64_t)1 << 32))
        return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_set_chain_offset: chain indices must stay below 2^32");
    m->dev.chain0 = first_chain;
    return MCD_OK;
}

int mcd_mh_set_state(mcd_mh_t* m, const double* birth, const double* death, const double* tH, const double* heights,
                     const double* rMu, const double* rVar, const double* rates, int64_t ld_state)
{
    if (!m || !birth || !death || !tH || !heights || !rMu || !rVar || !rates) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_set_state: NULL argument");
    mcd::MhDev& D = m->dev;
    if (ld_state < D.n_nodes) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_set_state: ld_state < n_nodes");
    MHIP_TRY(hipSetDevice(m->device));
    const size_t B = (size_t)D.batch;
    const double* sc_src[5] = {birth, death, tH, rMu, rVar};
    for (int i = 0; i < 5; ++i) MHIP_TRY(hipMemcpyAsync(D.sc + i * B, sc_src[i], sizeof(double) * B, hipMemcpyHostToDevice, m->stream));
    MHIP_TRY(hipMemcpy2DAsync(D.H, sizeof(double) * D.ld, heights, sizeof(double) * ld_state, sizeof(double) * D.n_nodes, B, hipMemcpyHostToDevice, m->stream));
    MHIP_TRY(hipMemcpy2DAsync(D.R, sizeof(double) * D.ld, rates, sizeof(double) * ld_state, sizeof(double) * D.n_nodes, B, hipMemcpyHostToDevice, m->stream));
    if (int rc = eval_posterior(m, D.sc, D.H, D.R, D.post)) return rc;
    MHIP_TRY(hipStreamSynchronize(m->stream));
    m->have_state = true;
    return MCD_OK;
}

int mcd_mh_get_state(const mcd_mh_t* cm, double* birth, double* death, double* tH, double* heights, double* rMu, double* rVar,
                     double* rates, int64_t ld_state)
{
    if (!cm || !birth || !death || !tH || !heights || !rMu || !rVar || !rates) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_get_state: NULL argument");
    const mcd::MhDev& D = cm->dev;
    if (ld_state < D.n_nodes) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_get_state: ld_state < n_nodes");
    MHIP_TRY(hipSetDevice(cm->device));
    MHIP_TRY(hipStreamSynchronize(cm->stream));
    const size_t B = (size_t)D.batch;
    double* sc_dst[5] = {birth, death, tH, rMu, rVar};
    for (int i = 0; i < 5; ++i) MHIP_TRY(hipMemcpy(sc_dst[i], D.sc + i * B, sizeof(double) * B, hipMemcpyDeviceToHost));
    MHIP_TRY(hipMemcpy2D(heights, sizeof(double) * ld_state, D.H, sizeof(double) * D.ld, sizeof(double) * D.n_nodes, B, hipMemcpyDeviceToHost));
    MHIP_TRY(hipMemcpy2D(rates, sizeof(double) * ld_state, D.R, sizeof(double) * D.ld, sizeof(double) * D.n_nodes, B, hipMemcpyDeviceToHost));
    return MCD_OK;
}

int mcd_mh_get_posterior(const mcd_mh_t* cm, double* post)
{
    if (!cm || !post) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_get_posterior: NULL argument");
    const mcd::MhDev& D = cm->dev;
    MHIP_TRY(hipSetDevice(cm->device));
    MHIP_TRY(hipStreamSynchronize(cm->stream));
    const size_t B = (size_t)D.batch;
    std::vector<double> tmp(3 * B);
    MHIP_TRY(hipMemcpy(tmp.data(), D.post, sizeof(double) * 3 * B, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b)
        for (int i = 0; i < 3; ++i) post[b * 3 + i] = tmp[i * B + b];
    return MCD_OK;
}

int mcd_mh_posterior_device(const mcd_mh_t* cm, const double** post, void** stream)
{
    if (!cm || !post) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_posterior_device: NULL argument");
    *post = cm->dev.post;                      // [3][batch]: ln prior, ln likelihood, ln jacobianRootBranch of the current states
    if (stream) *stream = (void*)cm->stream;   // the stream the sampler's launches are ordered on
    return MCD_OK;
}

int mcd_mh_last_path(const mcd_mh_t* m) { return m ? m->last_path : mfail(MCD_ERR_INVALID_ARG, "mcd_mh_last_path: NULL handle"); }
int64_t mcd_mh_last_dynamic_lds(const mcd_mh_t* m) { return m ? (int64_t)m->last_lds : (int64_t)mfail(MCD_ERR_INVALID_ARG, "mcd_mh_last_dynamic_lds: NULL handle"); }

// ---- Metropolis-coupled MCMC: the swap phase (k_mc3.hip) -----------------------------------------------------------------
int mcd_mh_mc3_init(mcd_mh_t* m, int n_chains, const double* betas, int64_t total_chains, uint64_t seed)
{
    if (!m || !betas) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_init: NULL argument");
    if (m->ham.h) return mfail(MCD_ERR_UNSUPPORTED, "mcd_mh_mc3_init: %s", kHamTempered);
    const mcd::MhDev& D = m->dev;
    if (n_chains < 2 || n_chains > 16) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_init: n_chains must be 2 .. 16");
    if (total_chains <= 0 || total_chains % n_chains != 0)
        return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_init: the global number of chains must be a multiple of n_chains");
    if (D.chain0 < 0 || D.chain0 + D.batch > total_chains) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_init: this handle's chains [%lld, %lld) lie outside 0 .. total_chains", (long long)D.chain0, (long long)(D.chain0 + D.batch));
    if (betas[0] != 1.0) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_init: betas[0] must be 1 (the cold chain)");
    for (int i = 1; i < n_chains; ++i)
        if (!(betas[i] > 0) || !(betas[i] < betas[i - 1])) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_init: betas must decrease and stay positive");
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    mcd::Mc3Dev& C = m->mc3;
    double* ladder = nullptr;
    if (int rc = dev_alloc(m, &ladder, (size_t)n_chains, false)) return rc;
    if (int rc = dev_alloc(m, &C.rank, (size_t)total_chains, false)) return rc;
    if (int rc = dev_alloc(m, &C.tried, (size_t)n_chains, true)) return rc;
    if (int rc = dev_alloc(m, &C.accepted, (size_t)n_chains, true)) return rc;
    C.ladder = ladder;
    C.n_chains = n_chains;
    C.total = total_chains;
    std::vector<int32_t> rank((size_t)total_chains);
    std::vector<double> beta((size_t)D.batch);
    for (int64_t c = 0; c < total_chains; ++c) rank[(size_t)c] = (int32_t)(c % n_chains);
    for (int64_t b = 0; b < D.batch; ++b) beta[(size_t)b] = betas[(D.chain0 + b) % n_chains];
    MHIP_TRY(hipMemcpy(ladder, betas, sizeof(double) * (size_t)n_chains, hipMemcpyHostToDevice));
    MHIP_TRY(hipMemcpy(C.rank, rank.data(), sizeof(int32_t) * rank.size(), hipMemcpyHostToDevice));
    MHIP_TRY(hipMemcpy(D.beta, beta.data(), sizeof(double) * beta.size(), hipMemcpyHostToDevice));
    m->dev.lik_only = 0;
    m->mc3_seed = seed;
    m->mc3_phase = 0;
    m->mc3_ladder.assign(betas, betas + n_chains);
    return MCD_OK;
}

int mcd_mh_mc3_swap(mcd_mh_t* m, int n_swaps, const double* gathered, int world, int64_t chains_per_rank)
{
    if (!m) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_swap: NULL handle");
    const mcd::MhDev& D = m->dev;
    const mcd::Mc3Dev& C = m->mc3;
    if (C.n_chains == 0) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_swap: call mcd_mh_mc3_init first");
    if (n_swaps < 1 || n_swaps > C.n_chains - 1) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_swap: need 1 <= n_swaps <= n_chains - 1");
    if (gathered == nullptr) {                           // one rank: the sampler's own [3][batch]
        if (C.total != D.batch || D.chain0 != 0) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_swap: a handle that holds a shard of the chains needs the gathered ln posteriors");
        gathered = D.post;
        world = 1;
        chains_per_rank = D.batch;
    } else {
        // the swap kernel reads global chain c at gathered[c / chains_per_rank][.][c % chains_per_rank] and writes this handle's temperatures at
        // c - chain0: equal shards, this handle holding exactly the shard of rank chain0 / chains_per_rank -- anything else would silently
        // read another chain's ln posterior
        if (world < 1 || chains_per_rank < 1 || (int64_t)world * chains_per_rank != C.total)
            return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_swap: world x chains_per_rank must equal the global number of chains (%lld)", (long long)C.total);
        if (chains_per_rank != D.batch)
            return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_swap: chains_per_rank (%lld) is not this handle's batch (%lld): the shards must be equally large",
                         (long long)chains_per_rank, (long long)D.batch);
        if (D.chain0 % chains_per_rank != 0 || D.chain0 / chains_per_rank >= world)
            return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_swap: this handle's first chain (%lld) is not the start of a shard of %lld chains", (long long)D.chain0,
                         (long long)chains_per_rank);
    }
    MHIP_TRY(hipSetDevice(m->device));
    // enqueued on the sampler's stream, behind the run and the all-gather that produced `gathered`: no host synchronisation
    MHIP_TRY(mcd::launch_mc3_swap(C, gathered, world, chains_per_rank, n_swaps, m->mc3_seed, m->mc3_phase, D.beta, D.chain0, D.batch, m->stream));
    m->mc3_phase += 1;
    return MCD_OK;
}

int mcd_mh_mc3_get(const mcd_mh_t* cm, int32_t* rank, int64_t* tried, int64_t* accepted, double* beta)
{
    if (!cm) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_get: NULL handle");
    const mcd::Mc3Dev& C = cm->mc3;
    if (C.n_chains == 0) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_mc3_get: call mcd_mh_mc3_init first");
    MHIP_TRY(hipSetDevice(cm->device));
    MHIP_TRY(hipStreamSynchronize(cm->stream));
    if (rank) MHIP_TRY(hipMemcpy(rank, C.rank, sizeof(int32_t) * (size_t)C.total, hipMemcpyDeviceToHost));
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "");
    if (tried) MHIP_TRY(hipMemcpy(tried, C.tried, sizeof(int64_t) * (size_t)(C.n_chains - 1), hipMemcpyDeviceToHost));
    if (accepted) MHIP_TRY(hipMemcpy(accepted, C.accepted, sizeof(int64_t) * (size_t)(C.n_chains - 1), hipMemcpyDeviceToHost));
    if (beta) MHIP_TRY(hipMemcpy(beta, cm->dev.beta, sizeof(double) * (size_t)cm->dev.batch, hipMemcpyDeviceToHost));
    return MCD_OK;
}

}  // extern "C"

// ---- the chains of a leapfrog / NUTS handle become this handle's, on the device, and the Hamiltonian proposal in the cycle ----------
// (`maybeHamiltonianProposal`, app/Definitions.hs:272-278; handover_device.hpp, k_handover.hip)
namespace {

mcd::ChainArrays arrays_of(const mcd_mh* m) { return {m->dev.sc, m->dev.H, m->dev.R, m->dev.ld}; }

// m := the chains at src once `ready` has passed on the source's stream: what mcd_mh_set_state does behind its copies -- the same
// eval_posterior launches, so post and the prior blocks are those of the new states, and a run derives the rest when it starts.  No host wait.
int take_chains(mcd_mh* m, const mcd::ChainArrays& src, hipEvent_t ready)
{
    const mcd::MhDev& D = m->dev;
    if (ready) MHIP_TRY(hipStreamWaitEvent(m->stream, ready, 0));
    MHIP_TRY(mcd::launch_handover(arrays_of(m), src, D.batch, D.n_nodes, m->stream));
    if (int rc = eval_posterior(m, D.sc, D.H, D.R, D.post)) return rc;
    m->have_state = true;
    return MCD_OK;
}

}  // namespace

int mcd_mh_chains_(const mcd_mh* m, mcd::ChainsView* v, hipEvent_t* mark)
{
    if (!m || !v) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_chains_: NULL argument");
    *v = mcd::ChainsView{m->device, m->stream, m->dev.n_nodes, m->dev.batch, m->host_parent, m->have_state, arrays_of(m)};
    if (mark) {
        MHIP_TRY(hipSetDevice(m->device));
        if (!m->mark) MHIP_TRY(hipEventCreateWithFlags(&m->mark, hipEventDisableTiming));
        MHIP_TRY(hipEventRecord(m->mark, m->stream));
        *mark = m->mark;
    }
    return MCD_OK;
}

// ---- what the checkpoint calls need of the handle (ckpt_device.hpp, ckpt_capi.cpp) ------------------------------------------------------
int mcd_mh_ckpt_view_(const mcd_mh* m, mcd::CkptView* v)
{
    if (!m || !v) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_ckpt_view_: NULL argument");
    const mcd::RecCounts& rc = m->rec.counts();
    const mcd_mh::Hamiltonian& A = m->ham;
    *v = mcd::CkptView{m->device, m->stream, m->dev, m->mvn != nullptr, m->have_state, m->mvn ? m->mvn->n : m->sp->n, m->seed, m->step, m->n_samples,
                       m->host_parent, m->rows.data(), m->dims.data(), m->rec.active(), rc.period, rc.iter, rc.fetched, m->mc3, m->mc3_ladder.data(),
                       m->mc3_seed, m->mc3_phase, A.h != nullptr, A.max_depth, A.h ? mcd_hmc_dim(A.h) : 0, A.seed, A.first + A.done, A.counted, A.d_eps,
                       A.d_inv_mass, A.d_sums};
    return MCD_OK;
}

int mcd_mh_ckpt_stage_(mcd_mh* m, size_t bytes, void** p)
{
    if (bytes > m->ckpt_cap) {
        MHIP_TRY(hipSetDevice(m->device));
        MHIP_TRY(hipStreamSynchronize(m->stream));                // (nothing of an earlier save or load may still read the old blob)
        if (m->d_ckpt) {
            m->allocs.erase(std::find(m->allocs.begin(), m->allocs.end(), m->d_ckpt));
            (void)hipFree(m->d_ckpt);
            m->d_ckpt = nullptr;
            m->ckpt_cap = 0;
        }
        unsigned char* d = nullptr;
        if (int rc = dev_alloc(m, &d, bytes, false)) return rc;
        m->d_ckpt = d;
        m->ckpt_cap = bytes;
    }
    *p = m->d_ckpt;
    return MCD_OK;
}

int mcd_mh_ckpt_commit_(mcd_mh* m, const mcd::CkptCommit& c)
{
    m->have_state = true;
    if (!c.full) return MCD_OK;
    m->step = c.step;
    m->n_samples = c.n_samples;
    m->dev.lik_only = c.lik_only;
    if (c.rec) m->rec.restore(c.rec_iter, c.rec_fetched);
    if (m->mc3.n_chains != 0) m->mc3_phase = c.mc3_phase;
    if (m->ham.h) {
        m->ham.first = c.ham_next;
        m->ham.done = 0;
        m->ham.counted = c.ham_counted;
    }
    return MCD_OK;
}

extern "C" {

// m := the states h holds (include/mcmcdate_mvn.h): mcd_mh_set_state after mcd_hmc_get_state, without the host in between
int mcd_mh_take_state(mcd_mh_t* m, const mcd_hmc_t* h)
{
    if (!m || !h) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_take_state: NULL handle");
    mcd::ChainsView dst, src;
    if (int rc = mcd_mh_chains_(m, &dst, nullptr)) return rc;
    if (int rc = mcd_hmc_chains_(h, &src, nullptr)) return rc;
    char why[256];
    if (!mcd::handover_allowed(dst, src, why, sizeof why)) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_take_state: %s", why);
    hipEvent_t ready = nullptr;
    if (int rc = mcd_hmc_chains_(h, &src, &ready)) return rc;
    MHIP_TRY(hipSetDevice(m->device));
    if (int rc = take_chains(m, src.a, ready)) return rc;
    MHIP_TRY(hipStreamSynchronize(m->stream));
    return MCD_OK;
}

int mcd_mh_attach_hamiltonian(mcd_mh_t* m, mcd_hmc_t* h, const double* eps, const double* inv_mass, int max_depth, uint64_t seed, uint64_t first_transition)
{
    const char* who = "mcd_mh_attach_hamiltonian";
    if (!m || !h || !eps) return mfail(MCD_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (m->ham.h) return mfail(MCD_ERR_INVALID_ARG, "%s: a Hamiltonian proposal is attached to this handle already (mcd_mh_detach_hamiltonian first)", who);
    mcd::ChainsView mine, theirs;
    if (int rc = mcd_mh_chains_(m, &mine, nullptr)) return rc;
    if (int rc = mcd_hmc_chains_(h, &theirs, nullptr)) return rc;
    theirs.have_state = mine.have_state = true;                   // (neither needs a state yet: every transition starts with a hand-over)
    char why[256];
    if (!mcd::handover_allowed(theirs, mine, why, sizeof why)) return mfail(MCD_ERR_INVALID_ARG, "%s: %s", who, why);
    const mcd::MhDev& D = m->dev;
    const size_t B = (size_t)D.batch;
    for (size_t b = 0; b < B; ++b)
        if (!(eps[b] > 0) || !std::isfinite(eps[b])) return mfail(MCD_ERR_INVALID_ARG, "%s: step sizes must be positive and finite (chain %zu: %g)", who, b, eps[b]);
    if (max_depth < 1 || max_depth > mcd::kNutsMaxDepthLevels)
        return mfail(MCD_ERR_INVALID_ARG, "%s: max_depth must be 1 .. %d", who, mcd::kNutsMaxDepthLevels);
    const int dim = mcd_hmc_dim(h);
    for (int k = 0; k < dim && inv_mass; ++k)
        if (!(inv_mass[k] > 0) || !std::isfinite(inv_mass[k])) return mfail(MCD_ERR_INVALID_ARG, "%s: inverse masses must be positive", who);
    if (m->mc3.n_chains != 0) return mfail(MCD_ERR_UNSUPPORTED, "%s: Metropolis-coupled MCMC is initialised on this handle: a tempered Hamiltonian target is not built", who);
    if (D.lik_only) return mfail(MCD_ERR_UNSUPPORTED, "%s: the handle is in power-posterior mode (mcd_mh_set_power): a tempered Hamiltonian target is not built", who);
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    std::vector<double> beta(B);
    MHIP_TRY(hipMemcpy(beta.data(), D.beta, sizeof(double) * B, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b)
        if (beta[b] != 1.0)
            return mfail(MCD_ERR_UNSUPPORTED, "%s: chain %zu has the reciprocal temperature %g: a tempered Hamiltonian target is not built", who, b, beta[b]);
    if (int rc = mcd_hmc_cycle_ready_(h, who, inv_mass == nullptr)) return rc;
    // step sizes, inverse masses and the sums stay on the device for as long as the attachment lasts
    mcd_mh::Hamiltonian A;
    hipError_t e = hipMalloc((void**)&A.d_eps, sizeof(double) * B);
    if (e == hipSuccess && inv_mass) e = hipMalloc((void**)&A.d_inv_mass, sizeof(double) * (size_t)dim);
    if (e == hipSuccess) e = hipMalloc(&A.d_sums, 4 * 8 * B);
    if (e == hipSuccess) e = hipMemcpy(A.d_eps, eps, sizeof(double) * B, hipMemcpyHostToDevice);
    if (e == hipSuccess && inv_mass) e = hipMemcpy(A.d_inv_mass, inv_mass, sizeof(double) * (size_t)dim, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(A.d_sums, 0, 4 * 8 * B);
    if (e != hipSuccess) {
        A.release();
        return mfail(MCD_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    static_assert(sizeof(double) == 8 && sizeof(int64_t) == 8, "");
    A.sums = mcd::HamSums{(double*)A.d_sums, (int64_t*)A.d_sums + B, (int64_t*)A.d_sums + 2 * B, (int64_t*)A.d_sums + 3 * B};
    A.h = h;
    A.max_depth = max_depth;
    A.seed = seed;
    A.first = first_transition;
    m->ham = A;
    return MCD_OK;
}

int mcd_mh_detach_hamiltonian(mcd_mh_t* m)
{
    if (!m) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_detach_hamiltonian: NULL handle");
    if (!m->ham.h) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_detach_hamiltonian: no Hamiltonian proposal is attached to this handle");
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipStreamSynchronize(m->stream));                    // (every run ends with this wait: nothing of the attachment is in flight)
    m->ham.release();
    return MCD_OK;
}

int mcd_mh_hamiltonian_stats(const mcd_mh_t* cm, int64_t* transitions, double* alpha_sum, int64_t* depth_sum, int64_t* leapfrog_steps, int64_t* divergent,
                             int reset)
{
    if (!cm) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_hamiltonian_stats: NULL handle");
    const mcd_mh::Hamiltonian& A = cm->ham;
    if (!A.h) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_hamiltonian_stats: no Hamiltonian proposal is attached to this handle");
    const size_t B = (size_t)cm->dev.batch;
    MHIP_TRY(hipSetDevice(cm->device));
    MHIP_TRY(hipStreamSynchronize(cm->stream));
    if (transitions) *transitions = A.counted;
    if (alpha_sum) MHIP_TRY(hipMemcpy(alpha_sum, A.sums.alpha, 8 * B, hipMemcpyDeviceToHost));
    if (depth_sum) MHIP_TRY(hipMemcpy(depth_sum, A.sums.depth, 8 * B, hipMemcpyDeviceToHost));
    if (leapfrog_steps) MHIP_TRY(hipMemcpy(leapfrog_steps, A.sums.leaves, 8 * B, hipMemcpyDeviceToHost));
    if (divergent) MHIP_TRY(hipMemcpy(divergent, A.sums.diverged, 8 * B, hipMemcpyDeviceToHost));
    if (reset) {
        MHIP_TRY(hipMemset(A.d_sums, 0, 4 * 8 * B));
        const_cast<mcd_mh*>(cm)->ham.counted = 0;                 // (the sums are the attachment's, not the chains': reading them may clear them)
    }
    return MCD_OK;
}

}  // extern "C"

namespace {

// ---- mcd_mh_run: a plan per run, one runner per family of launch structures ----------------------------------------------------

// the knobs (mcd_set_option) that a run depends on, read once when it starts: MCD_OPT_UNSET or the value
struct MhOptions {
    int per_phase, segments, incremental, prior, prior_cache, step_wg, chain_lw, prior_waves, seg_tail, ahead_from, prior_draws;
};

MhOptions mh_options()
{
    using mcd::opt_get;
    return MhOptions{opt_get(mcd::OPT_MH_PER_PHASE), opt_get(mcd::OPT_MH_SEGMENTS), opt_get(mcd::OPT_MH_INCREMENTAL), opt_get(mcd::OPT_MH_PRIOR),
                     opt_get(mcd::OPT_MH_PRIOR_CACHE), opt_get(mcd::OPT_MH_STEP_WG), opt_get(mcd::OPT_MH_CHAIN_LW), opt_get(mcd::OPT_MH_PRIOR_WAVES),
                     opt_get(mcd::OPT_MH_SEG_TAIL), opt_get(mcd::OPT_MH_AHEAD_FROM), opt_get(mcd::OPT_MH_PRIOR_DRAWS)};
}

// what a plan depends on besides the knobs: the handle's shape and its create-time decisions, as plain facts
struct MhShape {
    int n_nodes, n_prop;
    int64_t batch;
    bool dense;              // a dense likelihood (mvn), else a sparse one (sp)
    mcd::MvnFacts mvn;
    mcd::SparseFacts sp;
    bool chain_kernel, list_all;
};

MhShape shape_of(const mcd_mh* m)
{
    MhShape s{m->dev.n_nodes, m->dev.n_prop, m->dev.batch, m->mvn != nullptr, {}, {}, m->chain_kernel, m->list_all};
    if (m->mvn) s.mvn = *m->mvn;
    else s.sp = *m->sp;
    return s;
}

// every decision that the launches of one run depend on
struct MhPlan {
    int path = MCD_MH_PATH_NONE;
    const char* refused = nullptr;   // path NONE: why the run cannot be served
    bool likelihood_wave = false;    // small-tree kernel: the likelihood by a second wave per chain, beside the prior
    bool incremental = false;        // streamed chain kernel / per-step paths: sparse proposals by columns of L^-1 on a kept z
    bool beside = false, use_x = false, step_wg = false, keep = false;   // see plan_run
    bool inc_dense = false, inc_sparse = false, chunked = false, segments = false, tails = false;
    bool prior_waves = false, prior_draws = false;   // the segment kernels' prior waves, which also draw the next proposal
    int ahead_from = 0;              // MhSegPending::ahead_from
    int flags() const
    {
        const bool f[] = {likelihood_wave, incremental, beside, use_x, step_wg, keep, inc_dense, inc_sparse, chunked, segments, tails, prior_waves, prior_draws};
        int r = 0;
        for (int i = 0; i < (int)(sizeof f / sizeof f[0]); ++i) r |= (f[i] ? 1 : 0) << i;
        return r;
    }
};

MhPlan plan_run(const MhShape& s, const MhOptions& o)
{
    MhPlan p;
    const bool per_phase = o.per_phase == 1, seg_off = o.segments == 0, inc_off = o.incremental == 0;
    p.likelihood_wave = o.chain_lw != 0;
    p.incremental = !inc_off;
    p.prior_waves = o.prior_waves != 0;
    p.prior_draws = o.prior_draws != 0 && p.prior_waves;
    p.ahead_from = o.ahead_from != mcd::MCD_OPT_UNSET ? o.ahead_from : mcd::kSegAheadFrom;
    if (s.chain_kernel) {                      // trees of at most 64 nodes (mcd_mh_create): the whole schedule in one launch
        p.path = MCD_MH_PATH_CHAIN_LDS;
        return p;
    }
    // Larger trees at a sampler's batch: the whole schedule in one launch as well, the factor streamed once per step (k_mh_chain_big.hip).
    // From 259 nodes (R >= 6) the segment path is ahead of it (271 nodes x 512 chains 11.3 -> 9.6 us per lock step, 513 nodes 16.0 -> 9.6):
    // the factor streamed for every dense proposal costs more there than two launches for the few proposals that move more than 192
    // distances.
    const int64_t split_batch = std::min<int64_t>(s.batch, mcd::kSplitMaxBatch);
    const bool prefer_segments = s.dense && !seg_off && !inc_off && mcd::mh_segment_available(s.mvn, s.n_nodes, s.batch) && mcd::use_split(s.mvn, split_batch);
    if (s.dense && !per_phase && s.mvn.form != MCD_FORM_MULTIPLY && mcd::mh_chain_big_available(s.mvn, s.n_nodes, s.n_prop, s.batch) && !prefer_segments) {
        p.path = MCD_MH_PATH_CHAIN_STREAMED;
        return p;
    }
    // two launches per step: [accept step s-1 + propose step s + ln prior] and [likelihood + root-branch Jacobian]
    if ((size_t)s.n_nodes * 32 > 64 * 1024) {
        p.refused = "more than 2048 nodes";
        return p;
    }
    // The ln prior of a proposed state depends on the proposal only, like its ln likelihood: where the sweep serves the likelihood launch,
    // that launch carries the prior as workgroups of a second role (k_tree_logpdf.hip, mh_prior_role.hpp) and the step kernel leaves it out.
    // (A launch of its own for the prior with four waves per chain was measured for the larger trees: 58.9 -> 56.4 us per lock step at
    // 1025 nodes, 33.3 -> 35.4 at 513 -- the step kernel's other strided loops weigh more there; not kept.)
    p.beside = s.dense && !prefer_segments && o.prior != 0 && mcd::tree_logpdf_can_carry_prior(s.mvn, s.batch, s.n_nodes);
    const bool prior_inline = !p.beside;
    // Large trees: the workgroup-per-chain step kernel leaves the proposed states' DISTANCES, the likelihood launch takes them as plain
    // vectors (the row-split kernel's tree staging costs 6 us more at 1023 slots); same arithmetic, same bits.  MCD_MH_STEP_WG = 1 / 0
    // forces / forbids that step kernel.
    const int wg_from = !s.dense ? 0 : prefer_segments ? 258 : 320;
    const bool wg_fits = mcd::mh_step_wg_fits(s.n_nodes);
    auto wg_for = [&](int min_nodes) { return (o.step_wg != mcd::MCD_OPT_UNSET ? o.step_wg != 0 : (prior_inline && s.n_nodes > min_nodes)) && wg_fits; };
    p.use_x = wg_for(wg_from) && !p.beside && s.n_nodes > wg_from;
    if (!s.dense && !p.use_x) {
        p.refused = "the sparse driver needs the workgroup-per-chain step kernel (MCD_MH_STEP_WG must not be 0)";
        return p;
    }
    p.step_wg = p.use_x || wg_for(320);
    p.keep = prior_inline && wg_for(wg_from) && o.prior_cache != 0;   // (MCD_MH_PRIOR_CACHE = 0: every summand at every step)
    // Large trees at a sampler's batch: the likelihood launch only for the proposals that move many distances (k_mh_inc.hip); the others
    // are evaluated from columns of L^-1 on the kept z.  Over a sparse precision matrix (k_mh_segment_sparse.hip) the incremental form keeps
    // the quadratic form q itself (MhInc with NPz = 1); it exists only together with the segments.
    p.inc_dense = s.dense && p.use_x && !inc_off && s.mvn.cols && 64 * s.mvn.R <= 1024 && mcd::use_split(s.mvn, split_batch);
    p.inc_sparse = !s.dense && p.use_x && !inc_off && !seg_off && mcd::mh_segment_sparse_available(s.sp, s.n_nodes, s.batch) &&
                   mcd::sparse_quad_available(s.sp, s.batch);
    p.chunked = p.inc_dense && s.batch > mcd::kSplitMaxBatch;
    // Trees of 259 .. 1026 nodes: the runs of steps between two dense proposals as ONE launch each, every chain's state in LDS
    // (k_mh_segment.hip); a dense proposal: its likelihood by the row-split launch, decided by the step kernel or the next segment
    p.segments = p.inc_sparse || (p.inc_dense && !seg_off && mcd::mh_segment_available(s.mvn, s.n_nodes, s.batch));
    p.tails = p.keep && o.seg_tail != 0;
    p.path = p.segments ? (p.inc_sparse ? MCD_MH_PATH_SEGMENTS_SPARSE : MCD_MH_PATH_SEGMENTS)
             : !s.dense ? MCD_MH_PATH_STEP_WG_SPARSE
             : p.inc_dense ? MCD_MH_PATH_STEP_WG_INCREMENTAL
             : p.use_x ? MCD_MH_PATH_STEP_WG_X
             : p.beside ? MCD_MH_PATH_TWO_LAUNCH_PRIOR_BESIDE : MCD_MH_PATH_TWO_LAUNCH;
    return p;
}

// the device buffers of the per-step paths, allocated on first use: the proposed distances (d_X1), the kept summands of the ln prior
// (d_psum, d_psel), the arrays of the incremental likelihood (MhInc)
int plan_buffers(mcd_mh* m, const MhPlan& p)
{
    mcd::MhDev& D = m->dev;
    const size_t B = (size_t)D.batch, n_dim = (size_t)(m->mvn ? m->mvn->n : m->sp->n);
    if (p.use_x && m->d_X1 == nullptr)
        if (int rc = dev_alloc(m, &m->d_X1, B * n_dim, false)) return rc;
    if (p.keep && m->d_psum == nullptr) {
        const size_t NS = (size_t)((D.n_nodes - 1 + 63) / 64) * 64;
        if (int rc = dev_alloc(m, &m->d_psum, B * 4 * NS, false)) return rc;
        if (int rc = dev_alloc(m, &m->d_psel, 2 * B, false)) return rc;
    }
    D.psum = p.keep ? m->d_psum : nullptr;
    D.psel = p.keep ? m->d_psel : nullptr;
    mcd::MhInc& I = m->inc;
    if (p.inc_sparse && I.X0 == nullptr) {            // zcur / zprop = q of the current states / of the pending dense proposal
        I.NPz = 1;
        if (int rc = dev_alloc(m, &I.X0, B * n_dim, false)) return rc;
        if (int rc = dev_alloc(m, &I.zcur, 2 * B, false)) return rc;
        I.zprop = I.zcur + B;
    }
    if (p.inc_dense && I.X0 == nullptr) {
        I.NPz = 64 * m->mvn->R;
        if (int rc = dev_alloc(m, &I.X0, B * n_dim, false)) return rc;
        if (int rc = dev_alloc(m, &I.zcur, B * (size_t)I.NPz, false)) return rc;
        if (int rc = dev_alloc(m, &I.zprop, B * (size_t)I.NPz, false)) return rc;
        if (int rc = dev_alloc(m, &m->d_inc_ll, B, false)) return rc;
    }
    return MCD_OK;
}

const mcd::MhRow kNoRow{0, 0, 0, 0, 0, 1.0, 0.0};

// one run of a plan: the handle, the schedule and what the runners share
struct MhRun {
    mcd_mh* m;
    const MhPlan& p;
    const int32_t* schedule;         // (host) position 0 of this run
    int64_t off;                     // where that position lies in the call's device schedule and traces (m->d_sched, m->d_trace_*)
    int64_t total;                   // steps
    int32_t S;
    int accumulate;
    bool trace;
    uint64_t step_base;              // the step number of schedule position 0
    int n_dim;
    int prior_inline;
    const mcd::TreeDev* Tx;          // the step kernel's distances (use_x)
    double* X1;
    bool inc;
    int dense_mode;                  // where the z' (q') of a dense proposal is afterwards: zprop (1) or the z tiles (2)
    mcd::MhRec rec;                  // the sample recorder as it stands when the call starts (base null: off)

    MhRun(mcd_mh* m_, const MhPlan& p_, const int32_t* schedule_, int64_t off_, int64_t total_, int32_t S_, int accumulate_, bool trace_)
        : m(m_), p(p_), schedule(schedule_), off(off_), total(total_), S(S_), accumulate(accumulate_), trace(trace_), step_base(m_->step),
          n_dim(m_->mvn ? m_->mvn->n : m_->sp->n), prior_inline(p_.beside ? 0 : 1), Tx(p_.use_x ? m_->tree : nullptr), X1(p_.use_x ? m_->d_X1 : nullptr),
          inc(p_.inc_dense || p_.inc_sparse), dense_mode((p_.chunked || p_.inc_sparse) ? 1 : 2),
          rec(m_->rec.view(m_->rec.counts().iter)) {}
    // what the next launch sees of the recorder (MhDev::rec): a whole-schedule or segment launch whose step 0 is `steps_before` steps (whole
    // iterations) into the call; a step launch that decides schedule position gs (gs < 0: decides nothing); nothing
    void rec_launch(int64_t steps_before) const
    {
        m->dev.rec = rec;
        m->dev.rec.iter0 += steps_before / S;
    }
    void rec_step(int64_t gs) const
    {
        m->dev.rec = rec;
        if (gs < 0 || (gs + 1) % S != 0) m->dev.rec.base = nullptr;
        else m->dev.rec.iter0 += (gs + 1) / S;
    }
    double* alpha(int64_t gs) const { return trace ? m->d_trace_alpha + (off + gs) * m->dev.batch : nullptr; }
    int8_t* accept(int64_t gs) const { return trace ? m->d_trace_accept + (off + gs) * m->dev.batch : nullptr; }
    // the schedule positions [first, first + count) as one launch of a persistent kernel takes them
    mcd::MhSpan span(int64_t first, int64_t n) const { return {m->d_sched + off + first, n, S, accumulate ? 1 : 0, step_base + (uint64_t)first, m->seed, alpha(first), accept(first)}; }
    // the step launch that only proposes schedule position gs (nothing is pending, so no uniform is drawn from the step number; init: MhDev::psum
    // does not hold the current states' summands yet), and the one that decides position gs and proposes row pn (< 0: none) for position gs + 1
    mcd::MhStep propose(int64_t gs, bool init) const { return {-1, 0, schedule[gs], m->rows[(size_t)schedule[gs]], (int)(gs & 63), m->step, 0, nullptr, nullptr, init ? 1 : 0}; }
    mcd::MhStep decide(int64_t gs, int pn) const
    {
        return {schedule[gs], m->rows[(size_t)schedule[gs]].jac_root, pn, pn >= 0 ? m->rows[(size_t)pn] : kNoRow, (int)((gs + 1) & 63), m->step,
                (accumulate && (gs + 1) % S == 0) ? 1 : 0, alpha(gs), accept(gs), 0};
    }

    // the draws of schedule positions [64 k, 64 k + 64) are computed when position 64 k is about to be proposed
    int draws_for(int64_t idx) const
    {
        if ((idx & 63) == 0) {
            const int count = (int)((total - idx < 64) ? total - idx : 64);
            MHIP_TRY(mcd::launch_mh_draws(m->dev, m->d_sched + off, idx, count, step_base + (uint64_t)idx, m->seed, m->stream));
        }
        return MCD_OK;
    }
    // ll and z = L^-1 (X - mu) of every chain by full products (the row-split kernel, at most 1024 chains per launch); z to dst
    // (chain-major) -- or, for a batch of one launch and dst = null, left in that launch's z tiles
    int z_product(const double* X, double* ll, double* dst) const
    {
        const mcd::MhDev& D = m->dev;
        mcd::MhInc& I = m->inc;
        if (p.inc_sparse) {                            // the full form in one launch (k_sparse.hip: k_sparse_quad): ll and q (dst)
            MHIP_TRY(mcd::launch_sparse_quad(*m->sp, nullptr, X, nullptr, n_dim, nullptr, nullptr, D.batch, ll, nullptr, dst, m->stream));
            return MCD_OK;
        }
        for (int64_t c0 = 0; c0 < D.batch; c0 += mcd::kSplitMaxBatch) {
            const int64_t cnt = std::min<int64_t>(mcd::kSplitMaxBatch, D.batch - c0);
            MHIP_TRY(mcd::launch_logpdf_split_z(*m->mvn, X + c0 * n_dim, n_dim, cnt, ll + c0, &I.zt, &I.nr, m->stream));
            if (dst) MHIP_TRY(mcd::launch_mh_inc_take_z(I, dst, c0, cnt, m->stream));
        }
        return MCD_OK;
    }
    // (dense: the ll of that product is not used -- q is |z'|^2 afresh at every step; sparse: q itself is what is kept, and the chains' ln
    // likelihood is set to the recomputed value with it, so that the two stay the same number)
    int refresh_z() const { return z_product(m->inc.X0, p.inc_sparse ? m->dev.post + m->dev.batch : m->d_inc_ll, m->inc.zcur); }
    // how the likelihood of proposal row q is evaluated: 0 not moved, 1 by columns of L^-1 (rows of the matrix), 2 by a full product
    int inc_mode(int q) const
    {
        if (q < 0) return 0;
        const mcd::MhRow& r = m->rows[(size_t)q];
        if (r.kind == MCD_PROP_SCALE_SCALAR && (r.node == 0 || r.node == 1 || r.node == 4)) return 0;
        return m->sparse_rows[(size_t)q] ? 1 : 2;
    }
    // what both per-step runners start with: the first block of draws, X0 and z of the current states
    int begin() const
    {
        if (int rc = draws_for(0)) return rc;
        if (inc) {
            m->inc.mode = 0;
            MHIP_TRY(mcd::launch_mh_inc_init(m->dev, *m->tree, m->inc, n_dim, n_dim, m->stream));
            if (int rc = refresh_z()) return rc;
        }
        return MCD_OK;
    }
};

int run_chain(const MhRun& r)
{
    mcd_mh* m = r.m;
    r.rec_launch(0);
    MHIP_TRY(mcd::launch_mh_chain(m->dev, *m->mvn, *m->tree, *m->prior, m->d_Fp, r.span(0, r.total), r.p.likelihood_wave, m->stream));
    m->step += (uint64_t)r.total;
    if (r.accumulate) m->n_samples += r.total / r.S;
    return MCD_OK;
}

int run_streamed(const MhRun& r)
{
    mcd_mh* m = r.m;
    // (launches of at most ~64 k steps, whole iterations each: a second or so of kernel time; what a launch costs -- the chains' state in,
    // out again -- is some 20 us)
    const int64_t per_launch = (int64_t)r.S * (65536 / r.S > 0 ? 65536 / r.S : 1);
    for (int64_t done = 0; done < r.total; done += per_launch) {
        const int64_t now = (r.total - done < per_launch) ? r.total - done : per_launch;
        r.rec_launch(done);
        MHIP_TRY(mcd::launch_mh_chain_big(m->dev, *m->mvn, *m->tree, *m->prior, r.span(done, now), r.p.incremental, m->stream));
        m->step += (uint64_t)now;
    }
    if (r.accumulate) m->n_samples += r.total / r.S;
    return MCD_OK;
}

// the segment paths (MCD_MH_PATH_SEGMENTS, _SEGMENTS_SPARSE): every run of steps between two dense proposals in one launch
int run_segments(const MhRun& r)
{
    mcd_mh* m = r.m;
    const MhPlan& p = r.p;
    mcd::MhDev& D = m->dev;
    mcd::MhInc& I = m->inc;
    const int32_t* schedule = r.schedule;
    const int64_t total = r.total;
    if (int rc = r.begin()) return rc;
    static const mcd::MvnDev no_mvn{};                   // (k_mh_step_wg takes the incremental bookkeeping only with an MvnDev beside it)
    const mcd::MhStepRun steps{r.prior_inline, p.step_wg, r.Tx, r.n_dim, r.X1, r.n_dim, &I, m->mvn ? m->mvn : &no_mvn};
    bool summands_kept = false;                      // MhDev::psum holds the current states' summands
    int64_t draws_block = 0;                         // (begin: draws_for(0))
    auto need_draws = [&](int64_t idx) -> int {
        if ((idx >> 6) != draws_block) {
            draws_block = idx >> 6;
            return r.draws_for(idx & ~(int64_t)63);
        }
        return MCD_OK;
    };
    // a dense proposal followed by a segment is decided by that segment's launch (k_mh_segment.hip: MhSegPending), not by a
    // launch of the step kernel that would do nothing else
    mcd::MhSegPending pending{};
    pending.p_acc = -1;
    pending.ahead_from = p.ahead_from;
    pending.prior_draws = p.prior_draws ? 1 : 0;
    bool have_pending = false;
    // ... and a dense proposal that follows a segment is PROPOSED by that segment's launch, from the state it holds in LDS
    // (MhSegPending::p_tail), not by a launch of the step kernel that reads everything back first.  MCD_MH_SEG_TAIL=0: by the step kernel.
    bool proposed = false;                           // schedule[gs] is already proposed (by the segment before it)
    int64_t gs = 0;
    while (gs < total) {
        if (r.inc_mode(schedule[gs]) != 2) {
            int64_t e = gs + 1;                      // ... up to the next recomputation of z (every 256 steps)
            while (e < total && r.inc_mode(schedule[e]) != 2 && (e & 255) != 0) ++e;
            if (!have_pending) pending.p_acc = -1;
            pending.p_tail = (p.tails && e < total && r.inc_mode(schedule[e]) == 2) ? schedule[e] : -1;
            pending.X1_tail = r.X1;
            proposed = pending.p_tail >= 0;
            r.rec_launch(0);                         // (the segment kernels count from the call's first step: gs_base + their own)
            if (p.inc_sparse)
                MHIP_TRY(mcd::launch_mh_segment_sparse(D, *m->sp, *m->tree, *m->prior, I, r.span(gs, e - gs), gs, summands_kept ? 1 : 0, pending,
                                                       m->list_all ? 1 : 0, p.prior_waves, m->stream));
            else
                MHIP_TRY(mcd::launch_mh_segment(D, *m->mvn, *m->tree, *m->prior, I, r.span(gs, e - gs), gs, summands_kept ? 1 : 0, pending, p.prior_waves, m->stream));
            have_pending = false;
            if (D.psum != nullptr) summands_kept = true;
            if (r.accumulate) m->n_samples += (e / r.S) - (gs / r.S);      // iterations closed by steps gs .. e - 1
            m->step += (uint64_t)(e - gs);
            gs = e;
            if ((gs & 255) == 0 && gs < total)
                if (int rc = r.refresh_z()) return rc;
            continue;
        }
        // a dense proposal (and those that follow it directly)
        if (!proposed) {
            if (int rc = need_draws(gs)) return rc;
            I.mode = 0;
            I.prop_mode = 2;
            r.rec_step(-1);
            MHIP_TRY(mcd::launch_mh_step(D, *m->prior, steps, r.propose(gs, !summands_kept), m->seed, m->stream));
            if (D.psum != nullptr) summands_kept = true;
        }
        proposed = false;
        while (true) {
            const int pa = schedule[gs];
            if (int rc = r.z_product(r.X1, D.post1 + D.batch, (p.chunked || p.inc_sparse) ? I.zprop : nullptr)) return rc;
            I.mode = r.dense_mode;
            const bool closes = ((gs + 1) % r.S) == 0;
            const bool refresh_now = ((gs + 1) & 255) == 0;
            const int pn = (gs + 1 < total && r.inc_mode(schedule[gs + 1]) == 2) ? schedule[gs + 1] : -1;
            if (pn >= 0)
                if (int rc = need_draws(gs + 1)) return rc;
            if (pn < 0 && gs + 1 < total && !refresh_now && D.psum != nullptr && summands_kept) {
                pending.p_acc = pa;
                pending.jac_root = m->rows[pa].jac_root;
                pending.accumulate = (r.accumulate && closes) ? 1 : 0;
                pending.step = m->step;
                pending.trace_alpha = r.alpha(gs);
                pending.trace_accept = r.accept(gs);
                pending.X1 = r.X1;
                pending.z_in_zprop = p.chunked ? 1 : 0;
                have_pending = true;
                m->step += 1;
                if (r.accumulate && closes) m->n_samples += 1;
                gs += 1;
                break;
            }
            I.prop_mode = 2;
            r.rec_step(gs);
            MHIP_TRY(mcd::launch_mh_step(D, *m->prior, steps, r.decide(gs, pn), m->seed, m->stream));
            if (refresh_now && gs + 1 < total)
                if (int rc = r.refresh_z()) return rc;
            m->step += 1;
            if (r.accumulate && closes) m->n_samples += 1;
            gs += 1;
            if (pn < 0) break;
        }
    }
    return MCD_OK;
}

// the two-launch step loop (MCD_MH_PATH_TWO_LAUNCH .. _STEP_WG_SPARSE): [accept step s-1 + propose step s] and [the likelihood of step s]
int run_steps(const MhRun& r)
{
    mcd_mh* m = r.m;
    mcd::MhDev& D = m->dev;
    mcd::MhInc& I = m->inc;
    const int32_t* schedule = r.schedule;
    if (int rc = r.begin()) return rc;
    const mcd::MhStepRun steps{r.prior_inline, r.p.step_wg, r.Tx, r.n_dim, r.X1, r.n_dim, r.inc ? &I : nullptr, m->mvn};
    I.prop_mode = r.inc ? r.inc_mode(schedule[0]) : 0;
    r.rec_step(-1);
    MHIP_TRY(mcd::launch_mh_step(D, *m->prior, steps, r.propose(0, true), m->seed, m->stream));
    for (int64_t gs = 0; gs < r.total; ++gs) {
        const int pa = schedule[gs];
        if (r.inc) {
            I.mode = r.inc_mode(pa);                 // the step kernel evaluated modes 0 and 1 itself
            if (I.mode == 2) {
                if (int rc = r.z_product(r.X1, D.post1 + D.batch, r.p.chunked ? I.zprop : nullptr)) return rc;
                I.mode = r.dense_mode;
            }
        } else if (m->sp) {
            double* scr = nullptr;
            if (int rc = mcd_sparse_scratch_(m->sp_handle, m->stream, D.batch, &scr)) return rc;
            MHIP_TRY(mcd::launch_sparse_logpdf(*m->sp, r.X1, r.n_dim, D.batch, D.post1 + D.batch, scr, m->stream));
        } else if (r.p.use_x)
            MHIP_TRY(mcd::launch_logpdf(*m->mvn, r.X1, r.n_dim, D.batch, D.post1 + D.batch, m->stream));
        else if (r.p.beside)
            MHIP_TRY(mcd::launch_tree_logpdf_with_prior(*m->mvn, *m->tree, D.H1, D.R1, D.ld, D.sc1 + 2 * D.batch, D.sc1 + 3 * D.batch, D.batch,
                                                        D.post1 + D.batch, D.post1 + 2 * D.batch, D, *m->prior, m->stream));
        else
            MHIP_TRY(mcd::launch_tree_logpdf(*m->mvn, *m->tree, D.H1, D.R1, D.ld, D.sc1 + 2 * D.batch, D.sc1 + 3 * D.batch, D.batch,
                                             D.post1 + D.batch, D.post1 + 2 * D.batch, m->stream));
        const bool closes = ((gs + 1) % r.S) == 0;
        const int pn = (gs + 1 < r.total) ? schedule[gs + 1] : -1;
        if (pn >= 0)
            if (int rc = r.draws_for(gs + 1)) return rc;
        const bool refresh_now = r.inc && ((gs + 1) & 255) == 0;
        I.prop_mode = r.inc ? r.inc_mode(pn) : 0;
        r.rec_step(gs);
        MHIP_TRY(mcd::launch_mh_step(D, *m->prior, steps, r.decide(gs, pn), m->seed, m->stream));
        if (refresh_now)                                 // (X0 is exact; z has been updated column by column since the last full product)
            if (int rc = r.refresh_z()) return rc;
        m->step += 1;
        if (r.accumulate && closes) m->n_samples += 1;
    }
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_mh_run(mcd_mh_t* m, const int32_t* schedule, int64_t n_iter, int32_t S, int accumulate, double* trace_alpha,
               int8_t* trace_accept)
{
    if (!m) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_run: NULL handle");
    if (!m->have_state) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_run: call mcd_mh_set_state first");
    if (n_iter < 0 || S <= 0 || (n_iter > 0 && !schedule)) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_run: bad schedule");
    if (n_iter == 0) return MCD_OK;
    mcd::note_dynamic_lds(0);
    mcd::MhDev& D = m->dev;
    const size_t steps = (size_t)n_iter * (size_t)S;
    for (size_t i = 0; i < steps; ++i)
        if (schedule[i] < 0 || schedule[i] >= D.n_prop) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_run: schedule[%zu] = %d is not a proposal row", i, schedule[i]);
    if (int rc = m->rec.room("mcd_mh_run", n_iter)) return rc;   // an active recorder: the samples of this call must fit, or nothing is launched
    if (m->ham.h)                                                // an attachment: may its handle make the transitions, or nothing is launched
        if (int rc = mcd_hmc_cycle_ready_(m->ham.h, "mcd_mh_run", m->ham.d_inv_mass == nullptr)) return rc;
    MHIP_TRY(hipSetDevice(m->device));
    if (steps > m->sched_cap) {
        if (m->d_sched) (void)hipFree(m->d_sched);
        m->d_sched = nullptr;
        m->sched_cap = 0;
        MHIP_TRY(hipMalloc((void**)&m->d_sched, sizeof(int32_t) * steps));
        m->sched_cap = steps;
    }
    MHIP_TRY(hipMemcpyAsync(m->d_sched, schedule, sizeof(int32_t) * steps, hipMemcpyHostToDevice, m->stream));
    const bool trace = trace_alpha || trace_accept;
    const size_t B = (size_t)D.batch;
    if (trace && steps * B > m->trace_cap) {
        if (m->d_trace_alpha) (void)hipFree(m->d_trace_alpha);
        if (m->d_trace_accept) (void)hipFree(m->d_trace_accept);
        m->d_trace_alpha = nullptr;
        m->d_trace_accept = nullptr;
        m->trace_cap = 0;
        MHIP_TRY(hipMalloc((void**)&m->d_trace_alpha, sizeof(double) * steps * B));
        MHIP_TRY(hipMalloc((void**)&m->d_trace_accept, steps * B));
        m->trace_cap = steps * B;
    }
    const MhPlan p = plan_run(shape_of(m), mh_options());
    if (p.path == MCD_MH_PATH_NONE) return mfail(MCD_ERR_UNSUPPORTED, "mcd_mh_run: %s", p.refused);
    if (p.path != MCD_MH_PATH_CHAIN_LDS && p.path != MCD_MH_PATH_CHAIN_STREAMED)
        if (int rc = plan_buffers(m, p)) return rc;
    m->last_path = p.path;
    // the iterations [first, first + count) of the call as one run of the plan
    auto stretch = [&](int64_t first, int64_t count) -> int {
        const MhRun r(m, p, schedule + first * S, first * S, count * S, S, accumulate, trace);
        const int rc = p.path == MCD_MH_PATH_CHAIN_LDS ? run_chain(r) : p.path == MCD_MH_PATH_CHAIN_STREAMED ? run_streamed(r) : p.segments ? run_segments(r) : run_steps(r);
        m->dev.rec = mcd::MhRec{};
        if (rc) return rc;
        m->rec.advance(count);
        return MCD_OK;
    };
    if (!m->ham.h) {
        if (int rc = stretch(0, n_iter)) return rc;
    } else {
        // Every iteration begins with one NUTS transition of every chain on the attached handle, and the scheduled proposals follow as a
        // run of their own: mcd_hmc_take_state, mcd_hmc_nuts, mcd_mh_take_state, mcd_mh_run of one iteration, to the bit.  The two
        // streams are ordered by the handles' events; the host waits only where mcd_hmc_nuts waits.
        mcd_mh::Hamiltonian& A = m->ham;
        for (int64_t it = 0; it < n_iter; ++it) {
            mcd::ChainsView me;
            hipEvent_t mine = nullptr, theirs = nullptr;
            if (int rc = mcd_mh_chains_(m, &me, &mine)) return rc;
            if (int rc = mcd_hmc_cycle_transition_(A.h, me.a, mine, A.d_eps, A.d_inv_mass, A.max_depth, A.seed, D.chain0, A.first + A.done, A.sums, &theirs))
                return rc;
            A.done += 1;
            A.counted += 1;
            mcd::ChainsView other;
            if (int rc = mcd_hmc_chains_(A.h, &other, nullptr)) return rc;
            if (int rc = take_chains(m, other.a, theirs)) return rc;
            if (int rc = stretch(it, 1)) return rc;
        }
    }
    m->last_lds = mcd::last_dynamic_lds();
    if (trace_alpha) MHIP_TRY(hipMemcpyAsync(trace_alpha, m->d_trace_alpha, sizeof(double) * steps * B, hipMemcpyDeviceToHost, m->stream));
    if (trace_accept) MHIP_TRY(hipMemcpyAsync(trace_accept, m->d_trace_accept, steps * B, hipMemcpyDeviceToHost, m->stream));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    return MCD_OK;
}

int mcd_mh_tune(mcd_mh_t* m)
{
    if (!m) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_tune: NULL handle");
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(mcd::launch_mh_tune(m->dev, m->stream));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    return MCD_OK;
}

int mcd_mh_get_tuning(const mcd_mh_t* cm, double* tune, int32_t* accepted, int32_t* tried)
{
    if (!cm) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_get_tuning: NULL handle");
    const mcd::MhDev& D = cm->dev;
    MHIP_TRY(hipSetDevice(cm->device));
    MHIP_TRY(hipStreamSynchronize(cm->stream));
    const size_t BP = (size_t)D.batch * (size_t)D.n_prop;
    if (tune) MHIP_TRY(hipMemcpy(tune, D.tune, sizeof(double) * BP, hipMemcpyDeviceToHost));
    if (accepted) MHIP_TRY(hipMemcpy(accepted, D.acc, sizeof(int32_t) * BP, hipMemcpyDeviceToHost));
    if (tried) MHIP_TRY(hipMemcpy(tried, D.tried, sizeof(int32_t) * BP, hipMemcpyDeviceToHost));
    return MCD_OK;
}

int mcd_mh_set_tuning(mcd_mh_t* m, const double* tune)
{
    if (!m || !tune) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_set_tuning: NULL argument");
    const mcd::MhDev& D = m->dev;
    const size_t BP = (size_t)D.batch * (size_t)D.n_prop;
    for (size_t i = 0; i < BP; ++i)
        if (!(tune[i] > 0) || !std::isfinite(tune[i])) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_set_tuning: tuning parameters must be positive");
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    MHIP_TRY(hipMemcpy(D.tune, tune, sizeof(double) * BP, hipMemcpyHostToDevice));
    return MCD_OK;
}

int mcd_mh_set_temperatures(mcd_mh_t* m, const double* beta)
{
    if (!m || !beta) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_set_temperatures: NULL argument");
    const mcd::MhDev& D = m->dev;
    for (int64_t b = 0; b < D.batch; ++b)
        if (!(beta[b] > 0) || !(beta[b] <= 1.0)) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_set_temperatures: reciprocal temperatures must be in (0, 1]");
    for (int64_t b = 0; b < D.batch && m->ham.h; ++b)
        if (beta[b] != 1.0) return mfail(MCD_ERR_UNSUPPORTED, "mcd_mh_set_temperatures: chain %lld at %g: %s", (long long)b, beta[b], kHamTempered);
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    MHIP_TRY(hipMemcpy(D.beta, beta, sizeof(double) * (size_t)D.batch, hipMemcpyHostToDevice));
    m->dev.lik_only = 0;
    return MCD_OK;
}

// The power posterior prior x likelihood^beta: the same beta array, read by the acceptance ratio's other arm (MhDev::lik_only).
int mcd_mh_set_power(mcd_mh_t* m, const double* beta)
{
    if (!m || !beta) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_set_power: NULL argument");
    if (m->ham.h) return mfail(MCD_ERR_UNSUPPORTED, "mcd_mh_set_power: %s", kHamTempered);
    const mcd::MhDev& D = m->dev;
    if (m->mc3.n_chains != 0)
        return mfail(MCD_ERR_UNSUPPORTED, "mcd_mh_set_power: Metropolis-coupled MCMC is initialised on this handle: its swaps exchange temperatures of (prior x likelihood)^beta");
    for (int64_t b = 0; b < D.batch; ++b)
        if (!(beta[b] >= 0) || !(beta[b] <= 1.0)) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_set_power: the likelihood's exponents must be in [0, 1] (chain %lld: %g)", (long long)b, beta[b]);
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    MHIP_TRY(hipMemcpy(D.beta, beta, sizeof(double) * (size_t)D.batch, hipMemcpyHostToDevice));
    m->dev.lik_only = 1;
    return MCD_OK;
}

int mcd_mh_reset_counters(mcd_mh_t* m)
{
    if (!m) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_reset_counters: NULL handle");
    const mcd::MhDev& D = m->dev;
    const size_t BP = (size_t)D.batch * (size_t)D.n_prop;
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipMemsetAsync(D.acc, 0, sizeof(int32_t) * BP, m->stream));
    MHIP_TRY(hipMemsetAsync(D.tried, 0, sizeof(int32_t) * BP, m->stream));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    return MCD_OK;
}

int mcd_mh_get_age_sums(const mcd_mh_t* cm, double* age_sum, double* age_sq, int64_t* n_samples)
{
    if (!cm) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_get_age_sums: NULL handle");
    const mcd::MhDev& D = cm->dev;
    MHIP_TRY(hipSetDevice(cm->device));
    MHIP_TRY(hipStreamSynchronize(cm->stream));
    const size_t BN = (size_t)D.batch * (size_t)D.n_nodes;
    if (age_sum) MHIP_TRY(hipMemcpy(age_sum, D.age_sum, sizeof(double) * BN, hipMemcpyDeviceToHost));
    if (age_sq) MHIP_TRY(hipMemcpy(age_sq, D.age_sq, sizeof(double) * BN, hipMemcpyDeviceToHost));
    if (n_samples) *n_samples = cm->n_samples;
    return MCD_OK;
}

// ---- the sample recorder: thinned samples of every chain kept on the device while mcd_mh_run runs (mcd::MhRec, mvn_kernels.h) -------
int mcd_mh_record_begin(mcd_mh_t* m, int32_t period, int64_t capacity_samples)
{
    return m ? m->rec.begin("mcd_mh_record_begin", m->rec_on(), period, capacity_samples, 1) : mfail(MCD_ERR_INVALID_ARG, "mcd_mh_record_begin: NULL handle");
}

int mcd_mh_record_count(const mcd_mh_t* m, int64_t* n_samples)
{
    return m && n_samples ? m->rec.count("mcd_mh_record_count", n_samples) : mfail(MCD_ERR_INVALID_ARG, "mcd_mh_record_count: NULL argument");
}

int mcd_mh_record_fetch(mcd_mh_t* m, int64_t max_samples, int64_t* n_out, int64_t* iteration, double* scalars, double* heights, double* rates,
                        double* post, double* beta)
{
    if (!m || !n_out) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_record_fetch: NULL argument");
    return m->rec.fetch("mcd_mh_record_fetch", m->rec_on(), max_samples, n_out, iteration, scalars, heights, rates, post, beta, nullptr);
}

int mcd_mh_record_end(mcd_mh_t* m)
{
    return m ? m->rec.end("mcd_mh_record_end", m->rec_on()) : mfail(MCD_ERR_INVALID_ARG, "mcd_mh_record_end: NULL handle");
}

// ---- summaries of the waiting samples, read in the ring (k_summary.hip) -------------------------------------------------------------------
int mcd_mh_record_quantities(const mcd_mh_t* m, int64_t* q)
{
    if (!m || !q) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_record_quantities: NULL argument");
    *q = 2 * (int64_t)m->dev.n_nodes + 9;
    return MCD_OK;
}

int mcd_mh_record_summary(mcd_mh_t* m, int64_t skip, int64_t n_samples, int32_t max_lag, int64_t* n_used, double* pooled, double* per_chain)
{
    if (!m || !pooled) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_record_summary: NULL argument");
    if (n_used) *n_used = 0;
    const mcd::MhDev& D = m->dev;
    mcd::SumSrc S{};
    int64_t n = 0;
    if (int rc = m->rec.window("mcd_mh_record_summary", m->rec_on(), skip, n_samples, max_lag, &S, &n)) return rc;
    if (m->mc3.n_chains != 0)
        return mfail(MCD_ERR_UNSUPPORTED, "mcd_mh_record_summary: Metropolis-coupled MCMC is initialised on this handle: its temperatures wander between the chains, so a chain is not a cold sequence");
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    std::vector<double> beta((size_t)D.batch);
    MHIP_TRY(hipMemcpy(beta.data(), D.beta, sizeof(double) * beta.size(), hipMemcpyDeviceToHost));
    for (int64_t b = 0; b < D.batch; ++b)
        if (beta[(size_t)b] != 1.0)
            return mfail(MCD_ERR_UNSUPPORTED, "mcd_mh_record_summary: chain %lld has the reciprocal temperature %g: only cold chains (1) are summarised", (long long)b, beta[(size_t)b]);
    if (int rc = mcd_summary_run_(S, max_lag, m->stream, pooled, per_chain)) return rc;
    if (n_used) *n_used = n;
    return MCD_OK;
}

// The marginal likelihood from the window's ln likelihoods, read in the ring (k_marginal.hip): chain g = first_chain + b ran at betas[g mod n_points].
int mcd_mh_record_marginal(mcd_mh_t* m, int n_points, const double* betas, int64_t skip, int64_t n_samples, int64_t* n_used, double* point,
                           double* replicate, double* out)
{
    const char* who = "mcd_mh_record_marginal";
    if (!m || !betas) return mfail(MCD_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (n_used) *n_used = 0;
    const mcd::MhDev& D = m->dev;
    mcd::SumSrc R{};
    int64_t n = 0;
    if (int rc = m->rec.window(who, m->rec_on(), skip, n_samples, 0, &R, &n)) return rc;
    if (int rc = mcd_marginal_check_(who, n, D.batch, D.chain0, n_points, betas)) return rc;
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    // base, n, B, ring, K, then the ring's fields
    const mcd::MlSrc S{R.base, n, D.batch, 1, n_points, R.first, R.cap, R.stride, R.ld};
    if (int rc = mcd_marginal_run_(who, S, betas, m->stream, point, replicate, out)) return rc;
    if (n_used) *n_used = n;
    return MCD_OK;
}

// ... under MC3: the rung's sequence of every group is gathered out of the ring into a plain trace (k_mc3_summary.hip), which then goes
// through the same summary.  Everything the call allocates lives in one block that `Scratch` frees on every way out.
int mcd_mh_record_summary_mc3(mcd_mh_t* m, int rung, int64_t skip, int64_t n_samples, int32_t max_lag, int64_t* n_used, double* pooled,
                              double* per_group, int32_t* holder, int64_t* visits, int64_t* round_trips)
{
    const char* who = "mcd_mh_record_summary_mc3";
    if (!m || !pooled) return mfail(MCD_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (n_used) *n_used = 0;
    const mcd::MhDev& D = m->dev;
    mcd::SumSrc R{};
    int64_t n = 0;
    if (int rc = m->rec.window(who, m->rec_on(), skip, n_samples, max_lag, &R, &n)) return rc;
    const int C = m->mc3.n_chains;
    if (C == 0) return mfail(MCD_ERR_INVALID_ARG, "%s: Metropolis-coupled MCMC is not initialised on this handle (mcd_mh_mc3_init first)", who);
    if (rung < 0 || rung >= C) return mfail(MCD_ERR_INVALID_ARG, "%s: rung %d, the ladder has the rungs 0 .. %d", who, rung, C - 1);
    if (D.chain0 % C != 0 || D.batch % C != 0)
        return mfail(MCD_ERR_UNSUPPORTED, "%s: the handle's chains [%lld, %lld) are not whole groups of %d chains: a group's rung can lie on another handle", who,
                     (long long)D.chain0, (long long)(D.chain0 + D.batch), C);
    const int64_t G = D.batch / C, Q = R.Q, ldq = 8 * ((Q + 7) / 8);
    if (int rc = mcd_summary_check_(who, n, G, Q, max_lag)) return rc;
    const bool flow = visits || round_trips;
    // one block: the trace [n][G][ldq] doubles, visits [batch][C] and round_trips [batch] int64, the error word, holder [n][G] int32
    const size_t n_trace = (size_t)(n * G * ldq), n_flow = flow ? (size_t)(D.batch * (C + 1)) : 0, n_hold = (size_t)(n * G);
    const size_t bytes = 8 * (n_trace + n_flow + 1) + 4 * n_hold;
    struct Scratch {
        void* p = nullptr;
        ~Scratch() { if (p) (void)hipFree(p); }
    } buf;
    MHIP_TRY(hipSetDevice(m->device));
    if (hipError_t e = hipMalloc(&buf.p, bytes)) return mfail(MCD_ERR_HIP, "%s: %zu bytes for the gathered trace: %s", who, bytes, hipGetErrorString(e));
    double* d_trace = (double*)buf.p;
    int64_t* d_visits = (int64_t*)(d_trace + n_trace);
    int64_t* d_trips = d_visits + (flow ? D.batch * C : 0);
    unsigned long long* d_err = (unsigned long long*)(d_visits + n_flow);
    int32_t* d_holder = (int32_t*)(d_err + 1);
    const mcd::Mc3Win W{R.base, n, D.batch, R.first, R.cap, R.stride, R.ld, R.n_nodes, C, m->mc3.ladder};
    unsigned long long err = 0;
    MHIP_TRY(hipMemsetAsync(d_err, 0, sizeof err, m->stream));
    MHIP_TRY(mcd::launch_mc3_gather(W, rung, Q, ldq, d_trace, d_holder, d_err, m->stream));
    if (flow) MHIP_TRY(mcd::launch_mc3_flow(W, d_visits, d_trips, m->stream));
    MHIP_TRY(hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, m->stream));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    if (err != 0) {
        const int64_t p = (int64_t)(err >> 8 & 0xffffffffull);
        return mfail(MCD_ERR_INVALID_ARG, "%s: sample %lld of group %lld has %d chains at rung %d: the window holds samples recorded before mcd_mh_mc3_init or after a mcd_mh_set_temperatures",
                     who, (long long)(p / G), (long long)(p % G), (int)(err & 0xff), rung);
    }
    // base, n, B, Q, ldq, then the ring's fields: a plain trace
    const mcd::SumSrc S{d_trace, n, G, Q, ldq, 0, 0, 0, 0, 0, 0};
    if (int rc = mcd_summary_run_(S, max_lag, m->stream, pooled, per_group)) return rc;
    if (holder) MHIP_TRY(hipMemcpyAsync(holder, d_holder, sizeof(int32_t) * n_hold, hipMemcpyDeviceToHost, m->stream));
    if (visits) MHIP_TRY(hipMemcpyAsync(visits, d_visits, sizeof(int64_t) * (size_t)(D.batch * C), hipMemcpyDeviceToHost, m->stream));
    if (round_trips) MHIP_TRY(hipMemcpyAsync(round_trips, d_trips, sizeof(int64_t) * (size_t)D.batch, hipMemcpyDeviceToHost, m->stream));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    if (n_used) *n_used = n;
    return MCD_OK;
}

// Test hook (tests/test_host.py; no device): the plan of a run under the knobs as they stand, for a handle of these facts -- R > 0: a dense
// likelihood of dimension n in R register blocks, split = 1 where its row-split tables exist, form = the form in force (MCD_FORM_*); R = 0:
// a sparse one of dimension n; the other tables exist, as mcd_tree_create / mcd_sparse_tree_create build them -- and these create-time
// decisions.  Returns the path (MCD_MH_PATH_*; 0: refused) | MhPlan::flags() << 4.
int mcd_mh_plan_selftest_(int n_nodes, int n_prop, int64_t batch, int R, int n, int split, int form, int chain_kernel, int list_all)
{
    MhShape s{n_nodes, n_prop, batch, R > 0, {}, {}, chain_kernel != 0, list_all != 0};
    s.mvn.n = s.sp.n = n;
    s.mvn.R = R;
    s.mvn.form = form;
    s.mvn.split = split != 0;
    s.mvn.wide = s.mvn.cols = true;
    s.sp.rows = s.sp.quad = true;
    const MhPlan p = plan_run(s, mh_options());
    return p.path | p.flags() << 4;
}

int mcd_mh_reset_age_sums(mcd_mh_t* m)
{
    if (!m) return mfail(MCD_ERR_INVALID_ARG, "mcd_mh_reset_age_sums: NULL handle");
    const mcd::MhDev& D = m->dev;
    const size_t BN = (size_t)D.batch * (size_t)D.n_nodes;
    MHIP_TRY(hipSetDevice(m->device));
    MHIP_TRY(hipMemsetAsync(D.age_sum, 0, sizeof(double) * BN, m->stream));
    MHIP_TRY(hipMemsetAsync(D.age_sq, 0, sizeof(double) * BN, m->stream));
    MHIP_TRY(hipStreamSynchronize(m->stream));
    m->n_samples = 0;
    return MCD_OK;
}

}  // extern "C"
