// hmc_capi.cpp -- C ABI of the device leapfrog (include/mcmcdate_mvn.h, "mcd_hmc_*").  The state of `batch` chains, their
// momenta and gradients stay on the device; one leapfrog step = kick, drift (k_hmc.hip), prior gradient (k_prior_grad.hip),
// likelihood gradient (k_tree_grad.hip, or k_sparse_grad.hip over a sparse precision matrix: mcd_hmc_create_sparse).  No CPU path.
// A handle over a small tree may take a whole NUTS transition, or the steps of mcd_hmc_leapfrog, as one launch instead (k_nuts_chain.hip:
// mcd_hmc_set_transition_form).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/mcmcdate_mvn.h"
#include "handover_device.hpp"
#include "host_factor.h"
#include "mvn_kernels.h"
#include "nuts_rhs_plan.hpp"
#include "recorder.hpp"
#include "summary_device.hpp"

int mcd_summary_run_(const mcd::SumSrc& S, int32_t max_lag, hipStream_t st, double* pooled, double* per_chain);   // summary_capi.cpp
extern "C" int mcd_set_last_error_(int code, const char* msg);   // mvn_capi.cpp

namespace {

int hfail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mcd_set_last_error_(code, buf);
}

#define HHIP_TRY(expr)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return hfail(MCD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

}  // namespace

struct mcd_hmc {
    int device = 0;
    const mcd::MvnDev* mvn = nullptr;
    const mcd::TreeDev* tree = nullptr;
    // a likelihood over a SPARSE precision matrix instead (mcd_hmc_create_sparse): mvn and tree stay null
    const mcd::SparseDev* sp = nullptr;
    const mcd::SparseTreeDev* sp_tree = nullptr;
    const mcd::PriorDev* prior = nullptr;
    mcd::HmcDev dev{};
    double *d_eps = nullptr, *d_dir = nullptr, *d_inv_mass = nullptr;
    mcd::NutsDev nuts{};           // allocated by the first NUTS transition (mcd_hmc_nuts)
    int* d_active = nullptr;
    int* d_list = nullptr;         // [batch] the chains still building their trees (across-chains form of a dense metric), with the workspace
    double *d_s1 = nullptr, *d_s2 = nullptr;   // [dim] position moments of one mcd_hmc_nuts_run (k_hmc_moments)
    // the dense metric (mcd_hmc_set_metric): [dim][dim] device buffers behind dev.metric / dev.metric_uinv, allocated by the first
    // metric set; h_metric is the host copy of the stored symmetrised C.  dev.metric == nullptr: the diagonal metric.
    double *d_metric = nullptr, *d_uinv = nullptr;
    mutable std::vector<double> h_metric;
    // where the factors are taken (mcd_hmc_set_metric_factor).  MCD_HMC_FACTOR_DEVICE: k_metric_factor.hip writes S, U and U^-1 into the
    // workspace below ([dim][dim] each, allocated by the first factorisation; d_fc receives a host matrix), and only a factorisation whose
    // status word reports success is copied into d_metric / d_uinv; h_metric is then fetched when somebody asks for it (h_metric_stale)
    int factor = MCD_HMC_FACTOR_HOST;
    double *d_fc = nullptr, *d_fsym = nullptr, *d_fu = nullptr, *d_fw = nullptr;
    unsigned long long* d_fstatus = nullptr;
    mutable bool h_metric_stale = false;
    // the form of the dense metric's products (mcd_hmc_set_metric_form) and, for MCD_HMC_METRIC_ACROSS_CHAINS, the workspace of
    // k_metric_gemm.hip's right-hand sides and products: wx_slots x [batch][dim] each, allocated by the first call that needs them
    int form = MCD_HMC_METRIC_PER_CHAIN;
    mcd::MetricAcross wx{};
    int wx_slots = 0;
    // how a transition is launched (mcd_hmc_set_transition_form): MCD_HMC_TRANSITION_ONE_LAUNCH = k_nuts_chain.hip's one launch per transition
    // and per mcd_hmc_leapfrog, for the handles the setter admits
    int transition = MCD_HMC_TRANSITION_ROUNDS;
    double warmup_phase[4] = {0, 0, 0, 0};     // seconds of the last mcd_hmc_nuts_warmup_dense: factorisations, covariance, window buffer, transitions
    bool have_state = false;
    hipStream_t stream = nullptr;
    const int32_t* host_parent = nullptr;      // [n_nodes] the likelihood handle's host copy of the topology (hand-overs compare it)
    mutable hipEvent_t mark = nullptr;         // what another handle's stream waits for (mcd_hmc_chains_), created on first use
    std::vector<void*> allocs;
    mcd::Recorder rec{"mcd_hmc_record"};       // the sample recorder (mcd_hmc_record_*, recorder.cpp): it counts transitions
    mcd::RecOn rec_on() const { return {device, stream, mcd::MhRecDims{dev.batch, dev.ld, dev.n_nodes}}; }

    ~mcd_hmc()
    {
        (void)hipSetDevice(device);
        for (void* p : allocs) (void)hipFree(p);
        if (mark) (void)hipEventDestroy(mark);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

template <class T>
int halloc(mcd_hmc* m, T** p, size_t count)
{
    *p = nullptr;
    HHIP_TRY(hipMalloc((void**)p, sizeof(T) * (count ? count : 1)));
    m->allocs.push_back(*p);
    HHIP_TRY(hipMemset(*p, 0, sizeof(T) * (count ? count : 1)));
    return MCD_OK;
}

// ln target and its gradient at the current state: two batched gradient launches
int eval_gradients(mcd_hmc* m)
{
    const mcd::HmcDev& D = m->dev;
    const int64_t B = D.batch;
    HHIP_TRY(mcd::launch_prior_grad(*m->prior, D.sc, D.sc + B, D.sc + 2 * B, D.H, D.sc + 3 * B, D.sc + 4 * B, D.R, D.ld, B, D.lp, D.gp_sc,
                                    D.gp_sc + B, D.gp_sc + 2 * B, D.gp_H, D.gp_sc + 3 * B, D.gp_sc + 4 * B, D.gp_R, m->stream));
    if (m->sp)
        HHIP_TRY(mcd::launch_sparse_tree_grad(*m->sp, *m->sp_tree, D.H, D.R, D.ld, D.sc + 2 * B, D.sc + 3 * B, B, D.ll, D.gl_H, D.gl_R, D.gl_tH,
                                              D.gl_rMu, m->stream));
    else
        HHIP_TRY(mcd::launch_tree_grad(*m->mvn, *m->tree, D.H, D.R, D.ld, D.sc + 2 * B, D.sc + 3 * B, B, D.ll, D.gl_H, D.gl_R, D.gl_tH, D.gl_rMu,
                                       m->stream));
    return MCD_OK;
}

// the dense metric's products are taken across the chains (k_metric_gemm.hip)
bool across(const mcd_hmc* m) { return m->dev.metric && m->form == MCD_HMC_METRIC_ACROSS_CHAINS; }

// a transition, and the steps of mcd_hmc_leapfrog, are one launch (k_nuts_chain.hip); the setters keep the across-chains form off such a handle
bool one_launch(const mcd_hmc* m) { return m->transition == MCD_HMC_TRANSITION_ONE_LAUNCH; }

// under the across-chains form the workspace holds `slots` right-hand sides per chain (1: leapfrog steps; kNutsRhsMaxSlots: NUTS).  Called
// by the entry points before their first launch, never inside a round.
int across_alloc(mcd_hmc* m, int slots)
{
    if (!across(m) || m->wx_slots >= slots) return MCD_OK;
    HHIP_TRY(hipStreamSynchronize(m->stream));
    for (double* old : {m->wx.X, m->wx.Y})
        if (old) {
            m->allocs.erase(std::find(m->allocs.begin(), m->allocs.end(), (void*)old));
            (void)hipFree(old);
        }
    m->wx = mcd::MetricAcross{};
    m->wx_slots = 0;
    const size_t count = (size_t)slots * (size_t)m->dev.batch * (size_t)m->dev.dim;
    if (int rc = halloc(m, &m->wx.X, count)) return rc;
    if (int rc = halloc(m, &m->wx.Y, count)) return rc;
    if (!m->d_list)
        if (int rc = halloc(m, &m->d_list, (size_t)m->dev.batch)) return rc;
    m->wx_slots = slots;
    return MCD_OK;
}

// the drift of one leapfrog step under the across-chains form: Y = P C over all chains, then q += eps Y
int drift_across(mcd_hmc* m)
{
    const mcd::HmcDev& D = m->dev;
    HHIP_TRY(mcd::launch_metric_gemm(D.p, D.metric, m->wx.Y, D.batch, D.dim, false, m->stream));
    HHIP_TRY(mcd::launch_hmc_drift_across(D, m->wx.Y, m->stream));
    return MCD_OK;
}

// the largest position a dense metric serves on this handle: the form decides
int dense_max_dim(const mcd_hmc* m) { return m->form == MCD_HMC_METRIC_ACROSS_CHAINS ? MCD_HMC_DENSE_ACROSS_MAX_DIM : MCD_HMC_DENSE_MAX_DIM; }

// the refusal of a position too long for a dense metric in the handle's form
int dense_dim_refused(const mcd_hmc* m, const char* who)
{
    return hfail(MCD_ERR_UNSUPPORTED, "%s: dim = %d, a dense metric serves positions of up to %s = %d coordinates", who, m->dev.dim,
                 m->form == MCD_HMC_METRIC_ACROSS_CHAINS ? "MCD_HMC_DENSE_ACROSS_MAX_DIM" : "MCD_HMC_DENSE_MAX_DIM", dense_max_dim(m));
}

// The metric argument of an entry point: positive inverse masses [dim] -- or NULL while a dense metric is set on the handle, so that
// no caller runs another metric than the one it names.
int check_inv_mass(const mcd_hmc* m, const char* who, const double* inv_mass)
{
    if (m->dev.metric) {
        if (inv_mass) return hfail(MCD_ERR_INVALID_ARG, "%s: a dense metric is set on this handle (mcd_hmc_set_metric): inv_mass must be NULL", who);
        return MCD_OK;
    }
    if (!inv_mass) return hfail(MCD_ERR_INVALID_ARG, "%s: NULL argument", who);
    for (int k = 0; k < m->dev.dim; ++k)
        if (!(inv_mass[k] > 0) || !std::isfinite(inv_mass[k])) return hfail(MCD_ERR_INVALID_ARG, "%s: inverse masses must be positive", who);
    return MCD_OK;
}

// What an entry point hands over besides positions and momenta goes to the device: step sizes, the diagonal metric's inverse masses (a
// dense metric is there already), directions of time (null: forwards; a NUTS transition writes its own)
int upload_step_args(mcd_hmc* m, const double* eps, const double* inv_mass, const double* dir)
{
    HHIP_TRY(hipMemcpyAsync(m->d_eps, eps, sizeof(double) * (size_t)m->dev.batch, hipMemcpyHostToDevice, m->stream));
    if (!m->dev.metric) HHIP_TRY(hipMemcpyAsync(m->d_inv_mass, inv_mass, sizeof(double) * m->dev.dim, hipMemcpyHostToDevice, m->stream));
    if (dir) HHIP_TRY(hipMemcpyAsync(m->d_dir, dir, sizeof(double) * (size_t)m->dev.batch, hipMemcpyHostToDevice, m->stream));
    m->dev.dir = dir ? m->d_dir : nullptr;
    return MCD_OK;
}

// C [dim][dim] as a metric: sym = (C + C^T) / 2, uinv = U^-1 of sym = U U^T (lower triangular).  false, with the reason in `why`: a
// non-finite entry, an asymmetric pair, not positive definite -- the first offender named.
// What a refusal names besides its message (mcd_metric_factor's info): the kind (MCD_METRIC_FACTOR_*) and the offending entry.
struct MetricFault {
    int kind = MCD_METRIC_FACTOR_OK;
    size_t row = 0, col = 0;
};

// the checks of a host matrix that need no factor: every entry finite, a positive diagonal, symmetric pairs
bool metric_checks(int dim, const double* C, char* why, size_t len, MetricFault* fault = nullptr)
{
    const size_t n = (size_t)dim;
    auto refuse = [&](int kind, size_t i, size_t j) {
        if (fault) *fault = MetricFault{kind, i, j};
        return false;
    };
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j)
            if (!std::isfinite(C[i * n + j])) {
                snprintf(why, len, "C[%zu][%zu] = %g is not finite", i, j, C[i * n + j]);
                return refuse(MCD_METRIC_FACTOR_NOT_FINITE, i, j);
            }
    for (size_t i = 0; i < n; ++i)
        if (!(C[i * n + i] > 0.0)) {
            snprintf(why, len, "C is not positive definite: C[%zu][%zu] = %g", i, i, C[i * n + i]);
            return refuse(MCD_METRIC_FACTOR_DIAGONAL, i, i);
        }
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j) {
            const double a = C[i * n + j], b = C[j * n + i];
            if (std::fabs(a - b) > 1e-10 * std::sqrt(C[i * n + i] * C[j * n + j])) {
                snprintf(why, len, "C is not symmetric: C[%zu][%zu] = %.17g, C[%zu][%zu] = %.17g", i, j, a, j, i, b);
                return refuse(MCD_METRIC_FACTOR_ASYMMETRIC, i, j);
            }
        }
    return true;
}

// the refusal of a factorisation that stopped at `piv`, on the host or on the device
void pivot_refused(size_t piv, char* why, size_t len, MetricFault* fault)
{
    snprintf(why, len, "C is not positive definite: the Cholesky factorisation fails at pivot %zu", piv);
    if (fault) *fault = MetricFault{MCD_METRIC_FACTOR_PIVOT, piv, piv};
}

bool metric_factors(int dim, const double* C, std::vector<double>& sym, std::vector<double>& uinv, char* why, size_t len,
                    std::vector<double>* factor = nullptr, MetricFault* fault = nullptr)
{
    const size_t n = (size_t)dim;
    if (!metric_checks(dim, C, why, len, fault)) return false;
    sym.resize(n * n);
    for (size_t i = 0; i < n; ++i) {
        sym[i * n + i] = C[i * n + i];
        for (size_t j = i + 1; j < n; ++j) sym[i * n + j] = sym[j * n + i] = 0.5 * (C[i * n + j] + C[j * n + i]);
    }
    std::vector<double> U;
    if (!mcd::cholesky_lower(dim, sym, U)) {
        size_t piv = 0;                                   // the rows are factored in order: the first row without a diagonal entry failed
        while (piv < n && U[piv * n + piv] > 0.0) ++piv;
        pivot_refused(piv, why, len, fault);
        return false;
    }
    mcd::invert_factor(dim, U, uinv);
    if (factor) factor->swap(U);
    return true;
}

// what k_metric_factor.hip's status word says: true for success; else the message and the offender as the host names them
bool factor_status_ok(unsigned long long st, int dim, char* why, size_t len, MetricFault* fault = nullptr)
{
    if (st == mcd::kMfOk) return true;
    if (st >= mcd::kMfPivot) {
        pivot_refused((size_t)(st - mcd::kMfPivot), why, len, fault);
    } else {
        const size_t i = (size_t)(st / (unsigned long long)dim), j = (size_t)(st % (unsigned long long)dim);
        snprintf(why, len, "C[%zu][%zu] is not finite", i, j);
        if (fault) *fault = MetricFault{MCD_METRIC_FACTOR_NOT_FINITE, i, j};
    }
    return false;
}

// the prepared metric becomes the handle's
int metric_install(mcd_hmc* m, std::vector<double>& sym, const std::vector<double>& uinv)
{
    const size_t nn = (size_t)m->dev.dim * (size_t)m->dev.dim;
    HHIP_TRY(hipSetDevice(m->device));
    if (!m->d_metric) {
        if (int rc = halloc(m, &m->d_metric, nn)) return rc;
        if (int rc = halloc(m, &m->d_uinv, nn)) return rc;
    }
    HHIP_TRY(hipStreamSynchronize(m->stream));
    HHIP_TRY(hipMemcpy(m->d_metric, sym.data(), sizeof(double) * nn, hipMemcpyHostToDevice));
    HHIP_TRY(hipMemcpy(m->d_uinv, uinv.data(), sizeof(double) * nn, hipMemcpyHostToDevice));
    m->h_metric.swap(sym);
    m->h_metric_stale = false;
    m->dev.metric = m->d_metric;
    m->dev.metric_uinv = m->d_uinv;
    return MCD_OK;
}

// The factors of the device matrix d_C (or, d_C == nullptr, of the host matrix h_C uploaded first) into the handle's workspace, on the
// handle's stream (mcd_hmc_set_metric_factor: MCD_HMC_FACTOR_DEVICE); *st = the status word.  The handle's metric is not touched.
int metric_factor_device(mcd_hmc* m, const double* d_C, const double* h_C, bool shrink, double keep, double floor_, unsigned long long* st)
{
    const size_t nn = (size_t)m->dev.dim * (size_t)m->dev.dim;
    HHIP_TRY(hipSetDevice(m->device));
    if (!m->d_fsym) {
        if (int rc = halloc(m, &m->d_fsym, nn)) return rc;
        if (int rc = halloc(m, &m->d_fu, nn)) return rc;
        if (int rc = halloc(m, &m->d_fw, nn)) return rc;
        if (int rc = halloc(m, &m->d_fstatus, 1)) return rc;
    }
    if (!d_C) {
        if (!m->d_fc)
            if (int rc = halloc(m, &m->d_fc, nn)) return rc;
        HHIP_TRY(hipMemcpyAsync(m->d_fc, h_C, sizeof(double) * nn, hipMemcpyHostToDevice, m->stream));
        d_C = m->d_fc;
    }
    HHIP_TRY(mcd::launch_metric_factor(d_C, m->dev.dim, shrink, keep, floor_, m->d_fsym, m->d_fu, m->d_fw, m->d_fstatus, m->stream));
    HHIP_TRY(hipMemcpyAsync(st, m->d_fstatus, sizeof *st, hipMemcpyDeviceToHost, m->stream));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    return MCD_OK;
}

// the workspace's S and U^-1 (a factorisation that reported success) become the handle's
int metric_install_device(mcd_hmc* m)
{
    const size_t nn = (size_t)m->dev.dim * (size_t)m->dev.dim;
    if (!m->d_metric) {
        if (int rc = halloc(m, &m->d_metric, nn)) return rc;
        if (int rc = halloc(m, &m->d_uinv, nn)) return rc;
    }
    HHIP_TRY(hipMemcpyAsync(m->d_metric, m->d_fsym, sizeof(double) * nn, hipMemcpyDeviceToDevice, m->stream));
    HHIP_TRY(hipMemcpyAsync(m->d_uinv, m->d_fw, sizeof(double) * nn, hipMemcpyDeviceToDevice, m->stream));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    m->h_metric.clear();
    m->h_metric_stale = true;
    m->dev.metric = m->d_metric;
    m->dev.metric_uinv = m->d_uinv;
    return MCD_OK;
}

// the host copy of the stored C, fetched when it is asked for after a device factorisation
int metric_host_copy(const mcd_hmc* m)
{
    if (!m->h_metric_stale) return MCD_OK;
    const size_t nn = (size_t)m->dev.dim * (size_t)m->dev.dim;
    HHIP_TRY(hipSetDevice(m->device));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    m->h_metric.resize(nn);
    HHIP_TRY(hipMemcpy(m->h_metric.data(), m->d_metric, sizeof(double) * nn, hipMemcpyDeviceToHost));
    m->h_metric_stale = false;
    return MCD_OK;
}

void metric_clear(mcd_hmc* m)
{
    m->dev.metric = m->dev.metric_uinv = nullptr;
    m->h_metric.clear();
    m->h_metric_stale = false;
}

// the part of mcd_hmc_create / mcd_hmc_create_sparse behind the handles: the likelihood and the prior of `m` are set, `parent` is the host
// copy of the topology of n nodes
int hmc_build(std::unique_ptr<mcd_hmc>& m, int n, int root_right, const int32_t* parent, int calibrations_available, int64_t batch, mcd_hmc_t** out)
{
    // getMask (app/Hamiltonian.hs:33-47) in fold order of the state record, then toVector's reverse order (:49-53)
    std::vector<char> leaf(n, 1);
    for (int v = 1; v < n; ++v) leaf[parent[v]] = 0;
    std::vector<int32_t> field, index;
    auto push = [&](int f, int v) {
        field.push_back(f);
        index.push_back(v);
    };
    push(0, 0);
    push(1, 0);
    if (calibrations_available) push(2, 0);
    for (int v = 1; v < n; ++v)
        if (!leaf[v]) push(3, v);                 // root height and leaf heights are masked
    push(4, 0);
    push(5, 0);
    for (int v = 1; v < n; ++v) push(6, v);       // the stem of the rate tree is masked
    std::vector<int32_t> rf(field.rbegin(), field.rend()), ri(index.rbegin(), index.rend());
    const int dim = (int)rf.size();
    HHIP_TRY(hipSetDevice(m->device));
    HHIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    mcd::HmcDev& D = m->dev;
    m->host_parent = parent;
    D.n_nodes = n;
    D.dim = dim;
    D.root_right = root_right;
    D.batch = batch;
    D.ld = (n + 7) / 8 * 8;
    const size_t B = (size_t)batch, BL = B * (size_t)D.ld, BD = B * (size_t)dim;
    int32_t *pf = nullptr, *pi = nullptr;
    int rc = MCD_OK;
    if ((rc = halloc(m.get(), &pf, (size_t)dim)) || (rc = halloc(m.get(), &pi, (size_t)dim)) || (rc = halloc(m.get(), &D.sc, 5 * B)) ||
        (rc = halloc(m.get(), &D.H, BL)) || (rc = halloc(m.get(), &D.R, BL)) || (rc = halloc(m.get(), &D.lp, B)) ||
        (rc = halloc(m.get(), &D.gp_sc, 5 * B)) || (rc = halloc(m.get(), &D.gp_H, BL)) || (rc = halloc(m.get(), &D.gp_R, BL)) ||
        (rc = halloc(m.get(), &D.ll, B)) || (rc = halloc(m.get(), &D.gl_H, BL)) || (rc = halloc(m.get(), &D.gl_R, BL)) ||
        (rc = halloc(m.get(), &D.gl_tH, B)) || (rc = halloc(m.get(), &D.gl_rMu, B)) || (rc = halloc(m.get(), &D.q, BD)) ||
        (rc = halloc(m.get(), &D.p, BD)) || (rc = halloc(m.get(), &D.grad, BD)) || (rc = halloc(m.get(), &D.value, B)) ||
        (rc = halloc(m.get(), &m->d_eps, B)) || (rc = halloc(m.get(), &m->d_dir, B)) || (rc = halloc(m.get(), &m->d_inv_mass, (size_t)dim)))
        return rc;
    HHIP_TRY(hipMemcpy(pf, rf.data(), sizeof(int32_t) * dim, hipMemcpyHostToDevice));
    HHIP_TRY(hipMemcpy(pi, ri.data(), sizeof(int32_t) * dim, hipMemcpyHostToDevice));
    D.pos_field = pf;
    D.pos_index = pi;
    D.eps = m->d_eps;
    D.dir = m->d_dir;
    D.inv_mass = m->d_inv_mass;
    *out = m.release();
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_hmc_create(mcd_hmc_t** out, const mcd_tree_t* tree, const mcd_prior_t* prior, int calibrations_available, int64_t batch)
{
    if (!out) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create: out is NULL");
    *out = nullptr;
    if (!tree || !prior) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create: NULL tree or prior handle");
    if (batch <= 0) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create: batch must be positive");
    std::unique_ptr<mcd_hmc> m(new mcd_hmc());
    int dev_t = 0, dev_p = 0;
    const int32_t* parent = nullptr;
    const double* host_L = nullptr;
    if (mcd_tree_internal_(tree, &m->mvn, &m->tree, &dev_t, &parent, &host_L) || mcd_prior_internal_(prior, &m->prior, &dev_p))
        return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create: invalid handle");
    if (dev_t != dev_p) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create: tree and prior live on different GPUs");
    const int n = m->tree->n_nodes;
    if (m->prior->n_nodes != n) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create: tree has %d nodes, prior %d", n, m->prior->n_nodes);
    m->device = dev_t;
    return hmc_build(m, n, m->tree->root_right, parent, calibrations_available, batch, out);
}

// The same driver over a likelihood whose precision matrix stays sparse on the device (mcd_sparse_tree_create): the likelihood gradient is
// k_sparse_grad.hip's one launch, everything else is shared.
int mcd_hmc_create_sparse(mcd_hmc_t** out, const mcd_sparse_tree_t* tree, const mcd_prior_t* prior, int calibrations_available, int64_t batch)
{
    if (!out) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create_sparse: out is NULL");
    *out = nullptr;
    if (!tree || !prior) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create_sparse: NULL tree or prior handle");
    if (batch <= 0 || batch > 0x7fffffffLL) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create_sparse: batch must be in [1, 2^31)");
    std::unique_ptr<mcd_hmc> m(new mcd_hmc());
    int dev_t = 0, dev_p = 0;
    const int32_t* parent = nullptr;
    if (mcd_sparse_tree_grad_internal_(tree, &m->sp, &m->sp_tree, &dev_t, &parent) || mcd_prior_internal_(prior, &m->prior, &dev_p))
        return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create_sparse: invalid handle");
    const int n = m->sp_tree->n_nodes;
    if (n < 3 || n > mcd::kSparseGradMaxNodes || n > mcd::kPriorGradMaxNodes)
        return hfail(MCD_ERR_UNSUPPORTED, "mcd_hmc_create_sparse: %d nodes (the sparse driver serves trees of 3 .. %d nodes)", n, mcd::kSparseGradMaxNodes);
    if (!mcd::sparse_tree_grad_available(mcd::SparseFacts(*m->sp), n))
        return hfail(MCD_ERR_UNSUPPORTED, "mcd_hmc_create_sparse: the handle has no rows of the symmetric part");
    if (dev_t != dev_p) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create_sparse: tree and prior live on different GPUs");
    if (m->prior->n_nodes != n) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_create_sparse: tree has %d nodes, prior %d", n, m->prior->n_nodes);
    m->device = dev_t;
    return hmc_build(m, n, m->sp_tree->root_right, parent, calibrations_available, batch, out);
}

void mcd_hmc_destroy(mcd_hmc_t* m) { delete m; }

int mcd_hmc_dim(const mcd_hmc_t* m) { return m ? m->dev.dim : hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_dim: NULL handle"); }

int mcd_hmc_set_state(mcd_hmc_t* m, const double* birth, const double* death, const double* tH, const double* heights,
                      const double* rMu, const double* rVar, const double* rates, int64_t ld_state)
{
    if (!m || !birth || !death || !tH || !heights || !rMu || !rVar || !rates) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_state: NULL argument");
    mcd::HmcDev& D = m->dev;
    if (ld_state < D.n_nodes) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_state: ld_state < n_nodes");
    HHIP_TRY(hipSetDevice(m->device));
    const size_t B = (size_t)D.batch;
    const double* src[5] = {birth, death, tH, rMu, rVar};
    for (int i = 0; i < 5; ++i) HHIP_TRY(hipMemcpyAsync(D.sc + i * B, src[i], sizeof(double) * B, hipMemcpyHostToDevice, m->stream));
    HHIP_TRY(hipMemcpy2DAsync(D.H, sizeof(double) * D.ld, heights, sizeof(double) * ld_state, sizeof(double) * D.n_nodes, B, hipMemcpyHostToDevice, m->stream));
    HHIP_TRY(hipMemcpy2DAsync(D.R, sizeof(double) * D.ld, rates, sizeof(double) * ld_state, sizeof(double) * D.n_nodes, B, hipMemcpyHostToDevice, m->stream));
    if (int rc = eval_gradients(m)) return rc;
    HHIP_TRY(mcd::launch_hmc_collect(D, m->stream));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    m->have_state = true;
    return MCD_OK;
}

int mcd_hmc_get_state(const mcd_hmc_t* cm, double* birth, double* death, double* tH, double* heights, double* rMu, double* rVar,
                      double* rates, int64_t ld_state)
{
    if (!cm || !birth || !death || !tH || !heights || !rMu || !rVar || !rates) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_get_state: NULL argument");
    const mcd::HmcDev& D = cm->dev;
    if (ld_state < D.n_nodes) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_get_state: ld_state < n_nodes");
    HHIP_TRY(hipSetDevice(cm->device));
    HHIP_TRY(hipStreamSynchronize(cm->stream));
    const size_t B = (size_t)D.batch;
    double* dst[5] = {birth, death, tH, rMu, rVar};
    for (int i = 0; i < 5; ++i) HHIP_TRY(hipMemcpy(dst[i], D.sc + i * B, sizeof(double) * B, hipMemcpyDeviceToHost));
    HHIP_TRY(hipMemcpy2D(heights, sizeof(double) * ld_state, D.H, sizeof(double) * D.ld, sizeof(double) * D.n_nodes, B, hipMemcpyDeviceToHost));
    HHIP_TRY(hipMemcpy2D(rates, sizeof(double) * ld_state, D.R, sizeof(double) * D.ld, sizeof(double) * D.n_nodes, B, hipMemcpyDeviceToHost));
    return MCD_OK;
}

int mcd_hmc_get_position(const mcd_hmc_t* cm, double* q, double* value, double* grad)
{
    if (!cm) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_get_position: NULL handle");
    if (!cm->have_state) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_get_position: call mcd_hmc_set_state first");
    const mcd::HmcDev& D = cm->dev;
    HHIP_TRY(hipSetDevice(cm->device));
    HHIP_TRY(hipStreamSynchronize(cm->stream));
    const size_t B = (size_t)D.batch, BD = B * (size_t)D.dim;
    if (q) HHIP_TRY(hipMemcpy(q, D.q, sizeof(double) * BD, hipMemcpyDeviceToHost));
    if (value) HHIP_TRY(hipMemcpy(value, D.value, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (grad) HHIP_TRY(hipMemcpy(grad, D.grad, sizeof(double) * BD, hipMemcpyDeviceToHost));
    return MCD_OK;
}

int mcd_hmc_leapfrog(mcd_hmc_t* m, double* p, const double* eps, const double* dir, const double* inv_mass, int n_steps)
{
    if (!m || !p || !eps) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_leapfrog: NULL argument");
    if (!m->have_state) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_leapfrog: call mcd_hmc_set_state first");
    if (n_steps < 0) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_leapfrog: negative number of steps");
    mcd::HmcDev& D = m->dev;
    const size_t B = (size_t)D.batch, BD = B * (size_t)D.dim;
    if (int rc = check_inv_mass(m, "mcd_hmc_leapfrog", inv_mass)) return rc;
    HHIP_TRY(hipSetDevice(m->device));
    if (int rc = across_alloc(m, 1)) return rc;
    HHIP_TRY(hipMemcpyAsync(D.p, p, sizeof(double) * BD, hipMemcpyHostToDevice, m->stream));
    if (int rc = upload_step_args(m, eps, inv_mass, dir)) return rc;
    if (one_launch(m)) {                                  // the same sequence inside one launch, a workgroup per chain
        HHIP_TRY(mcd::launch_leapfrog_chain(D, *m->mvn, *m->tree, *m->prior, n_steps, m->stream));
        HHIP_TRY(hipMemcpyAsync(p, D.p, sizeof(double) * BD, hipMemcpyDeviceToHost, m->stream));
        HHIP_TRY(hipStreamSynchronize(m->stream));
        return MCD_OK;
    }
    // p += eps/2 g;  [ q += eps Minv p;  g = grad(q);  p += eps g ] x (n - 1);  q += eps Minv p;  g = grad(q);  p += eps/2 g
    // three launches per step (kick + drift fused, prior gradient, likelihood gradient), the closing half kick with the collect
    // (across-chains form of a dense metric: the kick, the product over all chains, the drift)
    for (int s = 0; s < n_steps; ++s) {
        if (across(m)) {
            HHIP_TRY(mcd::launch_hmc_kick(D, (s == 0) ? 0.5 : 1.0, 0, m->stream));
            if (int rc = drift_across(m)) return rc;
        } else {
            HHIP_TRY(mcd::launch_hmc_kick_drift(D, (s == 0) ? 0.5 : 1.0, m->stream));
        }
        if (int rc = eval_gradients(m)) return rc;
    }
    if (n_steps > 0)
        HHIP_TRY(mcd::launch_hmc_kick_collect(D, 0.5, m->stream));
    else
        HHIP_TRY(mcd::launch_hmc_collect(D, m->stream));
    HHIP_TRY(hipMemcpyAsync(p, D.p, sizeof(double) * BD, hipMemcpyDeviceToHost, m->stream));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    return MCD_OK;
}

int mcd_hmc_step_from(mcd_hmc_t* m, double* q, double* p, double* grad, int have_grad, const double* eps, const double* dir,
                      const double* inv_mass, double* value)
{
    if (!m || !q || !p || !grad || !eps) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_step_from: NULL argument");
    if (!m->have_state) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_step_from: call mcd_hmc_set_state first (fixes the masked entries)");
    mcd::HmcDev& D = m->dev;
    const size_t B = (size_t)D.batch, BD = B * (size_t)D.dim;
    if (int rc = check_inv_mass(m, "mcd_hmc_step_from", inv_mass)) return rc;
    HHIP_TRY(hipSetDevice(m->device));
    if (int rc = across_alloc(m, 1)) return rc;
    HHIP_TRY(hipMemcpyAsync(D.q, q, sizeof(double) * BD, hipMemcpyHostToDevice, m->stream));
    HHIP_TRY(hipMemcpyAsync(D.p, p, sizeof(double) * BD, hipMemcpyHostToDevice, m->stream));
    if (int rc = upload_step_args(m, eps, inv_mass, dir)) return rc;
    HHIP_TRY(mcd::launch_hmc_scatter(D, m->stream));
    if (have_grad) {
        HHIP_TRY(hipMemcpyAsync(D.grad, grad, sizeof(double) * BD, hipMemcpyHostToDevice, m->stream));
    } else {
        if (int rc = eval_gradients(m)) return rc;
    }
    HHIP_TRY(mcd::launch_hmc_kick(D, 0.5, have_grad ? 1 : 0, m->stream));
    if (across(m)) {
        if (int rc = drift_across(m)) return rc;
    } else {
        HHIP_TRY(mcd::launch_hmc_drift(D, m->stream));
    }
    if (int rc = eval_gradients(m)) return rc;
    HHIP_TRY(mcd::launch_hmc_kick(D, 0.5, 0, m->stream));
    HHIP_TRY(mcd::launch_hmc_collect(D, m->stream));
    HHIP_TRY(hipMemcpyAsync(q, D.q, sizeof(double) * BD, hipMemcpyDeviceToHost, m->stream));
    HHIP_TRY(hipMemcpyAsync(p, D.p, sizeof(double) * BD, hipMemcpyDeviceToHost, m->stream));
    HHIP_TRY(hipMemcpyAsync(grad, D.grad, sizeof(double) * BD, hipMemcpyDeviceToHost, m->stream));
    if (value) HHIP_TRY(hipMemcpyAsync(value, D.value, sizeof(double) * B, hipMemcpyDeviceToHost, m->stream));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    return MCD_OK;
}

}  // extern "C"

// ---- NUTS (k_nuts.hip) ------------------------------------------------------------------------------------------------
namespace {

constexpr int kNutsMaxDepth = 12;
static_assert(mcd::kHmcDenseMaxDim == MCD_HMC_DENSE_MAX_DIM, "the kernels' bound is the header's");
static_assert(mcd::kNutsMaxDepthLevels == kNutsMaxDepth, "the right-hand-side plan's depth is the driver's");
static_assert(MCD_HMC_DENSE_ACROSS_MAX_DIM >= 2 * mcd::kSparseGradMaxNodes + 2, "every dim a handle can have");

int nuts_alloc(mcd_hmc* m)
{
    if (m->nuts.qm) return MCD_OK;
    const mcd::HmcDev& D = m->dev;
    const size_t B = (size_t)D.batch, BD = B * (size_t)D.dim;
    mcd::NutsDev& N = m->nuts;
    N.max_depth = kNutsMaxDepth;
    int rc = MCD_OK;
    double** pd[] = {&N.qm, &N.pm, &N.gm, &N.qp, &N.pp, &N.gp, &N.qc, &N.gc, &N.qn, &N.gn};
    for (double** p : pd)
        if ((rc = halloc(m, p, BD))) return rc;
    if ((rc = halloc(m, &N.sq, BD * kNutsMaxDepth)) || (rc = halloc(m, &N.sp, BD * kNutsMaxDepth))) return rc;
    double** pb[] = {&N.lpc, &N.lpn, &N.log_u, &N.joint0, &N.alpha};
    for (double** p : pb)
        if ((rc = halloc(m, p, B))) return rc;
    int** pi[] = {&N.j, &N.v, &N.i, &N.n, &N.n1, &N.s1, &N.done, &N.n_alpha, &N.depth, &N.leaf, &N.diverged};
    for (int** p : pi)
        if ((rc = halloc(m, p, B))) return rc;
    if ((rc = halloc(m, &m->d_s1, (size_t)D.dim)) || (rc = halloc(m, &m->d_s2, (size_t)D.dim))) return rc;
    return halloc(m, &m->d_active, 1);
}

// The end of a round of tree building: the counter is cleared, the round's last kernel counts the chains that go on, the host reads the counter
template <class Launch>
int nuts_round_end(mcd_hmc* m, int* active, Launch launch_round_kernel)
{
    HHIP_TRY(hipMemsetAsync(m->d_active, 0, sizeof(int), m->stream));
    HHIP_TRY(launch_round_kernel());
    HHIP_TRY(hipMemcpyAsync(active, m->d_active, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    return MCD_OK;
}

// The tree building of one transition under the across-chains form of a dense metric (k_nuts_across.hip has the sequence): the chains are
// in lock step, so round r is leaf i of doubling j for every chain still building (nuts_round_position) and the number of products it
// needs is known here (nuts_rhs_plan).  The counter the host polls after every round is the number of chains that go on, and the kernel
// that counts them lists them: the products multiply the listed chains' rows only.
int nuts_build_across(mcd_hmc* m, int max_depth, uint64_t seed, int64_t chain0, uint64_t transition)
{
    const mcd::HmcDev& D = m->dev;
    const mcd::MetricAcross& W = m->wx;
    const int64_t B = D.batch;
    HHIP_TRY(mcd::launch_nutsx_draw(D, W.X, seed, chain0, transition, m->stream));
    HHIP_TRY(mcd::launch_metric_gemm(W.X, D.metric_uinv, W.Y, B, D.dim, true, m->stream));        // P = U^-T z
    HHIP_TRY(mcd::launch_metric_gemm(W.Y, D.metric, W.X, B, D.dim, false, m->stream));            // CP
    HHIP_TRY(mcd::launch_nutsx_begin(D, m->nuts, W.Y, W.X, seed, chain0, transition, m->stream));
    HHIP_TRY(mcd::launch_metric_gemm(D.p, D.metric, W.Y, B, D.dim, false, m->stream));
    HHIP_TRY(mcd::launch_nutsx_drift(D, m->nuts, W.Y, m->stream));
    const int64_t max_rounds = (int64_t)1 << max_depth;
    const int* list = nullptr;                                        // every chain in round 0
    int n = (int)B;
    for (int64_t r = 0; r < max_rounds; ++r) {
        int j = 0, i = 0;
        mcd::nuts_round_position(r, &j, &i);
        const mcd::NutsRhsPlan plan = mcd::nuts_rhs_plan(j, i);
        if (int rc = eval_gradients(m)) return rc;
        HHIP_TRY(mcd::launch_nutsx_leaf(D, m->nuts, W.X, m->stream));                                          // (a)
        HHIP_TRY(mcd::launch_metric_gemm_rows(W.X, D.metric, W.Y, (int64_t)plan.count * n, D.dim, false, list, n, B, m->stream));   // (b)
        int active = 0;
        auto book = [&] { return mcd::launch_nutsx_book(D, m->nuts, W.Y, seed, chain0, transition, max_depth, m->d_active, m->d_list, m->stream); };   // (c)
        if (int rc = nuts_round_end(m, &active, book)) return rc;
        if (active == 0) break;
        list = m->d_list;
        n = active;
        HHIP_TRY(mcd::launch_metric_gemm_rows(D.p, D.metric, W.Y, n, D.dim, false, list, n, B, m->stream));    // (d)
        HHIP_TRY(mcd::launch_nutsx_drift(D, m->nuts, W.Y, m->stream));                                          // (e)
    }
    return MCD_OK;
}

// the per-chain kernels: diagonal metric, or a dense one in the per-chain form
int nuts_build(mcd_hmc* m, int max_depth, uint64_t seed, int64_t chain0, uint64_t transition)
{
    const mcd::HmcDev& D = m->dev;
    HHIP_TRY(mcd::launch_nuts_begin(D, m->nuts, seed, chain0, transition, m->stream));
    const int64_t max_rounds = (int64_t)1 << max_depth;               // 2^max_depth - 1 leaves at most
    for (int64_t r = 0; r < max_rounds; ++r) {
        if (int rc = eval_gradients(m)) return rc;
        int active = 0;
        auto step = [&] { return mcd::launch_nuts_step(D, m->nuts, seed, chain0, transition, max_depth, m->d_active, m->stream); };
        if (int rc = nuts_round_end(m, &active, step)) return rc;
        if (active == 0) break;
    }
    return MCD_OK;
}

// one transition for every chain; eps and inv_mass already on the device
int nuts_transition(mcd_hmc* m, int max_depth, uint64_t seed, int64_t chain0, uint64_t transition)
{
    mcd::HmcDev& D = m->dev;
    D.dir = m->d_dir;
    if (one_launch(m)) {
        // everything below up to the recorder's store as ONE launch: no counter is polled, the gradient kernels' raw outputs are the
        // accepted point's when it ends
        HHIP_TRY(mcd::launch_nuts_chain(D, m->nuts, *m->mvn, *m->tree, *m->prior, seed, chain0, transition, max_depth, m->d_active, m->stream));
        if (m->rec.step()) HHIP_TRY(mcd::launch_hmc_record(D, m->nuts, m->rec.view(), m->rec.counts().taken(), m->stream));
        return MCD_OK;
    }
    if (int rc = across(m) ? nuts_build_across(m, max_depth, seed, chain0, transition) : nuts_build(m, max_depth, seed, chain0, transition)) return rc;
    HHIP_TRY(mcd::launch_nuts_end(D, m->nuts, m->stream));
    // k_nuts_end put the accepted point into D.q / D.grad / D.value and the state arrays, but the raw outputs of the gradient
    // kernels still belong to the LAST LEAF evaluated (another point, possibly outside the support).  mcd_hmc_leapfrog's first
    // half kick reads those raw outputs: evaluate them at the accepted point so that every entry point may follow a transition.
    if (int rc = eval_gradients(m)) return rc;
    HHIP_TRY(mcd::launch_hmc_collect(D, m->stream));
    // the sample recorder: D.lp / D.ll are the accepted point's now, D.eps the step sizes the transition used
    if (m->rec.step()) HHIP_TRY(mcd::launch_hmc_record(D, m->nuts, m->rec.view(), m->rec.counts().taken(), m->stream));
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_hmc_nuts(mcd_hmc_t* m, const double* eps, const double* inv_mass, int max_depth, uint64_t seed, int64_t chain_offset,
                 uint64_t transition, double* alpha, int32_t* depth)
{
    if (!m || !eps) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts: NULL argument");
    if (!m->have_state) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts: call mcd_hmc_set_state first");
    if (max_depth < 1 || max_depth > kNutsMaxDepth) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts: max_depth must be 1 .. %d", kNutsMaxDepth);
    mcd::HmcDev& D = m->dev;
    const size_t B = (size_t)D.batch;
    if (int rc = check_inv_mass(m, "mcd_hmc_nuts", inv_mass)) return rc;
    for (size_t b = 0; b < B; ++b)
        if (!(eps[b] > 0) || !std::isfinite(eps[b])) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts: step sizes must be positive");
    if (int rc = m->rec.room("mcd_hmc_nuts", 1)) return rc;
    HHIP_TRY(hipSetDevice(m->device));
    if (int rc = nuts_alloc(m)) return rc;
    if (int rc = across_alloc(m, mcd::kNutsRhsMaxSlots)) return rc;
    if (int rc = upload_step_args(m, eps, inv_mass, nullptr)) return rc;
    if (int rc = nuts_transition(m, max_depth, seed, chain_offset, transition)) return rc;
    std::vector<double> a(B);
    std::vector<int> na(B), dp(B);
    HHIP_TRY(hipMemcpyAsync(a.data(), m->nuts.alpha, sizeof(double) * B, hipMemcpyDeviceToHost, m->stream));
    HHIP_TRY(hipMemcpyAsync(na.data(), m->nuts.n_alpha, sizeof(int) * B, hipMemcpyDeviceToHost, m->stream));
    HHIP_TRY(hipMemcpyAsync(dp.data(), m->nuts.depth, sizeof(int) * B, hipMemcpyDeviceToHost, m->stream));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    for (size_t b = 0; b < B; ++b) {
        if (alpha) alpha[b] = a[b] / (double)(na[b] > 0 ? na[b] : 1);
        if (depth) depth[b] = dp[b];
    }
    return MCD_OK;
}

}  // extern "C"

// ---- the chains of a Metropolis-Hastings handle become this handle's, on the device (handover_device.hpp, k_handover.hip) -----------
namespace {

mcd::ChainArrays arrays_of(const mcd_hmc* h) { return {h->dev.sc, h->dev.H, h->dev.R, h->dev.ld}; }

// h := the chains at src once `ready` has passed on the source's stream: what mcd_hmc_set_state does behind its copies.  No host wait.
int take_chains(mcd_hmc* h, const mcd::ChainArrays& src, hipEvent_t ready)
{
    const mcd::HmcDev& D = h->dev;
    if (ready) HHIP_TRY(hipStreamWaitEvent(h->stream, ready, 0));
    HHIP_TRY(mcd::launch_handover(arrays_of(h), src, D.batch, D.n_nodes, h->stream));
    if (int rc = eval_gradients(h)) return rc;
    HHIP_TRY(mcd::launch_hmc_collect(D, h->stream));
    h->have_state = true;
    return MCD_OK;
}

}  // namespace

int mcd_hmc_chains_(const mcd_hmc* h, mcd::ChainsView* v, hipEvent_t* mark)
{
    if (!h || !v) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_chains_: NULL argument");
    *v = mcd::ChainsView{h->device, h->stream, h->dev.n_nodes, h->dev.batch, h->host_parent, h->have_state, arrays_of(h)};
    if (mark) {
        HHIP_TRY(hipSetDevice(h->device));
        if (!h->mark) HHIP_TRY(hipEventCreateWithFlags(&h->mark, hipEventDisableTiming));
        HHIP_TRY(hipEventRecord(h->mark, h->stream));
        *mark = h->mark;
    }
    return MCD_OK;
}

int mcd_hmc_cycle_ready_(mcd_hmc* h, const char* who, bool dense)
{
    if (h->rec.active())
        return hfail(MCD_ERR_INVALID_ARG, "%s: the attached mcd_hmc_t has an active recorder (mcd_hmc_record_end first): the cycle's samples are the mcd_mh_t's", who);
    if (dense && !h->dev.metric)
        return hfail(MCD_ERR_INVALID_ARG, "%s: the attachment names the dense metric of the mcd_hmc_t (inv_mass == NULL), which has none set (mcd_hmc_set_metric)", who);
    if (!dense && h->dev.metric)
        return hfail(MCD_ERR_INVALID_ARG, "%s: a dense metric is set on the attached mcd_hmc_t (mcd_hmc_set_metric): the attachment's inv_mass must be NULL", who);
    HHIP_TRY(hipSetDevice(h->device));
    if (int rc = nuts_alloc(h)) return rc;
    if (int rc = across_alloc(h, mcd::kNutsRhsMaxSlots)) return rc;
    return MCD_OK;
}

int mcd_hmc_cycle_transition_(mcd_hmc* h, const mcd::ChainArrays& src, hipEvent_t ready, const double* d_eps, const double* d_inv_mass, int max_depth,
                              uint64_t seed, int64_t chain0, uint64_t transition, const mcd::HamSums& sums, hipEvent_t* done)
{
    // the kernels read step sizes and inverse masses through HmcDev: for this transition the attachment's arrays, then the handle's own again
    mcd::HmcDev& D = h->dev;
    D.eps = d_eps;
    if (d_inv_mass) D.inv_mass = d_inv_mass;
    int rc = take_chains(h, src, ready);
    if (!rc) rc = nuts_transition(h, max_depth, seed, chain0, transition);
    if (!rc && mcd::launch_ham_stats(h->nuts, sums, D.batch, h->stream) != hipSuccess) rc = hfail(MCD_ERR_HIP, "mcd_mh_run: the attached transition's diagnostics could not be launched");
    D.eps = h->d_eps;
    D.inv_mass = h->d_inv_mass;
    if (rc) return rc;
    mcd::ChainsView v;
    return mcd_hmc_chains_(h, &v, done);
}

extern "C" {

// h := the current states of m (include/mcmcdate_mvn.h): mcd_hmc_set_state after mcd_mh_get_state, without the host in between
int mcd_hmc_take_state(mcd_hmc_t* h, const mcd_mh_t* m)
{
    if (!h || !m) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_take_state: NULL handle");
    mcd::ChainsView dst, src;
    if (int rc = mcd_hmc_chains_(h, &dst, nullptr)) return rc;
    if (int rc = mcd_mh_chains_(m, &src, nullptr)) return rc;
    char why[256];
    if (!mcd::handover_allowed(dst, src, why, sizeof why)) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_take_state: %s", why);
    hipEvent_t ready = nullptr;
    if (int rc = mcd_mh_chains_(m, &src, &ready)) return rc;
    HHIP_TRY(hipSetDevice(h->device));
    if (int rc = take_chains(h, src.a, ready)) return rc;
    HHIP_TRY(hipStreamSynchronize(h->stream));
    return MCD_OK;
}

}  // extern "C"

namespace {

// mcd_hmc_nuts_run; q_store (device, [n_transitions][batch][dim], or null) receives the positions after every transition
int nuts_run(mcd_hmc_t* m, int n_transitions, int adapt, double* eps, const double* inv_mass, double delta, int max_depth, uint64_t seed,
             int64_t chain_offset, uint64_t first_transition, double* mean_alpha, double* q_mean, double* q_var, double* q_store)
{
    if (!m || !eps) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_run: NULL argument");
    if (int rc = check_inv_mass(m, "mcd_hmc_nuts_run", inv_mass)) return rc;
    if (n_transitions < 0) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_run: negative number of transitions");
    if (adapt && !(delta > 0 && delta < 1)) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_run: delta must be in (0, 1)");
    if (int rc = m->rec.room("mcd_hmc_nuts_run", n_transitions)) return rc;
    const mcd::HmcDev& D = m->dev;
    const size_t B = (size_t)D.batch, dim = (size_t)D.dim;
    // dual averaging of ln eps per chain: Hoffman & Gelman (2014), Algorithm 6 (gamma = 0.05, t0 = 10, kappa = 0.75)
    const double gamma = 0.05, t0 = 10.0, kappa = 0.75;
    std::vector<double> mu(B), h_bar(B, 0.0), log_eps_bar(B, 0.0), cur(eps, eps + B), alpha(B), asum(B, 0.0);
    for (size_t b = 0; b < B; ++b) mu[b] = std::log(10.0 * eps[b]);
    // the position moments are summed on the device after every transition (k_hmc_moments: the order of the host loop this replaces,
    // chains in order inside a transition, transitions in order) and read once at the end
    const bool moments = q_mean || q_var;
    std::vector<double> s1(dim, 0.0), s2(dim, 0.0);
    for (int t = 1; t <= n_transitions; ++t) {
        if (int rc = mcd_hmc_nuts(m, cur.data(), inv_mass, max_depth, seed, chain_offset, first_transition + (uint64_t)(t - 1), alpha.data(), nullptr))
            return rc;
        for (size_t b = 0; b < B; ++b) {
            asum[b] += alpha[b];
            if (adapt) {
                h_bar[b] = (1.0 - 1.0 / (t + t0)) * h_bar[b] + (delta - alpha[b]) / (t + t0);
                const double log_eps = mu[b] - std::sqrt((double)t) / gamma * h_bar[b];
                const double w = std::pow((double)t, -kappa);
                log_eps_bar[b] = w * log_eps + (1.0 - w) * log_eps_bar[b];
                cur[b] = std::exp(log_eps);
            }
        }
        if (moments) {
            if (t == 1) {                                        // (the first transition has allocated them)
                HHIP_TRY(hipMemsetAsync(m->d_s1, 0, sizeof(double) * dim, m->stream));
                HHIP_TRY(hipMemsetAsync(m->d_s2, 0, sizeof(double) * dim, m->stream));
            }
            HHIP_TRY(mcd::launch_hmc_moments(D, m->d_s1, m->d_s2, m->stream));
        }
        if (q_store) HHIP_TRY(hipMemcpyAsync(q_store + (size_t)(t - 1) * B * dim, D.q, sizeof(double) * B * dim, hipMemcpyDeviceToDevice, m->stream));
    }
    if (moments && n_transitions > 0) {
        HHIP_TRY(hipMemcpyAsync(s1.data(), m->d_s1, sizeof(double) * dim, hipMemcpyDeviceToHost, m->stream));
        HHIP_TRY(hipMemcpyAsync(s2.data(), m->d_s2, sizeof(double) * dim, hipMemcpyDeviceToHost, m->stream));
        HHIP_TRY(hipStreamSynchronize(m->stream));
    }
    for (size_t b = 0; b < B; ++b) {
        if (adapt && n_transitions > 0) eps[b] = std::exp(log_eps_bar[b]);
        if (mean_alpha) mean_alpha[b] = n_transitions > 0 ? asum[b] / n_transitions : 0.0;
    }
    const double cnt = (double)B * (double)(n_transitions > 0 ? n_transitions : 1);
    for (size_t k = 0; k < dim && moments; ++k) {
        const double mean = s1[k] / cnt;
        if (q_mean) q_mean[k] = mean;
        if (q_var) q_var[k] = s2[k] / cnt - mean * mean;          // pooled over chains and transitions (what mass tuning uses)
    }
    return MCD_OK;
}

// Both warm-ups shrink a window's (co)variances towards 1e-3 (Stan's regularisation): keep * v, + floor on the diagonal, n_eff positions
constexpr double shrink_keep(double n_eff) { return n_eff / (n_eff + 5.0); }
constexpr double shrink_floor(double n_eff) { return 1e-3 * (5.0 / (n_eff + 5.0)); }

// device memory of one call
struct Scratch {
    double* p = nullptr;
    ~Scratch() { (void)hipFree(p); }
};

}  // namespace

extern "C" {

int mcd_hmc_nuts_run(mcd_hmc_t* m, int n_transitions, int adapt, double* eps, const double* inv_mass, double delta, int max_depth,
                     uint64_t seed, int64_t chain_offset, uint64_t first_transition, double* mean_alpha, double* q_mean, double* q_var)
{
    return nuts_run(m, n_transitions, adapt, eps, inv_mass, delta, max_depth, seed, chain_offset, first_transition, mean_alpha, q_mean, q_var, nullptr);
}

int mcd_hmc_set_metric(mcd_hmc_t* m, const double* inv_mass_dense)
{
    if (!m) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_metric: NULL handle");
    if (!inv_mass_dense) {
        metric_clear(m);
        return MCD_OK;
    }
    if (m->dev.dim > dense_max_dim(m)) return dense_dim_refused(m, "mcd_hmc_set_metric");
    std::vector<double> sym, uinv;
    char why[256];
    if (m->factor == MCD_HMC_FACTOR_DEVICE) {
        if (!metric_checks(m->dev.dim, inv_mass_dense, why, sizeof why)) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_metric: %s", why);
        unsigned long long st = 0;
        if (int rc = metric_factor_device(m, nullptr, inv_mass_dense, false, 1.0, 0.0, &st)) return rc;
        if (!factor_status_ok(st, m->dev.dim, why, sizeof why)) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_metric: %s", why);
        return metric_install_device(m);
    }
    if (!metric_factors(m->dev.dim, inv_mass_dense, sym, uinv, why, sizeof why)) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_metric: %s", why);
    return metric_install(m, sym, uinv);
}

int mcd_hmc_set_metric_form(mcd_hmc_t* m, int form)
{
    if (!m) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_metric_form: NULL handle");
    if (form != MCD_HMC_METRIC_PER_CHAIN && form != MCD_HMC_METRIC_ACROSS_CHAINS)
        return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_metric_form: form = %d is neither MCD_HMC_METRIC_PER_CHAIN nor MCD_HMC_METRIC_ACROSS_CHAINS", form);
    if (m->dev.metric)
        return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_metric_form: a dense metric is set on this handle: clear it first (mcd_hmc_set_metric(NULL))");
    if (form == MCD_HMC_METRIC_ACROSS_CHAINS && one_launch(m))
        return hfail(MCD_ERR_UNSUPPORTED,
                     "mcd_hmc_set_metric_form: the handle's transitions are one launch (MCD_HMC_TRANSITION_ONE_LAUNCH), which takes a dense metric's "
                     "products per chain only: MCD_HMC_METRIC_ACROSS_CHAINS is refused (mcd_hmc_set_transition_form(MCD_HMC_TRANSITION_ROUNDS) first)");
    m->form = form;
    return MCD_OK;
}

int mcd_hmc_set_transition_form(mcd_hmc_t* m, int form)
{
    if (!m) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_transition_form: NULL handle");
    if (form != MCD_HMC_TRANSITION_ROUNDS && form != MCD_HMC_TRANSITION_ONE_LAUNCH)
        return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_transition_form: form = %d is neither MCD_HMC_TRANSITION_ROUNDS nor MCD_HMC_TRANSITION_ONE_LAUNCH", form);
    if (form == MCD_HMC_TRANSITION_ONE_LAUNCH) {
        if (m->sp)
            return hfail(MCD_ERR_UNSUPPORTED,
                         "mcd_hmc_set_transition_form: the handle's likelihood is sparse (mcd_hmc_create_sparse, %d distances): one launch per "
                         "transition serves dense likelihoods of up to %d distances",
                         m->sp->n, 64);
        if (m->mvn->R != 1 || !mcd::nuts_chain_available(*m->mvn, *m->tree, *m->prior))
            return hfail(MCD_ERR_UNSUPPORTED,
                         "mcd_hmc_set_transition_form: the likelihood has %d distances (a tree of %d nodes): one launch per transition serves up to "
                         "%d distances (%d nodes), one 64-row block of the factor",
                         m->mvn->n, m->dev.n_nodes, 64, mcd::kNutsChainMaxNodes);
        if (m->form == MCD_HMC_METRIC_ACROSS_CHAINS)
            return hfail(MCD_ERR_UNSUPPORTED,
                         "mcd_hmc_set_transition_form: the handle takes a dense metric's products across the chains (MCD_HMC_METRIC_ACROSS_CHAINS); "
                         "one launch per transition takes them per chain only (mcd_hmc_set_metric_form(MCD_HMC_METRIC_PER_CHAIN) first)");
    }
    m->transition = form;
    return MCD_OK;
}

int mcd_hmc_get_transition_form(const mcd_hmc_t* m, int* form)
{
    if (!m || !form) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_get_transition_form: NULL argument");
    *form = m->transition;
    return MCD_OK;
}

int mcd_hmc_set_metric_factor(mcd_hmc_t* m, int where)
{
    if (!m) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_metric_factor: NULL handle");
    if (where != MCD_HMC_FACTOR_HOST && where != MCD_HMC_FACTOR_DEVICE)
        return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_set_metric_factor: where = %d is neither MCD_HMC_FACTOR_HOST nor MCD_HMC_FACTOR_DEVICE", where);
    m->factor = where;
    return MCD_OK;
}

int mcd_hmc_get_metric_factor(const mcd_hmc_t* m, int* where)
{
    if (!m || !where) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_get_metric_factor: NULL argument");
    *where = m->factor;
    return MCD_OK;
}

int mcd_hmc_get_metric_form(const mcd_hmc_t* m, int* form)
{
    if (!m || !form) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_get_metric_form: NULL argument");
    *form = m->form;
    return MCD_OK;
}

int mcd_hmc_get_metric(const mcd_hmc_t* m, int* is_dense, double* inv_mass_dense)
{
    if (!m || !is_dense) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_get_metric: NULL argument");
    *is_dense = m->dev.metric ? 1 : 0;
    if (m->dev.metric && inv_mass_dense) {
        if (int rc = metric_host_copy(m)) return rc;
        std::copy(m->h_metric.begin(), m->h_metric.end(), inv_mass_dense);
    }
    return MCD_OK;
}

// the handle's U^-1 [dim][dim] as the kernels read it, copied to the host (tests; not part of the public header)
int mcd_hmc_metric_uinv_(const mcd_hmc_t* m, double* out)
{
    if (!m || !out) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_metric_uinv_: NULL argument");
    if (!m->dev.metric) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_metric_uinv_: no dense metric is set on this handle");
    HHIP_TRY(hipSetDevice(m->device));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    HHIP_TRY(hipMemcpy(out, m->d_uinv, sizeof(double) * (size_t)m->dev.dim * (size_t)m->dev.dim, hipMemcpyDeviceToHost));
    return MCD_OK;
}

// mcd_hmc_nuts_warmup with the FULL covariance of the window's positions as the inverse mass matrix (k_hmc_cov.hip), the same shrinkage
// (its diagonal is the rule below) and the same rule for a window that cannot be used.
int mcd_hmc_nuts_warmup_dense(mcd_hmc_t* m, int windows, int window, double* eps, const double* inv_mass0, double delta, int max_depth,
                              uint64_t seed, int64_t chain_offset, uint64_t first_transition, double* mean_alpha, double* inv_mass_dense_out)
{
    if (!m || !eps || !inv_mass0) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_warmup_dense: NULL argument");
    if (windows < 1 || window < 1) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_warmup_dense: need windows >= 1 and window >= 1");
    const size_t B = (size_t)m->dev.batch, dim = (size_t)m->dev.dim;
    if (m->dev.dim > dense_max_dim(m)) return dense_dim_refused(m, "mcd_hmc_nuts_warmup_dense");
    for (size_t k = 0; k < dim; ++k)
        if (!(inv_mass0[k] > 0) || !std::isfinite(inv_mass0[k])) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_warmup_dense: inverse masses must be positive");
    if (int rc = m->rec.room("mcd_hmc_nuts_warmup_dense", ((int64_t)windows + 1) * (int64_t)window)) return rc;
    metric_clear(m);
    HHIP_TRY(hipSetDevice(m->device));
    // where the call's time goes (mcd_hmc_warmup_phases_): 0 factorisations (host, + upload; or on the device), 1 covariance, 2 window
    // buffer, 3 transitions
    const bool on_device = m->factor == MCD_HMC_FACTOR_DEVICE;
    using clk = std::chrono::steady_clock;
    double* phase = m->warmup_phase;
    std::fill(phase, phase + 4, 0.0);
    auto since = [](clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); };
    clk::time_point t0 = clk::now();
    const size_t n = B * (size_t)window;
    Scratch Q, mom;                                                   // [window][batch][dim] positions; [dim] means + [dim][dim] covariance
    HHIP_TRY(hipMalloc((void**)&Q.p, sizeof(double) * n * dim));
    HHIP_TRY(hipMalloc((void**)&mom.p, sizeof(double) * (dim + dim * dim)));
    phase[2] += since(t0);
    std::vector<double> alpha(B), cov(on_device ? 0 : dim * dim), sym, uinv;
    char why[256];
    uint64_t t = first_transition;
    for (int w = 0; w < windows; ++w) {
        if (int rc = nuts_run(m, window, 1, eps, m->dev.metric ? nullptr : inv_mass0, delta, max_depth, seed, chain_offset, t, alpha.data(), nullptr,
                              nullptr, Q.p))
            return rc;
        HHIP_TRY(hipStreamSynchronize(m->stream));
        phase[3] += since(t0);
        t0 = clk::now();
        t += (uint64_t)window;
        HHIP_TRY(mcd::launch_hmc_cov(Q.p, (int64_t)n, (int)dim, mom.p, mom.p + dim, m->stream));
        if (!on_device) HHIP_TRY(hipMemcpyAsync(cov.data(), mom.p + dim, sizeof(double) * dim * dim, hipMemcpyDeviceToHost, m->stream));
        HHIP_TRY(hipStreamSynchronize(m->stream));
        phase[1] += since(t0);
        t0 = clk::now();
        const double keep = shrink_keep((double)n), floor_ = shrink_floor((double)n);
        if (on_device) {                                              // shrinkage, symmetric part, factors: the matrix stays on the device
            unsigned long long st = 0;
            if (int rc = metric_factor_device(m, mom.p + dim, nullptr, true, keep, floor_, &st)) return rc;
            if (st == mcd::kMfOk)                                     // the rule below: a window without a factor keeps the metric
                if (int rc = metric_install_device(m)) return rc;
            phase[0] += since(t0);
            t0 = clk::now();
            continue;
        }
        for (size_t i = 0; i < dim; ++i)
            for (size_t j = 0; j < dim; ++j) cov[i * dim + j] = keep * cov[i * dim + j] + (i == j ? floor_ : 0.0);
        // a chain outside the support leaves NaN positions, a degenerate window no factor: keep the metric
        if (metric_factors((int)dim, cov.data(), sym, uinv, why, sizeof why))
            if (int rc = metric_install(m, sym, uinv)) return rc;
        phase[0] += since(t0);
        t0 = clk::now();
    }
    if (!m->dev.metric) {                                             // no window could be used: the starting masses as the dense metric
        cov.assign(dim * dim, 0.0);
        for (size_t k = 0; k < dim; ++k) cov[k * dim + k] = inv_mass0[k];
        if (on_device) {
            unsigned long long st = 0;
            if (int rc = metric_factor_device(m, nullptr, cov.data(), false, 1.0, 0.0, &st)) return rc;
            if (!factor_status_ok(st, (int)dim, why, sizeof why)) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_warmup_dense: %s", why);
            if (int rc = metric_install_device(m)) return rc;
        } else {
            if (!metric_factors((int)dim, cov.data(), sym, uinv, why, sizeof why)) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_warmup_dense: %s", why);
            if (int rc = metric_install(m, sym, uinv)) return rc;
        }
        phase[0] += since(t0);
        t0 = clk::now();
    }
    if (int rc = nuts_run(m, window, 1, eps, nullptr, delta, max_depth, seed, chain_offset, t, alpha.data(), nullptr, nullptr, nullptr)) return rc;
    HHIP_TRY(hipStreamSynchronize(m->stream));
    phase[3] += since(t0);
    if (mean_alpha) std::copy(alpha.begin(), alpha.end(), mean_alpha);
    if (inv_mass_dense_out) {
        if (int rc = metric_host_copy(m)) return rc;
        std::copy(m->h_metric.begin(), m->h_metric.end(), inv_mass_dense_out);
    }
    return MCD_OK;
}

// The factors of a dense metric on host arrays, without a handle: where = MCD_HMC_FACTOR_HOST runs metric_factors above (no device is
// touched), MCD_HMC_FACTOR_DEVICE the kernels of k_metric_factor.hip on device_id.
int mcd_metric_factor(int dim, const double* C, int where, int device_id, double* sym_out, double* U_out, double* Uinv_out, int64_t* info)
{
    auto report = [&](const MetricFault& f) {
        if (info) {
            info[0] = f.kind;
            info[1] = (int64_t)f.row;
            info[2] = (int64_t)f.col;
        }
    };
    report(MetricFault{});
    if (dim < 1 || !C) return hfail(MCD_ERR_INVALID_ARG, "mcd_metric_factor: need dim >= 1 and a matrix");
    if (where != MCD_HMC_FACTOR_HOST && where != MCD_HMC_FACTOR_DEVICE)
        return hfail(MCD_ERR_INVALID_ARG, "mcd_metric_factor: where = %d is neither MCD_HMC_FACTOR_HOST nor MCD_HMC_FACTOR_DEVICE", where);
    if (dim > MCD_HMC_DENSE_ACROSS_MAX_DIM)
        return hfail(MCD_ERR_UNSUPPORTED, "mcd_metric_factor: dim = %d, a dense metric serves positions of up to MCD_HMC_DENSE_ACROSS_MAX_DIM = %d coordinates",
                     dim, MCD_HMC_DENSE_ACROSS_MAX_DIM);
    const size_t nn = (size_t)dim * (size_t)dim;
    char why[256];
    MetricFault fault;
    if (where == MCD_HMC_FACTOR_HOST) {
        std::vector<double> sym, uinv, U;
        if (!metric_factors(dim, C, sym, uinv, why, sizeof why, &U, &fault)) {
            report(fault);
            return hfail(MCD_ERR_INVALID_ARG, "mcd_metric_factor: %s", why);
        }
        if (sym_out) std::copy(sym.begin(), sym.end(), sym_out);
        if (U_out) std::copy(U.begin(), U.end(), U_out);
        if (Uinv_out) std::copy(uinv.begin(), uinv.end(), Uinv_out);
        return MCD_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return hfail(MCD_ERR_NO_DEVICE, "mcd_metric_factor: no HIP device (MCD_HMC_FACTOR_DEVICE has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return hfail(MCD_ERR_INVALID_ARG, "mcd_metric_factor: device %d of %d", device_id, ndev);
    if (!metric_checks(dim, C, why, sizeof why, &fault)) {
        report(fault);
        return hfail(MCD_ERR_INVALID_ARG, "mcd_metric_factor: %s", why);
    }
    HHIP_TRY(hipSetDevice(device_id));
    struct Arena {
        hipStream_t st = nullptr;
        Scratch c, s, u, w, status;
        ~Arena()
        {
            if (st) (void)hipStreamDestroy(st);
        }
    } A;
    HHIP_TRY(hipStreamCreate(&A.st));
    for (Scratch* b : {&A.c, &A.s, &A.u, &A.w}) HHIP_TRY(hipMalloc((void**)&b->p, sizeof(double) * nn));
    HHIP_TRY(hipMalloc((void**)&A.status.p, sizeof(unsigned long long)));
    unsigned long long st = 0;
    HHIP_TRY(hipMemcpyAsync(A.c.p, C, sizeof(double) * nn, hipMemcpyHostToDevice, A.st));
    HHIP_TRY(mcd::launch_metric_factor(A.c.p, dim, false, 1.0, 0.0, A.s.p, A.u.p, A.w.p, (unsigned long long*)A.status.p, A.st));
    HHIP_TRY(hipMemcpyAsync(&st, A.status.p, sizeof st, hipMemcpyDeviceToHost, A.st));
    HHIP_TRY(hipStreamSynchronize(A.st));
    if (!factor_status_ok(st, dim, why, sizeof why, &fault)) {
        report(fault);
        return hfail(MCD_ERR_INVALID_ARG, "mcd_metric_factor: %s", why);
    }
    if (sym_out) HHIP_TRY(hipMemcpy(sym_out, A.s.p, sizeof(double) * nn, hipMemcpyDeviceToHost));
    if (U_out) HHIP_TRY(hipMemcpy(U_out, A.u.p, sizeof(double) * nn, hipMemcpyDeviceToHost));
    if (Uinv_out) HHIP_TRY(hipMemcpy(Uinv_out, A.w.p, sizeof(double) * nn, hipMemcpyDeviceToHost));
    return MCD_OK;
}

namespace {

// device buffers of one of the two entries below, each of exactly the size asked for
struct TestArena {
    hipStream_t st = nullptr;
    std::vector<void*> bufs;
    ~TestArena()
    {
        for (void* p : bufs) (void)hipFree(p);
        if (st) (void)hipStreamDestroy(st);
    }
    hipError_t upload(void** d, const void* h, size_t bytes)           // h == nullptr: allocate only
    {
        if (hipError_t e = hipMalloc(d, bytes)) return e;
        bufs.push_back(*d);
        return h ? hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    }
};

int test_device(const char* who, int device_id)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return hfail(MCD_ERR_NO_DEVICE, "%s: no HIP device", who);
    if (device_id < 0 || device_id >= ndev) return hfail(MCD_ERR_INVALID_ARG, "%s: device %d of %d", who, device_id, ndev);
    return MCD_OK;
}

}  // namespace

// launch_metric_gemm_rows (k_metric_gemm.hip) on host arrays: X [mem_rows][dim], A [dim][dim], the current contents of Y [mem_rows][dim]
// and the list [n_list] (or NULL) go to device buffers of exactly these sizes, the launcher runs unchanged, Y comes back.  A list entry
// or a mapped row outside mem_rows is refused before anything is launched (tests; not part of the public header)
int mcd_metric_gemm_(const double* X, const double* A, double* Y, int64_t mem_rows, int dim, int lower, const int* list, int n_list, int64_t stride,
                     int64_t rows, int device_id)
{
    const char* who = "mcd_metric_gemm_";
    if (!X || !A || !Y) return hfail(MCD_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (mem_rows < 1 || dim < 1 || rows < 0) return hfail(MCD_ERR_INVALID_ARG, "%s: need mem_rows >= 1, dim >= 1 and rows >= 0", who);
    if (list) {
        if (n_list < 1 || stride < 0) return hfail(MCD_ERR_INVALID_ARG, "%s: a list needs n_list >= 1 and stride >= 0", who);
        for (int k = 0; k < n_list; ++k)
            if (list[k] < 0 || list[k] >= mem_rows) return hfail(MCD_ERR_INVALID_ARG, "%s: list[%d] = %d is no row of %lld", who, k, list[k], (long long)mem_rows);
        for (int64_t r = 0; r < rows; ++r) {
            const int64_t slot = r / n_list;
            if (slot > 0 && stride > (mem_rows - 1 - list[r % n_list]) / slot)      // slot stride + list[..] > mem_rows - 1, without overflow
                return hfail(MCD_ERR_INVALID_ARG, "%s: product row %lld is memory row %lld x %lld + %d, outside %lld rows", who, (long long)r,
                             (long long)slot, (long long)stride, list[r % n_list], (long long)mem_rows);
        }
    } else if (rows > mem_rows) {
        return hfail(MCD_ERR_INVALID_ARG, "%s: %lld rows of %lld", who, (long long)rows, (long long)mem_rows);
    }
    if (int rc = test_device(who, device_id)) return rc;
    HHIP_TRY(hipSetDevice(device_id));
    TestArena T;
    HHIP_TRY(hipStreamCreate(&T.st));
    const size_t nx = (size_t)mem_rows * (size_t)dim;
    double *dX = nullptr, *dA = nullptr, *dY = nullptr;
    int* dlist = nullptr;
    HHIP_TRY(T.upload((void**)&dX, X, sizeof(double) * nx));
    HHIP_TRY(T.upload((void**)&dA, A, sizeof(double) * (size_t)dim * (size_t)dim));
    HHIP_TRY(T.upload((void**)&dY, Y, sizeof(double) * nx));
    if (list) HHIP_TRY(T.upload((void**)&dlist, list, sizeof(int) * (size_t)n_list));
    HHIP_TRY(mcd::launch_metric_gemm_rows(dX, dA, dY, rows, dim, lower != 0, dlist, list ? n_list : 0, list ? stride : 0, T.st));
    HHIP_TRY(hipMemcpyAsync(Y, dY, sizeof(double) * nx, hipMemcpyDeviceToHost, T.st));
    HHIP_TRY(hipStreamSynchronize(T.st));
    return MCD_OK;
}

// launch_hmc_cov (k_hmc_cov.hip) on the host array Q [n][dim]: mean_out [dim], cov_out [dim][dim] (tests; not part of the public header)
int mcd_hmc_cov_(const double* Q, int64_t n, int dim, double* mean_out, double* cov_out, int device_id)
{
    const char* who = "mcd_hmc_cov_";
    if (!Q || !mean_out || !cov_out) return hfail(MCD_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (n < 1 || dim < 1) return hfail(MCD_ERR_INVALID_ARG, "%s: need n >= 1 and dim >= 1", who);
    if (int rc = test_device(who, device_id)) return rc;
    HHIP_TRY(hipSetDevice(device_id));
    TestArena T;
    HHIP_TRY(hipStreamCreate(&T.st));
    const size_t nn = (size_t)dim * (size_t)dim;
    double *dQ = nullptr, *dmean = nullptr, *dcov = nullptr;
    HHIP_TRY(T.upload((void**)&dQ, Q, sizeof(double) * (size_t)n * (size_t)dim));
    HHIP_TRY(T.upload((void**)&dmean, nullptr, sizeof(double) * (size_t)dim));
    HHIP_TRY(T.upload((void**)&dcov, nullptr, sizeof(double) * nn));
    HHIP_TRY(mcd::launch_hmc_cov(dQ, n, dim, dmean, dcov, T.st));
    HHIP_TRY(hipMemcpyAsync(mean_out, dmean, sizeof(double) * (size_t)dim, hipMemcpyDeviceToHost, T.st));
    HHIP_TRY(hipMemcpyAsync(cov_out, dcov, sizeof(double) * nn, hipMemcpyDeviceToHost, T.st));
    HHIP_TRY(hipStreamSynchronize(T.st));
    return MCD_OK;
}

// seconds the last mcd_hmc_nuts_warmup_dense of this handle spent in its four phases: the factorisations (on the host with their upload,
// or on the device: mcd_hmc_set_metric_factor), the window
// covariance (kernel + copy), the window buffer's allocation, the transitions (tools/bench_nuts.py; not part of the public header)
int mcd_hmc_warmup_phases_(const mcd_hmc_t* m, double* seconds)
{
    if (!m || !seconds) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_warmup_phases_: NULL argument");
    std::copy(m->warmup_phase, m->warmup_phase + 4, seconds);
    return MCD_OK;
}

// Host-only self test of the right-hand-side plan of the across-chains NUTS (nuts_rhs_plan.hpp; tests/test_nuts_rhs_plan_host.py, no GPU):
// walks every leaf of every doubling j < depth as k_nuts_step does -- level k closes at leaf i when (i + 1) % 2^k == 0 and i % 2^k != 0,
// the whole tree's test follows leaf 2^j - 1 -- and compares count, slots and the round's (j, i) with the plan.  Returns the number of
// rounds checked (2^depth - 1), < 0 for the first kind of disagreement.  out[0 .. 2]: rounds, the largest count, the sum of all counts.
int mcd_nuts_rhs_plan_selftest_(int depth, int64_t* out)
{
    if (depth < 1 || depth > mcd::kNutsMaxDepthLevels) return -1;
    int64_t r = 0, total = 0;
    int largest = 0;
    for (int j = 0; j < depth; ++j)
        for (int i = 0; i < (1 << j); ++i, ++r) {
            int jr = -1, ir = -1;
            mcd::nuts_round_position(r, &jr, &ir);
            if (jr != j || ir != i) return -2;
            const mcd::NutsRhsPlan p = mcd::nuts_rhs_plan(j, i);
            int closes = 0;
            for (int k = 1; k <= j; ++k) {
                const int size = 1 << k;
                const bool opens = i % size == 0, closing = (i + 1) % size == 0;
                if (opens && closing) return -3;
                if (closing) {
                    if (k != closes + 1) return -4;               // the closed levels are 1 .. closes, in the order of the slots
                    ++closes;
                }
            }
            const int whole = (i + 1 == (1 << j)) ? 1 : 0;
            if (p.closes != closes || p.whole != whole || p.count != 1 + closes + whole) return -5;
            if (p.count < 1 || p.count > mcd::kNutsRhsMaxSlots) return -6;
            largest = std::max(largest, p.count);
            total += p.count;
        }
    if (r != ((int64_t)1 << depth) - 1) return -7;
    if (out) {
        out[0] = r;
        out[1] = largest;
        out[2] = total;
    }
    return (int)r;
}

// Step sizes AND masses: the reference tunes both (`HTuningConf HTuneLeapfrog HTuneAllMasses`, app/Hamiltonian.hs:62-63; the
// schedule of the package `mcmc` is not restated).  `windows` windows of `window` transitions: dual averaging of the step sizes
// inside a window (mcd_hmc_nuts_run, adapt = 1), then the inverse masses become the pooled variance of the positions the
// window visited, shrunk towards 1e-3 (Stan's regularisation); a closing window adapts the step sizes to the final masses.
int mcd_hmc_nuts_warmup(mcd_hmc_t* m, int windows, int window, double* eps, double* inv_mass, double delta, int max_depth, uint64_t seed,
                        int64_t chain_offset, uint64_t first_transition, double* mean_alpha)
{
    if (!m || !eps || !inv_mass) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_warmup: NULL argument");
    if (windows < 0 || window < 1) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_nuts_warmup: need windows >= 0 and window >= 1");
    if (int rc = m->rec.room("mcd_hmc_nuts_warmup", ((int64_t)windows + 1) * (int64_t)window)) return rc;
    const size_t B = (size_t)m->dev.batch, dim = (size_t)m->dev.dim;
    std::vector<double> qv(dim), alpha(B);
    uint64_t t = first_transition;
    for (int w = 0; w < windows; ++w) {
        if (int rc = mcd_hmc_nuts_run(m, window, 1, eps, inv_mass, delta, max_depth, seed, chain_offset, t, alpha.data(), nullptr, qv.data())) return rc;
        t += (uint64_t)window;
        const double n_eff = (double)B * (double)window;
        for (size_t k = 0; k < dim; ++k) {
            const double v = shrink_keep(n_eff) * qv[k] + shrink_floor(n_eff);
            inv_mass[k] = (v > 0 && std::isfinite(v)) ? v : inv_mass[k];      // a chain outside the support leaves NaN positions: keep the mass
        }
    }
    if (int rc = mcd_hmc_nuts_run(m, window, 1, eps, inv_mass, delta, max_depth, seed, chain_offset, t, alpha.data(), nullptr, nullptr)) return rc;
    if (mean_alpha) std::copy(alpha.begin(), alpha.end(), mean_alpha);
    return MCD_OK;
}

// ---- the sample recorder: thinned samples and the transitions' diagnostics kept on the device (k_hmc_record.hip; host side: recorder.cpp) ----
int mcd_hmc_record_begin(mcd_hmc_t* m, int32_t period, int64_t capacity_samples)
{
    return m ? m->rec.begin("mcd_hmc_record_begin", m->rec_on(), period, capacity_samples, mcd::kHmcRecDiag) : hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_record_begin: NULL handle");
}

int mcd_hmc_record_count(const mcd_hmc_t* m, int64_t* n_samples)
{
    return m && n_samples ? m->rec.count("mcd_hmc_record_count", n_samples) : hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_record_count: NULL argument");
}

int mcd_hmc_record_fetch(mcd_hmc_t* m, int64_t max_samples, int64_t* n_out, int64_t* transition, double* scalars, double* heights, double* rates,
                         double* post, double* nuts)
{
    if (!m || !n_out) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_record_fetch: NULL argument");
    return m->rec.fetch("mcd_hmc_record_fetch", m->rec_on(), max_samples, n_out, transition, scalars, heights, rates, post, nullptr, nuts);
}

int mcd_hmc_record_end(mcd_hmc_t* m)
{
    return m ? m->rec.end("mcd_hmc_record_end", m->rec_on()) : hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_record_end: NULL handle");
}

int mcd_hmc_record_quantities(const mcd_hmc_t* m, int64_t* q)
{
    if (!m || !q) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_record_quantities: NULL argument");
    *q = 2 * (int64_t)m->dev.n_nodes + 9;
    return MCD_OK;
}

int mcd_hmc_record_summary(mcd_hmc_t* m, int64_t skip, int64_t n_samples, int32_t max_lag, int64_t* n_used, double* pooled, double* per_chain,
                           double* nuts_stats)
{
    if (!m || !pooled) return hfail(MCD_ERR_INVALID_ARG, "mcd_hmc_record_summary: NULL argument");
    if (n_used) *n_used = 0;
    const mcd::HmcDev& D = m->dev;
    mcd::SumSrc S{};
    int64_t n = 0;
    if (int rc = m->rec.window("mcd_hmc_record_summary", m->rec_on(), skip, n_samples, max_lag, &S, &n)) return rc;
    HHIP_TRY(hipSetDevice(m->device));
    HHIP_TRY(hipStreamSynchronize(m->stream));
    if (int rc = mcd_summary_run_(S, max_lag, m->stream, pooled, per_chain)) return rc;
    if (nuts_stats) {
        double* d_stats = nullptr;
        HHIP_TRY(hipMalloc((void**)&d_stats, sizeof(double) * 4 * (size_t)D.batch));
        hipError_t e = mcd::launch_hmc_record_stats(m->rec_on().dims, m->rec.view(), S.first, n, d_stats, m->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nuts_stats, d_stats, sizeof(double) * 4 * (size_t)D.batch, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
        (void)hipFree(d_stats);
        if (e != hipSuccess) return hfail(MCD_ERR_HIP, "mcd_hmc_record_summary: diagnostics: %s", hipGetErrorString(e));
    }
    if (n_used) *n_used = n;
    return MCD_OK;
}

}  // extern "C"
