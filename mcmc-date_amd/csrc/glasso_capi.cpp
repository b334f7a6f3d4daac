// glasso_capi.cpp -- the C ABI of the device graphical lasso (include/mcmcdate_mvn.h: mcd_glasso, mcd_glasso_components) on top of
// k_glasso.hip.  Replaces: the glasso call of `prepare` (app/Main.hs:257-276) for the sparse likelihood at the reference's production
// tree sizes; prepare.graphical_lasso stays the host statement of the same algorithm.  No CPU fallback.
//
// Exact screening (Witten, Friedman, Simon 2011; Mazumder, Hastie 2012): the connected components of the graph {i != j : |S_ij| > rho} are
// the blocks of the optimal Theta; between blocks Theta and W are 0.  Every component of two or more variables is one independent problem
// (one workgroup of k_glasso_pass), a singleton is closed-form.  The host launches one outer pass at a time and applies
// prepare.graphical_lasso's stopping rule to the largest change of W over all problems.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/mcmcdate_mvn.h"
#include "glasso_device.hpp"

extern "C" int mcd_set_last_error_(int code, const char* msg);

static_assert(MCD_GLASSO_MAX_DIM == mcd::kGlassoMaxDim, "the header states the kernel's limit");

namespace {

int gfail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mcd_set_last_error_(code, buf);
}

#define GHIP_TRY(expr)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return gfail(MCD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

// device buffers and the stream of one call
struct Arena {
    hipStream_t st = nullptr;
    std::vector<void*> bufs;
    ~Arena()
    {
        for (void* p : bufs) (void)hipFree(p);
        if (st) (void)hipStreamDestroy(st);
    }
    template <class T>
    hipError_t alloc(T** out, size_t count)
    {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, sizeof(T) * (count ? count : 1));
        if (e == hipSuccess) bufs.push_back(p);
        *out = (T*)p;
        return e;
    }
};

// label[i] = component of variable i in the graph {i != j : |S_ij| > rho or |S_ji| > rho}, numbered by the smallest member (breadth first)
int components(int n, const double* S, double rho, int32_t* label)
{
    std::fill(label, label + n, (int32_t)-1);
    std::vector<int> queue((size_t)n);
    int nc = 0;
    for (int r = 0; r < n; ++r) {
        if (label[r] >= 0) continue;
        size_t head = 0, tail = 0;
        queue[tail++] = r;
        label[r] = nc;
        while (head < tail) {
            const int i = queue[head++];
            for (int j = 0; j < n; ++j)
                if (label[j] < 0 && (std::fabs(S[(size_t)i * n + j]) > rho || std::fabs(S[(size_t)j * n + i]) > rho)) {
                    label[j] = nc;
                    queue[tail++] = j;
                }
        }
        ++nc;
    }
    return nc;
}

int check_matrix(const char* who, int n, const double* S, double rho)
{
    if (n < 1) return gfail(MCD_ERR_INVALID_ARG, "%s: n = %d, must be at least 1", who, n);
    if (!S) return gfail(MCD_ERR_INVALID_ARG, "%s: S is NULL", who);
    if (!(rho >= 0.0) || !std::isfinite(rho)) return gfail(MCD_ERR_INVALID_ARG, "%s: the penalty rho = %g must be finite and not negative", who, rho);
    for (size_t e = 0; e < (size_t)n * n; ++e)
        if (!std::isfinite(S[e])) return gfail(MCD_ERR_INVALID_ARG, "%s: S[%zu][%zu] is not finite", who, e / n, e % n);
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_glasso_components(int n, const double* S, double rho, int32_t* label, int32_t* n_components)
{
    if (const int rc = check_matrix("mcd_glasso_components", n, S, rho)) return rc;
    if (!label || !n_components) return gfail(MCD_ERR_INVALID_ARG, "mcd_glasso_components: NULL output");
    *n_components = components(n, S, rho, label);
    return MCD_OK;
}

int mcd_glasso(int n, const double* S, double rho, int penalize_diagonal, double tol, int max_iter, int device_id, double* W, double* Theta,
               int64_t* info)
{
    if (const int rc = check_matrix("mcd_glasso", n, S, rho)) return rc;
    if (!W || !Theta || !info) return gfail(MCD_ERR_INVALID_ARG, "mcd_glasso: NULL output");
    if (!(tol >= 0.0)) return gfail(MCD_ERR_INVALID_ARG, "mcd_glasso: tol = %g is negative or not a number", tol);
    if (max_iter < 1) return gfail(MCD_ERR_INVALID_ARG, "mcd_glasso: max_iter = %d, must be at least 1", max_iter);
    const size_t N = (size_t)n;
    double off_sum = 0.0;
    for (size_t i = 0; i < N; ++i) {
        if (!(S[i * N + i] > 0.0)) return gfail(MCD_ERR_INVALID_ARG, "mcd_glasso: S[%zu][%zu] = %g, the diagonal must be positive", i, i, S[i * N + i]);
        for (size_t j = 0; j < N; ++j) {
            if (j == i) continue;
            const double a = S[i * N + j], b = S[j * N + i];
            if (std::fabs(a - b) > MCD_GLASSO_SYMMETRY_TOL * std::max(1.0, std::max(std::fabs(a), std::fabs(b))))
                return gfail(MCD_ERR_INVALID_ARG, "mcd_glasso: S is not symmetric: S[%zu][%zu] = %.17g, S[%zu][%zu] = %.17g", i, j, a, j, i, b);
            off_sum += std::fabs(a);
        }
    }
    std::fill(info, info + MCD_GLASSO_INFO_LEN, (int64_t)0);
    // exact screening
    std::vector<int32_t> label(N);
    const int nc = components(n, S, rho, label.data());
    std::vector<std::vector<int>> members((size_t)nc);
    for (int i = 0; i < n; ++i) members[(size_t)label[(size_t)i]].push_back(i);
    int largest = 0;
    for (const auto& m : members) largest = std::max(largest, (int)m.size());
    info[2] = nc;
    info[3] = largest;
    if (largest > mcd::kGlassoMaxDim)
        return gfail(MCD_ERR_UNSUPPORTED, "mcd_glasso: a connected component of {|S_ij| > rho} has %d variables, the device solver takes up to %d per component",
                     largest, mcd::kGlassoMaxDim);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return gfail(MCD_ERR_NO_DEVICE, "mcd_glasso: no HIP device (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return gfail(MCD_ERR_INVALID_ARG, "mcd_glasso: device %d of %d", device_id, ndev);

    const double pen = penalize_diagonal ? rho : 0.0;
    std::fill(W, W + N * N, 0.0);
    std::fill(Theta, Theta + N * N, 0.0);
    // the problems: components of two or more variables, packed one after the other; a singleton is W_ii = S_ii (+ rho), Theta_ii = 1 / W_ii
    std::vector<int> prob;
    std::vector<int32_t> dim;
    std::vector<int64_t> off, doff;
    int64_t total = 0, dtotal = 0;
    for (int c = 0; c < nc; ++c) {
        const auto& m = members[(size_t)c];
        if (m.size() == 1) {
            const size_t i = (size_t)m[0];
            W[i * N + i] = S[i * N + i] + pen;
            Theta[i * N + i] = 1.0 / W[i * N + i];
            continue;
        }
        prob.push_back(c);
        dim.push_back((int32_t)m.size());
        off.push_back(total);
        doff.push_back(dtotal);
        total += (int64_t)m.size() * (int64_t)m.size();
        dtotal += (int64_t)m.size();
    }
    const int np = (int)prob.size();
    info[6] = np;
    if (np == 0) {
        info[1] = 1;
        return MCD_OK;
    }
    std::vector<double> hS((size_t)total), hW((size_t)total);
    for (int q = 0; q < np; ++q) {
        const auto& m = members[(size_t)prob[(size_t)q]];
        const size_t p = m.size();
        double* s = hS.data() + off[(size_t)q];
        double* w = hW.data() + off[(size_t)q];
        for (size_t a = 0; a < p; ++a)
            for (size_t b = 0; b < p; ++b) {
                s[a * p + b] = S[(size_t)m[b] * N + (size_t)m[a]];      // row a = column m[a] of S, what the host solver reads as s12
                w[a * p + b] = s[a * p + b] + (a == b ? pen : 0.0);
            }
    }
    GHIP_TRY(hipSetDevice(device_id));
    Arena A;
    GHIP_TRY(hipStreamCreate(&A.st));
    mcd::GlassoDev G;
    G.n_problems = np;
    double *dS = nullptr, *dW = nullptr, *dWo = nullptr, *dB = nullptr, *dtd = nullptr, *dchg = nullptr;
    int32_t *ddim = nullptr, *dcap = nullptr;
    int64_t *doffs = nullptr, *ddoff = nullptr;
    unsigned long long* dupd = nullptr;
    GHIP_TRY(A.alloc(&dS, (size_t)total));
    GHIP_TRY(A.alloc(&dW, (size_t)total));
    GHIP_TRY(A.alloc(&dWo, (size_t)total));
    GHIP_TRY(A.alloc(&dB, (size_t)total));
    GHIP_TRY(A.alloc(&dtd, (size_t)dtotal));
    GHIP_TRY(A.alloc(&dchg, (size_t)np));
    GHIP_TRY(A.alloc(&ddim, (size_t)np));
    GHIP_TRY(A.alloc(&dcap, (size_t)np));
    GHIP_TRY(A.alloc(&doffs, (size_t)np));
    GHIP_TRY(A.alloc(&ddoff, (size_t)np));
    GHIP_TRY(A.alloc(&dupd, (size_t)np));
    GHIP_TRY(hipMemcpyAsync(dS, hS.data(), sizeof(double) * (size_t)total, hipMemcpyHostToDevice, A.st));
    GHIP_TRY(hipMemcpyAsync(dW, hW.data(), sizeof(double) * (size_t)total, hipMemcpyHostToDevice, A.st));
    GHIP_TRY(hipMemsetAsync(dB, 0, sizeof(double) * (size_t)total, A.st));
    GHIP_TRY(hipMemcpyAsync(ddim, dim.data(), sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice, A.st));
    GHIP_TRY(hipMemcpyAsync(doffs, off.data(), sizeof(int64_t) * (size_t)np, hipMemcpyHostToDevice, A.st));
    GHIP_TRY(hipMemcpyAsync(ddoff, doff.data(), sizeof(int64_t) * (size_t)np, hipMemcpyHostToDevice, A.st));
    G.dim = ddim;
    G.off = doffs;
    G.doff = ddoff;
    G.S = dS;
    G.W = dW;
    G.W_old = dWo;
    G.B = dB;
    G.Theta = dWo;                       // W_old has served its purpose when Theta is formed
    G.theta_diag = dtd;
    G.change = dchg;
    G.updates = dupd;
    G.capped = dcap;
    // prepare.graphical_lasso's rule: max |W - W_old| <= tol max(1, mean |S - diag S|), the mean over all n^2 entries
    const double threshold = tol * std::max(1.0, off_sum / ((double)n * (double)n));
    std::vector<double> chg((size_t)np);
    std::vector<unsigned long long> upd((size_t)np);
    std::vector<int32_t> cap((size_t)np);
    int64_t passes = 0, updates = 0, converged = 0, capped = 0;
    for (int pass = 0; pass < max_iter; ++pass) {
        GHIP_TRY(hipMemcpyAsync(dWo, dW, sizeof(double) * (size_t)total, hipMemcpyDeviceToDevice, A.st));
        GHIP_TRY(mcd::launch_glasso_pass(G, rho, tol, max_iter, A.st));
        GHIP_TRY(hipMemcpyAsync(chg.data(), dchg, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, A.st));
        GHIP_TRY(hipMemcpyAsync(upd.data(), dupd, sizeof(unsigned long long) * (size_t)np, hipMemcpyDeviceToHost, A.st));
        GHIP_TRY(hipMemcpyAsync(cap.data(), dcap, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, A.st));
        GHIP_TRY(hipStreamSynchronize(A.st));
        ++passes;
        double worst = 0.0;
        for (int q = 0; q < np; ++q) {
            if (!(chg[(size_t)q] <= worst)) worst = chg[(size_t)q];       // (a NaN stays the worst: never "converged")
            updates += (int64_t)upd[(size_t)q];
            capped |= cap[(size_t)q] != 0;
        }
        if (worst <= threshold) {
            converged = 1;
            break;
        }
    }
    GHIP_TRY(mcd::launch_glasso_theta(G, largest, A.st));
    std::vector<double>& hT = hS;        // (the packed S is no longer needed on the host)
    GHIP_TRY(hipMemcpyAsync(hW.data(), dW, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, A.st));
    GHIP_TRY(hipMemcpyAsync(hT.data(), G.Theta, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, A.st));
    GHIP_TRY(hipStreamSynchronize(A.st));
    for (int q = 0; q < np; ++q) {
        const auto& m = members[(size_t)prob[(size_t)q]];
        const size_t p = m.size();
        const double* w = hW.data() + off[(size_t)q];
        const double* th = hT.data() + off[(size_t)q];
        for (size_t a = 0; a < p; ++a)
            for (size_t b = 0; b < p; ++b) {
                W[(size_t)m[a] * N + (size_t)m[b]] = w[a * p + b];
                Theta[(size_t)m[a] * N + (size_t)m[b]] = th[a * p + b];
            }
    }
    info[0] = passes;
    info[1] = converged;
    info[4] = updates;
    info[5] = capped;
    return MCD_OK;
}

}  // extern "C"
