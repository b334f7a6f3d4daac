// k_sparse_grad.hip -- tree state -> ln likelihood and its gradient with respect to the state over a SPARSE precision matrix (gfx950):
// what k_tree_grad.hip computes from a dense factor, on the matrix as it is.  ONE launch, no scratch buffer.
//
// Reference: likelihoodFunctionWrapper over logDensitySparseMultivariateNormal (app/Probability.hs:178-184, 195-207), differentiated by
// AD in the Hamiltonian target (app/Hamiltonian.hs:72-92).  Per chain
//     dx = d - mu,   y = 1/2 (P + P^T) dx,   ll = c - 1/2 (logdet + dx . y),   g = d ll / d d = -y,
// and the chain rule of k_tree_grad.hip back to the state (s = tH rMu, d_v = s r_v (h_parent - h_v)):
//     gR[v] = s g (h_parent - h_v),   e[v] = s g r_v,   gH[v] = sum_children e[c] - e[v],   gtH = g . d / tH,   grMu = g . d / rMu
// (the root's two children share distance slot 0; the stem of the rate tree gets 0).
//
// Mapping: a workgroup of 256 threads owns C chains (1 or 2) from the first load to the last store.
//   1  dx of its chains into LDS, the distances formed on the way exactly as k_sparse_quad<C, true> stages them;
//   2  a thread owns the rows j = tid, tid + 256, ...: it walks the row's record of the symmetric part in entry order -- the SLICE-MAJOR
//      copy of the 16-wide records (SparseDev::ellT_*: [16][n_pad], so the k-th load of the 64 rows of a wave is one coalesced line;
//      all 32 loads of a row are in flight before the first FMA), entries beyond the record from the CSR arrays -- gathering dx from LDS;
//      with two chains every matrix entry is loaded once for both.  y_j never leaves the thread: dx_j y_j and g_j d_j join the thread's
//      partial sums, gR of the row's node is stored, e of that node goes to LDS;
//   3  the partial sums are added lane by lane (butterfly) and wave by wave in a fixed order; after the barrier a thread owns the nodes
//      v = tid, tid + 256, ... and gathers gH[v] from its children's e in child order.
// Every sum runs in an order that the matrix and the tree fix -- a row's product in entry order, dx . y over a thread's rows in ascending
// order and then over lanes and waves, a node's children in ascending order -- whatever the batch, the number of chains per workgroup or
// the kind of pointers: a chain's outputs are the same bits however it is called.  No atomics.  A chain whose ln likelihood is NaN gets
// NaN in every gradient entry (what the dense factor sweep does by itself); nothing of one chain reaches another.
// LDS: C (n + n_nodes) doubles: 32 KiB per chain at 2048 nodes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lds_optin.hpp"

#include "mvn_kernels.h"
#include "options.h"

namespace mcd {

namespace {

__device__ __forceinline__ double sg_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int C>
__global__ __launch_bounds__(256) void k_sparse_tree_grad(SparseDev S, SparseTreeDev T, const double* __restrict__ H, const double* __restrict__ Rt,
                                                         int64_t ld, const double* __restrict__ tH, const double* __restrict__ rMu, int64_t batch,
                                                         double* __restrict__ ll, double* __restrict__ gH, double* __restrict__ gR,
                                                         double* __restrict__ gtH, double* __restrict__ grMu)
{
    constexpr int W = kSparseEllW;
    extern __shared__ double gsh[];                          // per chain dx [n], e [n_nodes]; then the waves' partial sums [C][2][4]
    const int n = S.n, nn = T.n_nodes, per = n + nn;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * C;
    const int rr = T.root_right;
    double* red = gsh + (size_t)C * per;
    int64_t bc[C];
    bool live[C];
    double sc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        live[c] = b0 + c < batch;
        bc[c] = live[c] ? b0 + c : batch - 1;                // (a chain beyond the batch: the last one again, nothing stored)
        sc[c] = tH[bc[c]] * rMu[bc[c]];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double* h = H + bc[c] * ld;
        const double* r = Rt + bc[c] * ld;
        double* dx = gsh + (size_t)c * per;
        for (int j = tid; j < n; j += 256) {
            const int a = T.slot_node[j], pa = T.slot_parent[j];
            double d = (h[pa] - h[a]) * r[a];                // heightTreeToLengthTree, times * rates   (app/Probability.hs:201-207)
            if (j == 0) d = d + (h[0] - h[rr]) * r[rr];      // sumFirstTwo
            d = d * sc[c];
            dx[j] = d - S.mu[j];
        }
        if (tid == 0) dx[n] = 0.0;                           // e[0]: the root has no branch
    }
    __syncthreads();
    double q[C], gd[C];
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = gd[c] = 0.0;
    const int np = S.n_pad;
    for (int j = tid; j < n; j += 256) {
        const int p0 = S.s_rowptr[j], p1 = S.s_rowptr[j + 1];
        const int len = p1 - p0;
        int col[W];
        double val[W];
#pragma unroll
        for (int u = 0; u < W; ++u) {
            col[u] = S.ellT_col[(size_t)u * np + j];
            val[u] = S.ellT_val[(size_t)u * np + j];
        }
        const int a = T.slot_node[j], pa = T.slot_parent[j];
        double y[C];
#pragma unroll
        for (int c = 0; c < C; ++c) y[c] = 0.0;
#pragma unroll
        for (int u = 0; u < W; ++u) {                        // (padding of a short record: the row's own column, skipped)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double t = fma(val[u], gsh[(size_t)c * per + col[u]], y[c]);
                y[c] = (u < len) ? t : y[c];
            }
        }
        for (int p = p0 + W; p < p1; ++p) {                  // a row longer than its record
            const int k = S.s_col[p];
            const double v = S.s_val[p];
#pragma unroll
            for (int c = 0; c < C; ++c) y[c] = fma(v, gsh[(size_t)c * per + k], y[c]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double* h = H + bc[c] * ld;
            const double* r = Rt + bc[c] * ld;
            double* dx = gsh + (size_t)c * per;
            double* e = dx + n;
            const double hd = h[pa] - h[a], ra = r[a];
            double hd2 = 0.0, ra2 = 0.0;
            double d = hd * ra;
            if (j == 0) {
                hd2 = h[0] - h[rr];
                ra2 = r[rr];
                d = d + hd2 * ra2;
            }
            d = d * sc[c];
            const double g = -y[c], sg = sc[c] * g;
            q[c] = fma(dx[j], y[c], q[c]);
            gd[c] = fma(g, d, gd[c]);
            e[a] = sg * ra;
            if (live[c]) gR[bc[c] * ld + a] = sg * hd;
            if (j == 0) {
                e[rr] = sg * ra2;
                if (live[c]) gR[bc[c] * ld + rr] = sg * hd2;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double wq = sg_wave_sum(q[c]), wg = sg_wave_sum(gd[c]);
        if (lane == 0) {
            red[(c * 2 + 0) * 4 + wave] = wq;
            red[(c * 2 + 1) * 4 + wave] = wg;
        }
    }
    __syncthreads();                                         // the partial sums and every e
    const double bad = __builtin_nan("");
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (!live[c]) continue;                              // (workgroup-uniform; no barrier below)
        const int64_t b = bc[c];
        const double* rq = red + (c * 2 + 0) * 4;
        const double* rg = red + (c * 2 + 1) * 4;
        const double qq = ((rq[0] + rq[1]) + rq[2]) + rq[3];
        const double gdot = ((rg[0] + rg[1]) + rg[2]) + rg[3];
        const double llv = S.c + (-0.5) * (S.logdet + qq);   // :180 (c - 1/2 (logdet + q))
        const bool ok = llv == llv;
        const double* e = gsh + (size_t)c * per + n;
        if (tid == 0) {
            ll[b] = llv;
            gR[b * ld] = ok ? 0.0 : bad;                     // stem rate: unused by the likelihood
            gtH[b] = ok ? gdot / tH[b] : bad;
            grMu[b] = ok ? gdot / rMu[b] : bad;
        }
        if (!ok) {                                           // this thread's own stores of step 2, again
            for (int j = tid; j < n; j += 256) {
                gR[b * ld + T.slot_node[j]] = bad;
                if (j == 0) gR[b * ld + rr] = bad;
            }
        }
        for (int v = tid; v < nn; v += 256) {
            double acc = (v == 0) ? 0.0 : -e[v];
            for (int ci = T.child_ptr[v]; ci < T.child_ptr[v + 1]; ++ci) acc += e[T.child_idx[ci]];
            gH[b * ld + v] = ok ? acc : bad;
        }
    }
}

size_t sparse_grad_lds(int n, int n_nodes, int C) { return sizeof(double) * ((size_t)C * ((size_t)n + (size_t)n_nodes) + 8 * (size_t)C); }

template <int C>
hipError_t launch_grad_C(const SparseDev& S, const SparseTreeDev& T, const double* H, const double* Rt, int64_t ld, const double* tH, const double* rMu,
                         int64_t batch, double* ll, double* gH, double* gR, double* gtH, double* grMu, hipStream_t st)
{
    const size_t lds = sparse_grad_lds(S.n, T.n_nodes, C);
    if (lds > 64 * 1024)                                     // more than 64 KiB of LDS has to be allowed once per device
        if (hipError_t e = allow_dynamic_lds<k_sparse_tree_grad<C>>((int)sparse_grad_lds(kSparseGradMaxNodes - 2, kSparseGradMaxNodes, C))) return e;
    hipLaunchKernelGGL((k_sparse_tree_grad<C>), dim3((unsigned)((batch + C - 1) / C)), dim3(256), lds, st, S, T, H, Rt, ld, tH, rMu, batch, ll, gH, gR, gtH,
                       grMu);
    return hipGetLastError();
}

}  // namespace

bool sparse_tree_grad_available(const SparseFacts& S, int n_nodes)
{
    return S.rows && n_nodes >= 3 && n_nodes <= kSparseGradMaxNodes && S.n == n_nodes - 2;
}

hipError_t launch_sparse_tree_grad(const SparseDev& S, const SparseTreeDev& T, const double* H, const double* Rt, int64_t ld, const double* tH,
                                   const double* rMu, int64_t batch, double* ll, double* gH, double* gR, double* gtH, double* grMu, hipStream_t st)
{
    if (batch <= 0) return hipSuccess;
    if (!sparse_tree_grad_available(S, T.n_nodes) || S.ellT_col == nullptr || T.child_ptr == nullptr) return hipErrorInvalidValue;
    if (batch > 0x7fffffffLL) return hipErrorInvalidValue;
    // two chains per workgroup share a pass over the matrix once every CU has a workgroup anyway (as k_sparse_quad); mcd_set_option
    // "MCD_SPARSE_GRAD_CHAINS" = 1 / 2 forces either (tests, timing): the same bits
    const int force = opt_get(OPT_SPARSE_GRAD_CHAINS);
    const bool two = force == 2 || (force != 1 && batch >= 512);
    if (two) return launch_grad_C<2>(S, T, H, Rt, ld, tH, rMu, batch, ll, gH, gR, gtH, grMu, st);
    return launch_grad_C<1>(S, T, H, Rt, ld, tH, rMu, batch, ll, gH, gR, gtH, grMu, st);
}

}  // namespace mcd
