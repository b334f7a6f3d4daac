// host_factor.cpp -- one-time host preparation of the likelihood operands.
//
// The reference prepares (mu, Sigma^-1, logdet Sigma) once in `prepare` (app/Main.hs:207-208,
// 230-231) and closes over them (app/Main.hs:333-347).  Here the same one-time step produces
// the Cholesky factor of Sigma and the two scaled, packed triangular factors the kernels stream.
// Inner products are accumulated in long double: this runs once per analysis, accuracy wins.
#include "host_factor.h"
#include "fc_layout.hpp"
#include "split_sched.hpp"

#include <cmath>
#include <cstring>

namespace mcd {

bool cholesky_lower(int n, const std::vector<double>& A, std::vector<double>& L)
{
    L.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        double* Li = &L[(size_t)i * n];
        for (int j = 0; j <= i; ++j) {
            const double* Lj = &L[(size_t)j * n];
            long double s = A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= (long double)Li[k] * (long double)Lj[k];
            if (i == j) {
                if (!(s > 0.0L) || !std::isfinite((double)s)) return false;
                Li[i] = (double)sqrtl(s);
            } else {
                Li[j] = (double)(s / (long double)Lj[j]);
            }
        }
    }
    return true;
}

// inverse of a lower-triangular matrix (row-major), result lower-triangular
static void tri_lower_inverse(int n, const std::vector<double>& C, std::vector<double>& W)
{
    W.assign((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        W[(size_t)j * n + j] = 1.0 / C[(size_t)j * n + j];
        for (int i = j + 1; i < n; ++i) {
            long double s = 0.0L;
            const double* Ci = &C[(size_t)i * n];
            for (int k = j; k < i; ++k) s -= (long double)Ci[k] * (long double)W[(size_t)k * n + j];
            W[(size_t)i * n + j] = (double)(s / (long double)Ci[i]);
        }
    }
}

bool precision_factors(int n, const std::vector<double>& P, std::vector<double>& W, std::vector<double>& L)
{
    // P = W^T W with W lower triangular: the Cholesky factor of P with rows and columns reversed, reversed back and
    // transposed (J P J = C C^T, W = J C^T J).  No matrix is inverted on the way to W -- the factor the multiply-form kernels
    // stream -- so its error is that of one Cholesky factorisation; L = W^-1 (Sigma = L L^T), which the column sweeps
    // stream, costs one triangular inversion: errors grow with cond(W) = sqrt(cond(P)), not with cond(P)^2 as through
    // Sigma = P^-1 followed by a second factorisation.
    std::vector<double> R((size_t)n * n), C;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) R[(size_t)i * n + j] = P[(size_t)(n - 1 - i) * n + (n - 1 - j)];
    if (!cholesky_lower(n, R, C)) return false;
    W.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) W[(size_t)i * n + j] = C[(size_t)(n - 1 - j) * n + (n - 1 - i)];
    tri_lower_inverse(n, W, L);
    return true;
}

bool spd_inverse(int n, const std::vector<double>& P, std::vector<double>& S)
{
    std::vector<double> C, W;
    if (!cholesky_lower(n, P, C)) return false;      // P = C C^T
    tri_lower_inverse(n, C, W);                      // W = C^-1
    S.assign((size_t)n * n, 0.0);                    // S = W^T W
    // column-of-W dot products: transpose W first so the inner loop is contiguous
    std::vector<double> Wt((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Wt[(size_t)j * n + i] = W[(size_t)i * n + j];
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j <= i; ++j) {
            long double s = 0.0L;
            const double* a = &Wt[(size_t)i * n];
            const double* b = &Wt[(size_t)j * n];
            for (int k = i; k < n; ++k) s += (long double)a[k] * (long double)b[k];  // W[k][i] = 0 for k < i
            S[(size_t)i * n + j] = S[(size_t)j * n + i] = (double)s;
        }
    }
    return true;
}

size_t packed_index(int R, int row, int col)
{
    const int k = row >> 6, lane = row & 63;
    return ((((size_t)(col >> 1) * R + k) * 64 + lane) << 1) + (size_t)(col & 1);
}

void pack_factors(int n, int R, const std::vector<double>& L, std::vector<double>& mu_pad, const double* mu,
                  std::vector<double>& invdiag, std::vector<double>& Ft, std::vector<double>& Ut)
{
    const int NP = 64 * R;
    mu_pad.assign(NP, 0.0);
    invdiag.assign(NP, 1.0);
    Ft.assign((size_t)NP * NP, 0.0);
    Ut.assign((size_t)NP * NP, 0.0);
    for (int i = 0; i < n; ++i) {
        mu_pad[i] = mu[i];
        invdiag[i] = 1.0 / L[(size_t)i * n + i];
    }
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < i; ++j) {
            const double lij = L[(size_t)i * n + j];
            // forward:  row i, column j  ->  L_ij / L_ii
            Ft[packed_index(R, i, j)] = lij * invdiag[i];
            // backward: U = L^T; row j, column i  ->  U_ji / U_jj = L_ij / L_jj
            Ut[packed_index(R, j, i)] = lij * invdiag[j];
        }
    }
}

void pack_compact_forward(int R, const std::vector<double>& Ft, std::vector<double>& Fc)
{
    const int CP = fc_cp(R), CPB = fc_cpb(R);
    Fc.assign((size_t)fc_total_units(R) * 128, 0.0);
    auto unit = [&](int pair, int k) { return &Ft[((size_t)pair * R + k) * 128]; };   // 64 lanes x 2 columns
    for (int ci = 0; ci < fc_nchunk(R); ++ci) {
        const int JB = ci / CPB, lc = ci % CPB;
        double* c = &Fc[(size_t)fc_chunk_base(R, ci) * 128];
        for (int p = 0; p < CP; ++p) {                     // diagonal part: lanes 2 p' + 1 .. 63 of each pair
            const int pl = lc * CP + p;
            const double* u = unit(32 * JB + pl, JB);
            double* dst = c + 2 * (size_t)fc_diag_start(R, lc, p);
            for (int l = 2 * pl + 1; l < 64; ++l, dst += 2) {
                dst[0] = u[2 * l];
                dst[1] = u[2 * l + 1];
            }
        }
        double* o = c + (size_t)fc_diag_units(R, lc) * 128;
        for (int p = 0; p < CP; ++p)                       // off-diagonal units
            for (int k = JB + 1; k < R; ++k, o += 128) std::memcpy(o, unit(32 * JB + lc * CP + p, k), 128 * sizeof(double));
    }
}

void pack_inverse_forward(int n, int R, const std::vector<double>& W, std::vector<double>& Fw)
{
    const int NP = 64 * R;
    std::vector<double> Wp((size_t)NP * NP, 0.0);         // the padded stream's layout first: pack_compact_forward owns the compact one
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) Wp[packed_index(R, i, j)] = W[(size_t)i * n + j];
    pack_compact_forward(R, Wp, Fw);
}

void invert_factor(int n, const std::vector<double>& L, std::vector<double>& W)
{
    // rows of W one after the other: W_i: = (e_i - sum_{k<i} L_ik W_k:) / L_ii, long double accumulation
    W.assign((size_t)n * n, 0.0);
    std::vector<long double> acc(n);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < i; ++j) acc[j] = 0.0L;
        const double* Li = &L[(size_t)i * n];
        for (int k = 0; k < i; ++k) {
            const long double lik = Li[k];
            const double* Wk = &W[(size_t)k * n];
            for (int j = 0; j <= k; ++j) acc[j] -= lik * (long double)Wk[j];
        }
        const long double d = Li[i];
        for (int j = 0; j < i; ++j) W[(size_t)i * n + j] = (double)(acc[j] / d);
        W[(size_t)i * n + i] = (double)(1.0L / d);
    }
}

// one A-operand tile of v_mfma_f64_16x16x4_f64: row block ib, k tile kt; lane l = W[16 ib + (l & 15)][4 kt + (l >> 4)]
static void w_tile(int n, const std::vector<double>& W, int ib, int kt, double* t)
{
    for (int l = 0; l < 64; ++l) {
        const int row = 16 * ib + (l & 15), colk = 4 * kt + (l >> 4);
        t[l] = (row < n && colk <= row) ? W[(size_t)row * n + colk] : 0.0;
    }
}

void build_split_schedule(int n, int G, const std::vector<double>& W, SplitScheduleHost& out)
{
    const int NB = (n + 15) / 16;
    out.G = G;
    out.NB = NB;
    out.nc = (16 * NB + 255) / 256;
    out.base.assign(G, 0);
    out.Ws.clear();
    out.Ws.reserve(((size_t)2 * NB * (NB + 1) + 2) * 64);
    int toff = 0;
    for (int g = 0; g < G; ++g) {
        out.base[g] = toff;
        // the group's stream: block after block (split_sched.hpp), k ascending; the four runs are consecutive pieces of it,
        // so packing the stream in order packs every wave's run in the order the wave consumes it
        for (int r = 0; r * G < NB; ++r) {
            const int b = sp_block(G, g, r);
            if (b >= NB) continue;
            for (int kt = 0; kt < 4 * (b + 1); ++kt, ++toff) {
                out.Ws.resize(out.Ws.size() + 64);
                w_tile(n, W, b, kt, &out.Ws[out.Ws.size() - 64]);
            }
        }
    }
    // tiles travel in pairs: lane l's element of tile 2 i, then of tile 2 i + 1 (one 16-byte load per lane); every wave's run
    // is a whole number of pairs (multiples of 4 tiles)
    for (size_t t = 0; t + 1 < (size_t)toff; t += 2) {
        double tmp[128];
        double* p = &out.Ws[t * 64];
        for (int l = 0; l < 64; ++l) {
            tmp[2 * l] = p[l];
            tmp[2 * l + 1] = p[64 + l];
        }
        std::memcpy(p, tmp, sizeof tmp);
    }
    out.Ws.resize(out.Ws.size() + 128, 0.0);                       // one zero pair: the clamped prefetch of an empty run reads it
}

void pack_w_tiles(int n, const std::vector<double>& W, std::vector<double>& Wt, std::vector<double>& Wtb)
{
    const int NB = (n + 15) / 16;
    Wt.assign((size_t)2 * NB * (NB + 1) * 64, 0.0);
    for (int ib = 0; ib < NB; ++ib)
        for (int kt = 0; kt < 4 * (ib + 1); ++kt) {
            double* t = &Wt[((size_t)2 * ib * (ib + 1) + kt) * 64];
            for (int l = 0; l < 64; ++l) {
                const int row = 16 * ib + (l & 15), colk = 4 * kt + (l >> 4);
                if (row < n && colk <= row) t[l] = W[(size_t)row * n + colk];
            }
        }
    Wtb.assign((size_t)2 * NB * (NB + 1) * 64, 0.0);      // sum over ib of 4 (NB - ib) tiles = 2 NB (NB + 1)
    for (int ib = 0; ib < NB; ++ib)
        for (int kt = 4 * ib; kt < 4 * NB; ++kt) {
            double* t = &Wtb[((size_t)4 * (ib * NB - ib * (ib - 1) / 2) + (kt - 4 * ib)) * 64];
            for (int l = 0; l < 64; ++l) {
                const int row = 4 * kt + (l >> 4), colk = 16 * ib + (l & 15);     // element (row, colk) of W
                if (row < n && colk <= row) t[l] = W[(size_t)row * n + colk];
            }
        }
}

}  // namespace mcd

// Host-only self test of the row-split schedule (tests/test_host.py, no GPU): runs k_split.hip's walk -- the arithmetic of
// split_sched.hpp over the tile stream build_split_schedule packed: runs, whole and cut blocks, LDS slots, the fixed-order
// combination -- on the CPU for one random residual vector and returns the relative difference between the sum of squares it
// finds and |W r|^2 computed directly; < 0 for a structural fault.
extern "C" double mcd_split_schedule_selftest_(int n, int G, unsigned seed)
{
    if (n < 1 || G < 1 || G > 32) return -1.0;
    std::vector<double> W((size_t)n * n, 0.0), r(((size_t)n + 15) / 16 * 16 + 16, 0.0);
    unsigned long long st = 0x9E3779B97F4A7C15ull ^ seed;
    auto rnd = [&]() {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return (double)((st >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 53) - 0.5;
    };
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) W[(size_t)i * n + j] = rnd();
    for (int i = 0; i < n; ++i) r[i] = rnd();
    mcd::SplitScheduleHost h;
    mcd::build_split_schedule(n, G, W, h);
    const int NB = (n + 15) / 16;
    if (h.nc != (16 * NB + 255) / 256 || h.NB != NB) return -2.0;
    long tiles_seen = 0;
    long double total = 0.0L;
    int fault = 0;
    for (int g = 0; g < G; ++g) {
        const mcd::SpGroup q = mcd::sp_group(NB, G, g);
        if ((h.base[g] & 3) || mcd::sp_run_start(q, mcd::SP_NW) != q.Tg) return -3.0;
        std::vector<std::vector<double>> slot(mcd::SP_NSLOT, std::vector<double>(16, 0.0));
        std::vector<bool> slot_set(mcd::SP_NSLOT, false), used(mcd::SP_NSLOT, false);
        long double ss = 0.0L;
        for (int w = 0; w < mcd::SP_NW; ++w) {
            int pos = mcd::sp_run_start(q, w);                                     // stream position of the run's next tile
            int nseg = 0;
            mcd::sp_for_each_segment(NB, G, g, q, w, [&](int k0, int nt, int kind) {
                if (nt <= 0 || (nt & 3) || (k0 & 3) || kind < 0 || kind > 2) fault = 4;
                if (4 * (k0 + nt) > q.ncols) fault = 5;                            // reads a column the group does not stage
                if (++nseg > mcd::SPH_MAXSEG) fault = 3;
                double acc[16] = {0};
                for (int j = 0; j < nt; ++j, ++pos) {
                    const size_t t = (size_t)h.base[g] + pos;
                    const double* pair = &h.Ws[(t >> 1) * 128];
                    for (int l = 0; l < 64; ++l) acc[l & 15] += pair[2 * l + (t & 1)] * r[4 * (k0 + j) + (l >> 4)];
                }
                tiles_seen += nt;
                if (kind == 0) {
                    for (int i = 0; i < 16; ++i) ss += (long double)acc[i] * acc[i];
                } else {
                    const int sl = kind == 1 ? 2 * w - 1 : 2 * w;
                    if (sl < 0 || sl >= mcd::SP_NSLOT || slot_set[sl]) {
                        fault = 6;
                        return;
                    }
                    slot_set[sl] = true;
                    for (int i = 0; i < 16; ++i) slot[sl][i] = acc[i];
                }
            });
            if (pos != mcd::sp_run_start(q, w + 1)) fault = 7;
        }
        mcd::sp_for_each_cut(NB, G, g, q, [&](int wf, int wl, int blk) {
            if (wf < 0 || wl >= mcd::SP_NW || wl <= wf || blk < 0 || blk >= NB) {
                fault = 9;
                return;
            }
            double z[16] = {0};
            for (int w = wf; w <= wl; ++w) {
                const int sl = w == wf ? 2 * wf : 2 * w - 1;
                if (!slot_set[sl] || used[sl]) {
                    fault = 10;
                    continue;
                }
                used[sl] = true;
                for (int k = 0; k < 16; ++k) z[k] += slot[sl][k];
            }
            for (int k = 0; k < 16; ++k) ss += (long double)z[k] * z[k];
        });
        for (int sl = 0; sl < mcd::SP_NSLOT; ++sl)
            if (slot_set[sl] && !used[sl]) fault = 11;
        total += ss;
    }
    if (fault) return -(double)fault;
    if (tiles_seen != 2L * NB * (NB + 1)) return -12.0;
    long double direct = 0.0L;
    for (int i = 0; i < n; ++i) {
        long double z = 0.0L;
        for (int j = 0; j <= i; ++j) z += (long double)W[(size_t)i * n + j] * r[j];
        direct += z * z;
    }
    return (double)(fabsl(total - direct) / direct);
}

// Host-only self test of the compact forward stream (tests/test_compact_stream.py, no GPU): packs a random lower-triangular factor
// of dimension n both ways (pack_factors' Ft, pack_compact_forward's Fc), then unpacks Fc chunk by chunk exactly as the sweep reads
// it (a diagonal unit's lane l of pair p' from the diagonal part when l > 2 p', else zero; the off-diagonal units in order) and
// compares every element with Ft at packed_index, and every nonzero with the dense scaled factor.  Returns the number of units of Fc
// (256 at n = 256) if all of it agrees, < 0 for a fault.
extern "C" int mcd_compact_stream_selftest_(int n, unsigned seed)
{
    if (n < 1 || n > 1024) return -1;
    int R = 0;
    for (int a : {1, 2, 3, 4, 6, 8, 12, 16})
        if (R == 0 && (n + 63) / 64 <= a) R = a;
    if (R == 0) return -1;
    unsigned long long st = 0x9E3779B97F4A7C15ull ^ seed;
    auto rnd = [&]() {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return (double)((st >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 53) + 0.5;
    };
    std::vector<double> L((size_t)n * n, 0.0), mu(n, 0.0), mu_pad, invdiag, Ft, Ut, Fc;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) L[(size_t)i * n + j] = rnd();        // in [0.5, 1.5): every scaled entry is nonzero
    mcd::pack_factors(n, R, L, mu_pad, mu.data(), invdiag, Ft, Ut);
    mcd::pack_compact_forward(R, Ft, Fc);
    const int CP = mcd::fc_cp(R), CPB = mcd::fc_cpb(R), NP = 64 * R;
    if (Fc.size() != (size_t)mcd::fc_total_units(R) * 128) return -2;
    std::vector<double> D((size_t)NP * NP, 0.0);          // Fc unpacked: D[row * NP + col]
    std::vector<int> seen((size_t)NP * NP, 0);
    for (int ci = 0; ci < mcd::fc_nchunk(R); ++ci) {
        const int JB = ci / CPB, lc = ci % CPB, ND = mcd::fc_diag_units(R, lc);
        const double* c = &Fc[(size_t)mcd::fc_chunk_base(R, ci) * 128];
        for (int p = 0; p < CP; ++p) {
            const int pl = lc * CP + p, col = 64 * JB + 2 * pl;
            for (int k = JB; k < R; ++k)
                for (int l = 0; l < 64; ++l) {
                    const double* e = nullptr;
                    static const double zero[2] = {0.0, 0.0};
                    if (k == JB) {
                        const int idx = mcd::fc_diag_start(R, lc, p) - (2 * pl + 1) + l;
                        e = l > 2 * pl ? c + 2 * (size_t)idx : zero;
                        if (l > 2 * pl && idx >= 64 * ND) return -3;
                    } else {
                        e = c + ((size_t)ND + (size_t)p * (R - 1 - JB) + (k - JB - 1)) * 128 + 2 * l;
                    }
                    for (int h = 0; h < 2; ++h) {
                        const size_t at = (size_t)(64 * k + l) * NP + col + h;
                        D[at] = e[h];
                        ++seen[at];
                    }
                }
        }
    }
    for (int row = 0; row < NP; ++row)
        for (int col = 0; col < NP; ++col) {
            const size_t at = (size_t)row * NP + col;
            const bool below = row >= 64 * (col / 64);     // a row block the sweep applies to this column
            if (seen[at] != (below ? 1 : 0)) return -4;
            const double f = Ft[mcd::packed_index(R, row, col)];
            if (!below) {
                if (f != 0.0) return -5;                   // (Ft holds zeros above the diagonal block)
                continue;
            }
            if (D[at] != f) return -6;
            const double want = (row < n && col < row) ? L[(size_t)row * n + col] / L[(size_t)row * n + row] : 0.0;
            if ((col < row && row < n) && (D[at] == 0.0 || std::fabs(D[at] - want) > 1e-15 * std::fabs(want))) return -7;
            if (!(col < row && row < n) && D[at] != 0.0) return -8;
        }
    return mcd::fc_total_units(R);
}

// Host-only hook of the inverse stream (tests/test_inverse_stream_host.py, no GPU): packs the lower-triangular W (row-major n x n) as
// pack_inverse_forward does into Fw, and into Fc_ref what pack_compact_forward makes of a padded stream laid out here from the same
// matrix by the layout's definition (mvn_device.hpp, "Factor stream").  Both hold fc_total_units(R) units of 128 doubles; returns that
// number, < 0 where no compact stream exists (R other than 3, 4).
extern "C" int mcd_inverse_stream_pack_(int n, const double* W, double* Fw_out, double* Fc_ref)
{
    if (n < 1 || !W || !Fw_out || !Fc_ref) return -1;
    const int R = (n + 63) / 64;
    if (n > 256 || !mcd::fwd_stream_compact(R)) return -1;
    const std::vector<double> Wv(W, W + (size_t)n * n);
    std::vector<double> Fw, Wp((size_t)64 * R * 64 * R, 0.0), Fc;
    mcd::pack_inverse_forward(n, R, Wv, Fw);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) Wp[((((size_t)(j >> 1) * R + (i >> 6)) * 64 + (i & 63)) << 1) + (j & 1)] = Wv[(size_t)i * n + j];
    mcd::pack_compact_forward(R, Wp, Fc);
    if (Fw.size() != (size_t)mcd::fc_total_units(R) * 128 || Fc.size() != Fw.size()) return -2;
    std::memcpy(Fw_out, Fw.data(), Fw.size() * sizeof(double));
    std::memcpy(Fc_ref, Fc.data(), Fc.size() * sizeof(double));
    return mcd::fc_total_units(R);
}
