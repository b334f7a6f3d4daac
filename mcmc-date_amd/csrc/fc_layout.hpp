// fc_layout.hpp -- the compact forward factor stream Fc (host_factor.cpp packs it, mvn_device.hpp reads it); plain constexpr C++,
// shared by the host and the device.
//
// The column sweep consumes the scaled forward factor in chunks of CP column pairs x the row blocks k = JB .. R-1 of the
// chunk's 64-column block JB, one 1-KiB unit (16 bytes per lane) per (column pair, row block).  In the padded stream Ft a
// diagonal unit (k = JB) of the pair p' (0 .. 31 inside the block) is nonzero only in lanes 2 p' + 1 .. 63: about a fifth
// of the stream at R = 4 is stored zeros.  Fc keeps the chunks in consumption order and lays out each one as
//   * its diagonal part: the nonzero lanes 2 p' + 1 .. 63 of each of the chunk's pairs, back to back (16 bytes per lane),
//     padded with zeros up to a whole number of units (CP = 4: R = 6, 8; whole already for CP >= 8);
//   * then the off-diagonal units (pair p, row block k > JB), pair after pair, k ascending -- the padded order.
// A chunk is therefore a run of consecutive units, copied to its LDS ring slot as it is.
#pragma once

namespace mcd {

// column pairs per chunk (mvn_device.hpp: Cfg<R>::CP, which is checked against this)
constexpr int fc_cp(int R) { return (R == 1) ? 32 : (R == 2) ? 16 : (R <= 4) ? 8 : (R <= 8) ? 4 : ((R >= 12 ? 64 : 32) / 16); }
constexpr int fc_cpb(int R) { return 32 / fc_cp(R); }                     // chunks per 64-column block
constexpr int fc_nchunk(int R) { return R * fc_cpb(R); }

// 16-byte lanes of the diagonal part before pair p of chunk lc (0 .. CPB-1) of a block
constexpr int fc_diag_start(int R, int lc, int p) { return p * (64 - 2 * lc * fc_cp(R) - p); }   // sum over q < p of 63 - 2 (lc CP + q)
constexpr int fc_diag_units(int R, int lc) { return (fc_diag_start(R, lc, fc_cp(R)) + 63) / 64; }
// units of chunk ci
constexpr int fc_chunk_units(int R, int ci)
{
    return fc_diag_units(R, ci % fc_cpb(R)) + fc_cp(R) * (R - 1 - ci / fc_cpb(R));
}
// first unit of chunk ci in Fc
constexpr int fc_chunk_base(int R, int ci)
{
    int s = 0;
    for (int c = 0; c < ci; ++c) s += fc_chunk_units(R, c);
    return s;
}
constexpr int fc_total_units(int R) { return fc_chunk_base(R, fc_nchunk(R)); }

// the sweeps that read Fc: 129 .. 256 dimensions (mvn_device.hpp: fwd_stream); elsewhere it is not made (MvnDev::Fc = NULL)
constexpr bool fwd_stream_compact(int R) { return R == 3 || R == 4; }

static_assert(fc_total_units(4) == 256, "N = 256: the triangle in 256 units");
static_assert(fc_diag_units(4, 0) == 7 && fc_diag_units(4, 1) == 5 && fc_diag_units(4, 2) == 3 && fc_diag_units(4, 3) == 1,
              "R = 4: whole diagonal units per chunk");

}  // namespace mcd
