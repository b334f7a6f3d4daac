#pragma once
// sweep_groups.hpp -- host side of the column sweep that its kernel files (k_logpdf.hip, k_grad.hip, k_tree_logpdf.hip, k_tree_grad.hip)
// and the choice of form (sweep_launch.cpp) share: the R groups, the launch geometry and the per-R ring configuration.
//
// Each sweep kernel file is compiled once per R group (-DMCD_RGROUP=0: R in {1,2,3,4}; 1: {6,8}; 2: {12}; 3: {16}) so that the template
// instantiations build in parallel and the big ones never share a translation unit.  A compile defines launch_*_g<MCD_RGROUP>, the
// entry of its group; the public launch_* (sweep_launch.cpp) pick the form and hand the sweep to the group of the handle's R.
#include <type_traits>

#include "fc_layout.hpp"
#include "mvn_kernels.h"
#include "options.h"

namespace mcd {

constexpr int kSweepGroups = 4;
constexpr int sweep_group(int R) { return (R >= 1 && R <= 4) ? 0 : (R == 6 || R == 8) ? 1 : (R == 12) ? 2 : (R == 16) ? 3 : -1; }

// MCD_DISPATCH_R(R_, CALL): return CALL(R) for the R of this compile's group that equals R_, hipErrorInvalidValue if there is none.  A
// switch, so that a group's instantiations -- and with them its kernels in the device object -- keep the order of its R; the
// static_asserts hold the lists to sweep_group.
#ifndef MCD_RGROUP
#define MCD_RGROUP 0
#endif
#define MCD_R_CASE(R, CALL) case R: static_assert(sweep_group(R) == MCD_RGROUP, "sweep_group"); return CALL(R);
#if MCD_RGROUP == 0
#define MCD_GROUP_R(CALL) MCD_R_CASE(1, CALL) MCD_R_CASE(2, CALL) MCD_R_CASE(3, CALL) MCD_R_CASE(4, CALL)
#elif MCD_RGROUP == 1
#define MCD_GROUP_R(CALL) MCD_R_CASE(6, CALL) MCD_R_CASE(8, CALL)
#elif MCD_RGROUP == 2
#define MCD_GROUP_R(CALL) MCD_R_CASE(12, CALL)
#else
#define MCD_GROUP_R(CALL) MCD_R_CASE(16, CALL)
#endif
#define MCD_DISPATCH_R(R_, CALL) switch (R_) { MCD_GROUP_R(CALL) default: return hipErrorInvalidValue; }
#define MCD_CAT2(a, b) a##b
#define MCD_CAT(a, b) MCD_CAT2(a, b)

// The groups' entries.  The gradients have none at R = 16: launch_grad / launch_tree_grad take the row split there.
using SweepLogpdfFn = hipError_t(const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, hipStream_t st);
using SweepGradFn = hipError_t(const MvnDev& M, const double* X, int64_t ldx, int64_t batch, double* ll, double* G, int64_t ldg, hipStream_t st);
using SweepTreeLogpdfFn = hipError_t(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds, const double* tH,
                                     const double* rMu, int64_t batch, double* ll, double* logjac, hipStream_t st);
using SweepTreeLogpdfPriorFn = hipError_t(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds, const double* tH,
                                          const double* rMu, int64_t batch, double* ll, double* logjac, const MhDev& J, const PriorDev& JP,
                                          hipStream_t st);
using SweepTreeGradFn = hipError_t(const MvnDev& M, const TreeDev& T, const double* H, const double* Rt, int64_t lds, const double* tH,
                                   const double* rMu, int64_t batch, double* ll, double* gH, double* gR, double* gtH, double* grMu, hipStream_t st);
SweepLogpdfFn launch_logpdf_g0, launch_logpdf_g1, launch_logpdf_g2, launch_logpdf_g3;
SweepTreeLogpdfFn launch_tree_logpdf_g0, launch_tree_logpdf_g1, launch_tree_logpdf_g2, launch_tree_logpdf_g3;
SweepTreeLogpdfPriorFn launch_tree_logpdf_prior_g0, launch_tree_logpdf_prior_g1, launch_tree_logpdf_prior_g2, launch_tree_logpdf_prior_g3;
SweepGradFn launch_grad_g0, launch_grad_g1, launch_grad_g2;
SweepTreeGradFn launch_tree_grad_g0, launch_tree_grad_g1, launch_tree_grad_g2;

// 1-KiB units per LDS ring slot (two slots): 32 KiB slots up to N = 512; above that a chunk of 32 units is
// only 4 columns and the per-chunk barrier + loader bookkeeping dominate (measured at N = 1024: the compute
// waves spent half of the sweep waiting at barriers), so 64-unit slots (128 KiB of LDS, one workgroup per CU).
constexpr int sweep_slot_units(int R) { return (R >= 12) ? 64 : 32; }
// loader waves per workgroup
constexpr int sweep_loader_waves(int R) { return (R >= 12) ? 4 : 2; }

// launch geometry by batch size (host side)
struct Geometry {
    int cw, lw, bt;
};
static inline Geometry pick_geometry(int64_t batch)
{
    // <= 512 chains (a sampler's usual batch): 2 compute waves + 2 loaders per workgroup, so that every
    // chain gets a SIMD to itself and all 256 CUs take part in pulling the factor out of L2.
    // Up to 4096 chains: 4 compute waves per workgroup keep the grid within one wave of workgroups
    // per CU for longer (measured at N = 256, B = 1024: 9.5 us against 14.4 us).
    // More: 4 compute waves x 2 chains share each pass over the factor.
    const int force = opt_get(OPT_GEOM);                 // tuning (mcd_set_option "MCD_GEOM"): 21 | 41 | 42 = compute waves, chains per wave
    if (force == 21) return {2, 2, 1};
    if (force == 41 || force == 42) return {4, 2, force == 42 ? 2 : 1};
    if (batch <= 512) return {2, 2, 1};
    if (batch <= 4096) return {4, 2, 1};
    return {4, 2, 2};
}
// ... of the likelihood sweeps (k_logpdf.hip, k_tree_logpdf.hip): at R = 16 one chain per compute wave whatever the batch -- two do not
// fit the register file (1 048 spilled registers raw x, 1 188 tree states); such a batch -- more than 4096 chains on the sweep -- is
// only reached with the form forced, the automatic choice takes the multiply form there
static inline Geometry sweep_geometry(int R, int64_t batch)
{
    Geometry g = pick_geometry(batch);
    if (R >= 16) g.bt = 1;
    return g;
}

// The forward factor stream of a likelihood sweep with cw compute waves (mcd_set_option "MCD_FSTREAM"; mvn_device.hpp: Ring, fwd_stream):
// 0 padded, 1 compact, 2 compact by LDS-DMA, 3 the inverse stream (raw x only: k_logpdf.hip, k_logpdf_stripe).  has_inverse: the launch has an FS = 3 kernel at
// all -- raw x, two compute waves, R = 3, 4; inverse_window: ... and the call lies where it is the default (logpdf_inverse_window).
// MCD_FSTREAM = 3 selects it wherever it exists, under any form, and means the geometry's default where it does not.
static inline int sweep_fwd_stream(int R, int cw, bool has_inverse, bool inverse_window)
{
    if (!fwd_stream_compact(R)) return 0;
    const int dflt = cw == 2 ? 2 : 0;
    const bool inv = has_inverse && cw == 2;
    const int f = opt_or(OPT_FSTREAM, inv && inverse_window ? 3 : dflt);
    if (f == 3) return inv ? 3 : dflt;
    return (f == 1 || f == 2) ? f : 0;
}

}  // namespace mcd
