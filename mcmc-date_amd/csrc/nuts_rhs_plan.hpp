// nuts_rhs_plan.hpp -- which products with C one round of the across-chains NUTS needs (k_nuts_across.hip, hmc_capi.cpp), shared by host
// and device.  The chains of a transition are in lock step: every chain still building its tree is at doubling j, leaf i of the sub tree
// of 2^j leaves, and (j, i) is a function of the round alone.  After the leaf's second half kick the round multiplies, in this order of
// slots,
//     slot 0                  the leaf's momentum                                         (kinetic energy 1/2 p^T C p)
//     slots 1 .. closes       q+ - q- of the aligned sub tree of 2^k leaves that leaf i closes, k = 1 .. closes, i.e. (i + 1) % 2^k == 0
//                             (the order in which k_nuts_step tests them)
//     slot closes + 1         q+ - q- of the whole tree, when i + 1 == 2^j                (the sub tree is complete)
// Slot s of chain b is row s * batch + b of the workspace, so the slots in use are one [count * batch][dim] matrix.
#pragma once

#ifdef __HIPCC__
#define MCD_RHS_HD __host__ __device__ inline
#else
#define MCD_RHS_HD inline
#endif

namespace mcd {

constexpr int kNutsMaxDepthLevels = 12;                        // = kNutsMaxDepth (hmc_capi.cpp): j <= 11
constexpr int kNutsRhsMaxSlots = kNutsMaxDepthLevels + 1;      // 1 + 11 + 1 at j = 11, i = 2^11 - 1

struct NutsRhsPlan {
    int closes;     // aligned sub trees closed by the leaf: levels 1 .. closes
    int whole;      // 1: the sub tree of 2^j leaves is complete, the whole tree's U-turn test follows
    int count;      // right-hand sides of the round = 1 + closes + whole
};

// (j, i) of round r = 0, 1, ... of a transition: leaf r is leaf i of doubling j, r + 1 = 2^j + i
MCD_RHS_HD void nuts_round_position(long long r, int* j, int* i)
{
    int jj = 0;
    while (((long long)2 << jj) <= r + 1) ++jj;
    *j = jj;
    *i = (int)(r + 1 - ((long long)1 << jj));
}

MCD_RHS_HD NutsRhsPlan nuts_rhs_plan(int j, int i)
{
    NutsRhsPlan p;
    p.closes = 0;
    while (p.closes < j && ((i + 1) & ((2 << p.closes) - 1)) == 0) ++p.closes;   // level k = closes + 1 has 2^k = 2 << closes leaves
    p.whole = (i + 1 == (1 << j)) ? 1 : 0;
    p.count = 1 + p.closes + p.whole;
    return p;
}

}  // namespace mcd
