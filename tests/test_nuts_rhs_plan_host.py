"""The right-hand-side plan of the across-chains NUTS (csrc/nuts_rhs_plan.hpp) is shared by the host, which sizes a round's product, and
the kernels, which fill and read its slots.  No GPU involved: the library walks every leaf of every doubling on the CPU as k_nuts_step
does, and the totals are recounted here from the definition."""
import ctypes as C

import mcmc_date_amd as M


def brute_force(depth):
    """(rounds, largest count, sum of counts) over every (j, i), j < depth: one product for the leaf's momentum, one per aligned sub tree
    of 2^k leaves (1 <= k <= j) that leaf i closes, one for the whole tree after the last leaf of the doubling."""
    rounds = largest = total = 0
    for j in range(depth):
        for i in range(1 << j):
            count = 1 + sum(1 for k in range(1, j + 1) if (i + 1) % (1 << k) == 0 and i % (1 << k) != 0) + (1 if i + 1 == (1 << j) else 0)
            rounds, largest, total = rounds + 1, max(largest, count), total + count
    return rounds, largest, total


def test_rhs_plan_selftest_every_leaf_up_to_depth_12():
    L = C.CDLL(M._capi.LIB_PATH)
    f = L.mcd_nuts_rhs_plan_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.POINTER(C.c_int64)]
    for depth in range(1, 13):
        out = (C.c_int64 * 3)()
        assert f(depth, out) == (1 << depth) - 1, depth
        assert tuple(out) == brute_force(depth), depth
    out = (C.c_int64 * 3)()
    f(12, out)
    assert out[1] == 13                       # 1 + 11 + 1 at the last leaf of doubling 11: the slots of the handle's workspace
    assert f(0, None) < 0 and f(13, None) < 0


def test_the_binding_knows_the_metric_forms():
    from mcmc_date_amd import _capi

    assert (_capi.MCD_HMC_METRIC_PER_CHAIN, _capi.MCD_HMC_METRIC_ACROSS_CHAINS) == (0, 1)
    assert _capi.MCD_HMC_DENSE_ACROSS_MAX_DIM == 2 * 2048 + 2 > _capi.MCD_HMC_DENSE_MAX_DIM
    for name in ("mcd_hmc_set_metric_form", "mcd_hmc_get_metric_form"):
        assert name in _capi.SYMBOLS and hasattr(C.CDLL(M._capi.LIB_PATH), name)
