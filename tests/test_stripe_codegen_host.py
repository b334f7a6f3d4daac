"""Schedule 2 of the stripe kernel (csrc/stripe_device.hpp) keeps loads in flight into registers the compiler believes written, so its
correctness hangs on the generated code: a spill, a copy or a reuse of such a register before its covering wait gives wrong values
without any message.  These checks read the kernels out of the library as it was built (tools/stripe_inflight_audit.py: the code
object's metadata and a walk of the disassembly along every path): no scratch, no spills, no AGPRs, and no instruction that touches a
register with a load in flight.  And the host's choice of kernel (csrc/stripe_plan.hpp: stripe_schedule, the function the launcher
calls): schedule 2 for whole sweeps, schedule 1 where the sweep stops early.  No GPU involved."""
import ctypes as C
import importlib.util
import os

import pytest

import mcmc_date_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("stripe_inflight_audit", os.path.join(ROOT, "tools", "stripe_inflight_audit.py"))
audit = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(audit)

UNITS = {3: (96, 48), 4: (192, 64)}              # off-diagonal and diagonal units of the stream (fc_layout.hpp)
LEADING = {3: 12, 4: 16}                         # the prologue's loads of x, mu and 1/diag: four per row block


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("stripe_codegen"))


@pytest.mark.parametrize("R", (3, 4))
@pytest.mark.parametrize("SC", (1, 2))
def test_stripe_kernel_as_built(work, R, SC):
    r = audit.report(M._capi.LIB_PATH, audit.STRIPE % (R, SC), work, verbose=False)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["agpr_count"] == 0 and r["vgpr_count"] <= 256, r
    assert r["violations"] == 0, r
    assert r["register_loads"] == LEADING[R] + (UNITS[R][0] if SC == 2 else 0), r   # the audit saw the loads it is about
    assert r["most_outstanding"] < 64, r


def test_audit_finds_a_premature_use():
    """the walk itself: a register read under a load that only the other side of a branch has waited for"""
    sym = "k"
    text = [(0, "global_load_dwordx4", "v[4:7], v1, s[2:3]", None), (4, "s_cbranch_scc1", "2", 16), (8, "s_waitcnt", "vmcnt(0)", None),
            (12, "v_fmac_f64_e32", "v[8:9], v[4:5], v[2:3]", None), (16, "v_fmac_f64_e32", "v[8:9], v[6:7], v[2:3]", None),
            (20, "s_waitcnt", "vmcnt(0)", None), (24, "ds_read_b128", "v[4:7], v0", None), (28, "ds_read_b128", "v[12:15], v0", None),
            (32, "s_waitcnt", "lgkmcnt(1)", None), (36, "v_mov_b32_e32", "v9, v4", None), (40, "v_mov_b32_e32", "v9, v12", None),
            (44, "s_endpgm", "", None)]
    r = audit.audit(text, verbose=False)
    assert r == {"register_loads": 1, "most_outstanding": 1, "violations": 2}, (sym, r)   # 16 on the taken side, 40 under lgkmcnt(1)


def schedule(R, ncols):
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_schedule_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int]
    return f(R, ncols)


def test_stripe_schedule_choice():
    names = ("MCD_STRIPE_SCHED", "MCD_STRIPE_PROLOGUE")
    before = {k: M.get_option(k) for k in names}
    try:
        for k in names:
            M.set_option(k, None)
        for n in range(129, 257):
            R, ncols = (n + 63) // 64, 16 * ((n + 15) // 16)
            whole = ncols == 64 * R                                      # N = 177 .. 192 and 241 .. 256: no chunk is cut
            assert schedule(R, ncols) == (2 if whole else 1), n          # the default
            M.set_option("MCD_STRIPE_SCHED", 1)
            assert schedule(R, ncols) == 1
            M.set_option("MCD_STRIPE_SCHED", 0)
            assert schedule(R, ncols) == 0
            M.set_option("MCD_STRIPE_SCHED", 2)
            M.set_option("MCD_STRIPE_PROLOGUE", 0)
            assert schedule(R, ncols) == -1                              # the private prologue has round 14's loop only
            for k in names:
                M.set_option(k, None)
        assert schedule(2, 128) == -2
    finally:
        for k in names:
            M.set_option(k, before[k])
