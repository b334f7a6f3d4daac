"""The stripe kernel with a finishing wave per chain (csrc/stripe_device.hpp: k_logpdf_stripe_fin, MCD_STRIPE_FINISH = 1) is schedule 2
with another tail, so it keeps loads in flight into registers the compiler believes written and adds LDS reads of the same kind, the
hand-over reads, and a scalar load the compiler does not know of.  Its generated code is
held to what tests/test_stripe_codegen_host.py holds schedule 2 to (tools/stripe_inflight_audit.py: no scratch, no spills, no AGPRs,
no instruction that touches a register with a load in flight, the register loads of schedule 2).  And the host's choice
(csrc/stripe_plan.hpp: stripe_finish, the function the launcher calls) under every value of the three stripe options.  No GPU involved."""
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
    return str(tmp_path_factory.mktemp("stripe_finish_codegen"))


@pytest.mark.parametrize("R", (3, 4))
def test_finish_kernel_as_built(work, R):
    r = audit.report(M._capi.LIB_PATH, audit.STRIPE_FIN % R, work, verbose=False)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["agpr_count"] == 0 and r["vgpr_count"] <= 256, r
    assert r["violations"] == 0, r
    assert r["register_loads"] == LEADING[R] + UNITS[R][0], r           # schedule 2's: 12 + 96 and 16 + 192
    assert r["most_outstanding"] < 64, r


def hook(name, R, ncols):
    f = getattr(C.CDLL(M._capi.LIB_PATH), name)
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int]
    return f(R, ncols)


def test_stripe_finish_choice():
    names = ("MCD_STRIPE_SCHED", "MCD_STRIPE_PROLOGUE", "MCD_STRIPE_FINISH")
    before = {k: M.get_option(k) for k in names}
    try:
        for n in range(129, 257):
            R, ncols = (n + 63) // 64, 16 * ((n + 15) // 16)
            whole = ncols == 64 * R                                      # N = 177 .. 192 and 241 .. 256: schedule 2 runs there
            for sched in (None, 0, 1, 2):
                for prologue in (None, 0, 1):
                    for fin in (None, 0, 1):
                        for k, v in zip(names, (sched, prologue, fin)):
                            M.set_option(k, v)
                        two = whole and sched in (None, 2) and prologue != 0
                        assert hook("mcd_stripe_finish_selftest_", R, ncols) == (1 if two and fin != 0 else 0), (n, sched, prologue, fin)
                        # ... and the schedule's report does not know the finish
                        want = -1 if prologue == 0 else (2 if whole else 1) if sched in (None, 2) else sched
                        assert hook("mcd_stripe_schedule_selftest_", R, ncols) == want, (n, sched, prologue, fin)
        for k in names:
            M.set_option(k, None)
        assert hook("mcd_stripe_finish_selftest_", 2, 128) == -2
    finally:
        for k in names:
            M.set_option(k, before[k])
