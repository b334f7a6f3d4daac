"""k_logpdf_stripe_reg (csrc/stripe_device.hpp: stripe_wave_reg, MCD_STRIPE_DIAG = 1) requests every unit of the inverse stream by a
register load the compiler does not know to be in flight, the diagonal parts included, and has no LDS ring.  Its generated code is
held to what tests/test_stripe_finish_codegen_host.py holds the ring's kernel to (tools/stripe_inflight_audit.py: no scratch, no
spills, no AGPRs, no instruction that touches a register with a load in flight), to its count of register loads -- the prologue's,
one per off-diagonal unit and eight per diagonal part -- and to having no LDS-DMA at all.  No GPU involved."""
import importlib.util
import os

import pytest

import mcmc_date_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("stripe_inflight_audit", os.path.join(ROOT, "tools", "stripe_inflight_audit.py"))
audit = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(audit)

OFFDIAG = {3: 96, 4: 192}                        # off-diagonal units of the stream (fc_layout.hpp)
PARTS = {3: 12, 4: 16}                           # diagonal parts: four per 64-column block
LEADING = {3: 12, 4: 16}                         # the prologue's loads of x, mu and 1/diag: four per row block


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("stripe_regdiag_codegen"))


@pytest.mark.parametrize("R", (3, 4))
def test_regdiag_kernel_as_built(work, R):
    r = audit.report(M._capi.LIB_PATH, audit.STRIPE_REG % R, work, verbose=False)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["agpr_count"] == 0 and r["vgpr_count"] <= 256, r
    assert r["violations"] == 0, r
    assert r["register_loads"] == LEADING[R] + OFFDIAG[R] + 8 * PARTS[R], r   # 16 + 192 + 128 and 12 + 96 + 96
    assert r["most_outstanding"] < 64, r
    assert r["lds_dmas"] == 0, r


def test_ring_kernel_keeps_its_dmas(work):
    """the count that must be 0 above does count: the ring's kernel has one LDS-DMA per unit of a diagonal part"""
    r = audit.report(M._capi.LIB_PATH, audit.STRIPE_FIN % 4, work, verbose=False)
    assert r["lds_dmas"] == 64, r
