"""mcd_sparse_tree_grad_batch / mcd_hmc_create_sparse without a GPU: declared in the header, exported by the built library, bound by
the ctypes table and the Python mirror; NULL arguments are refused with a message before anything touches a device."""
import ctypes as C
import os
import re

import mcmc_date_amd as M
from mcmc_date_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["mcd_sparse_tree_grad_batch", "mcd_hmc_create_sparse"]


def test_new_calls_are_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "mcmcdate_mvn.h")).read()
    lib = _capi.lib()
    for name in NEW_CALLS:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), f"{name} is not declared in include/mcmcdate_mvn.h"
        assert name in _capi.SYMBOLS and callable(getattr(lib, name))
    assert callable(M.SparseTreeLikelihood.grad)
    # the comment that named the dense route as the only one to NUTS is gone
    assert "remains the route to the gradient" not in header and "mcd_hmc_create_sparse" in header


def test_null_arguments_are_refused_with_a_message():
    lib = _capi.lib()
    h = C.c_void_p(0x1)
    assert lib.mcd_hmc_create_sparse(C.byref(h), None, None, 1, 4) == _capi.MCD_ERR_INVALID_ARG
    assert not h.value and b"mcd_hmc_create_sparse" in lib.mcd_last_error()
    assert lib.mcd_hmc_create_sparse(None, None, None, 1, 4) == _capi.MCD_ERR_INVALID_ARG
    assert b"mcd_hmc_create_sparse" in lib.mcd_last_error()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.mcd_sparse_tree_grad_batch(None, p, p, 8, p, p, 1, 0, None, p, p, p, p, p) == _capi.MCD_ERR_INVALID_ARG
    assert b"mcd_sparse_tree_grad_batch" in lib.mcd_last_error()
