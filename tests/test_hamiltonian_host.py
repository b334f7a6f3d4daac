"""Host-side checks of the hand-over and the attached Hamiltonian proposal (mcd_hmc_take_state, mcd_mh_take_state,
mcd_mh_attach_hamiltonian, mcd_mh_detach_hamiltonian, mcd_mh_hamiltonian_stats): the symbols are declared, bound and exported, and
without handles -- which no machine without a device can make -- the calls are loud errors, never a host path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcd_hmc_take_state", "mcd_mh_take_state", "mcd_mh_attach_hamiltonian", "mcd_mh_detach_hamiltonian", "mcd_mh_hamiltonian_stats")
ARITY = {"mcd_hmc_take_state": 2, "mcd_mh_take_state": 2, "mcd_mh_attach_hamiltonian": 7, "mcd_mh_detach_hamiltonian": 1,
         "mcd_mh_hamiltonian_stats": 7}


def test_the_new_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mcmcdate_mvn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _capi.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/mcmcdate_mvn.h"
        assert len(m.group(1).split(",")) == ARITY[name] == len(_capi.SYMBOLS[name][1]), name
        assert _capi.SYMBOLS[name][0] is C.c_int
        assert hasattr(lib, name) and re.search(r"\sT\s+" + name + r"$", exported, flags=re.M), f"{name} is not exported"
    # every new entry point cites the reference's lines, and the table's comment no longer says NUTS is not built
    for cite in ("app/Definitions.hs:272-278", "app/Main.hs:349-368", "app/Hamiltonian.hs:95-105"):
        assert hdr.count(cite) >= 2, cite
    assert "is not built" not in hdr[hdr.index("Batched Metropolis-Hastings-Green driver"):hdr.index("#define MCD_PROP_SCALE_SCALAR")]
    # the deviation in cycle position is stated where the call is declared and in the design notes
    assert "DEVIATION" in hdr[hdr.index("mcd_mh_attach_hamiltonian   "):hdr.index("int mcd_mh_attach_hamiltonian(")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Hamiltonian proposal in the cycle" in design and "Hamiltonian proposal in the cycle" in open(os.path.join(ROOT, "README.md")).read()


def test_python_layers_offer_the_calls():
    for cls, names in ((M.Sampler, ("attach_hamiltonian", "detach_hamiltonian", "hamiltonian_stats", "take_state")), (M.Leapfrog, ("take_state",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def test_without_handles_every_call_is_a_returned_error():
    """No device is needed to be refused: a NULL handle is MCD_ERR_INVALID_ARG with a message that names the call, as for the neighbouring
    mcd_mh_* / mcd_hmc_* entry points (mcd_mh_last_path, mcd_hmc_dim), and nothing is computed on the host instead."""
    lib = _capi.lib()
    eps = np.ones(4)
    null = C.c_void_p()
    n = C.c_int64(7)
    calls = {
        "mcd_hmc_take_state": lambda: lib.mcd_hmc_take_state(null, null),
        "mcd_mh_take_state": lambda: lib.mcd_mh_take_state(null, null),
        "mcd_mh_attach_hamiltonian": lambda: lib.mcd_mh_attach_hamiltonian(null, null, eps.ctypes.data_as(C.POINTER(C.c_double)), None, 6, 1, 0),
        "mcd_mh_detach_hamiltonian": lambda: lib.mcd_mh_detach_hamiltonian(null),
        "mcd_mh_hamiltonian_stats": lambda: lib.mcd_mh_hamiltonian_stats(null, C.byref(n), None, None, None, None, 0),
    }
    assert sorted(calls) == sorted(NEW)
    assert lib.mcd_mh_last_path(null) == _capi.MCD_ERR_INVALID_ARG and lib.mcd_hmc_dim(null) == _capi.MCD_ERR_INVALID_ARG     # the neighbours
    for name, call in calls.items():
        assert call() == _capi.MCD_ERR_INVALID_ARG, name
        assert name in lib.mcd_last_error().decode(), name
        with pytest.raises(M.McdError, match=name):
            _capi.check(call())
    assert n.value == 7                                               # nothing was written


def test_handles_cannot_be_made_without_a_device():
    """... and a machine without a device cannot get as far as a handle: the likelihood under a driver is MCD_ERR_NO_DEVICE."""
    if _capi.lib().mcd_device_count() > 0:
        return
    with pytest.raises(M.NoDevice):
        M.MvnLikelihood.from_covariance(np.zeros(3), np.eye(3))
