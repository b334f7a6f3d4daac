"""hmc.factor_metric(C, where="host") -- mcd_metric_factor over the host's long double loops, what mcd_hmc_set_metric runs by default: the
factors meet the textbook componentwise bounds and the structure the kernels rely on, every refusal names its offender, and the device
path never falls back to the host.  No GPU needed.  Matrices, bounds and refusals: tests/metric_factor_cases.py."""
import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi

import metric_factor_cases as K


@pytest.mark.parametrize("dim", K.DIMS)
@pytest.mark.parametrize("family", K.FAMILIES)
def test_host_factors_meet_the_bounds_and_the_structure(family, dim):
    C = K.matrix(family, dim)
    sym, U, W = M.factor_metric(C, where="host")
    K.check_factors(C, sym, U, W, f"host, {family}, dim {dim}")
    again = M.factor_metric(C)                                                    # the default is the host
    assert all(np.array_equal(a, b) for a, b in zip(again, (sym, U, W)))


def test_the_symmetric_part_is_taken_within_the_symmetry_bound():
    C = K.scaled_matrix(65)
    skew = C.copy()
    skew[3, 40] += 5e-12 * np.sqrt(C[3, 3] * C[40, 40])                           # a twentieth of the bound: accepted and averaged
    sym, U, W = M.factor_metric(skew, where="host")
    assert sym[3, 40] == sym[40, 3] == 0.5 * (skew[3, 40] + skew[40, 3])
    K.check_factors(skew, sym, U, W, "host, skew within the bound, dim 65")


@pytest.mark.parametrize("case", K.refusal_cases(), ids=lambda c: c[0])
def test_host_refusals_name_the_offender(case):
    K.check_refusal(case, "host")


def test_outputs_may_be_null_and_info_reports_success():
    import ctypes
    C = K.scaled_matrix(5)
    info = (ctypes.c_int64 * 3)(9, 9, 9)
    dp = ctypes.POINTER(ctypes.c_double)
    assert _capi.lib().mcd_metric_factor(5, C.ctypes.data_as(dp), _capi.MCD_HMC_FACTOR_HOST, 0, None, None, None, info) == _capi.MCD_OK
    assert tuple(info) == (_capi.MCD_METRIC_FACTOR_OK, 0, 0)
    assert _capi.lib().mcd_metric_factor(5, C.ctypes.data_as(dp), _capi.MCD_HMC_FACTOR_HOST, 0, None, None, None, None) == _capi.MCD_OK


def test_limits_and_a_bad_where():
    with pytest.raises(M.McdError) as ei:
        M.factor_metric(np.eye(_capi.MCD_HMC_DENSE_ACROSS_MAX_DIM + 1), where="host")
    assert ei.value.code == _capi.MCD_ERR_UNSUPPORTED and "4099" in str(ei.value) and "4098" in str(ei.value)
    with pytest.raises(M.McdError) as ei:
        M.factor_metric(np.eye(3), where="both")
    assert ei.value.code == _capi.MCD_ERR_INVALID_ARG
    import ctypes
    C = np.eye(3)
    rc = _capi.lib().mcd_metric_factor(3, C.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 7, 0, None, None, None, None)
    assert rc == _capi.MCD_ERR_INVALID_ARG and "where = 7" in _capi.lib().mcd_last_error().decode()
    with pytest.raises(ValueError):
        M.factor_metric(np.ones((3, 4)))


def test_the_device_path_never_falls_back_to_the_host():
    C = K.scaled_matrix(65)
    if _capi.lib().mcd_device_count() > 0:                                        # a machine with a GPU: the device answers
        sym, U, W = M.factor_metric(C, where="device")
        K.check_factors(C, sym, U, W, "device, scaled, dim 65")
        return
    with pytest.raises(M.McdError) as ei:
        M.factor_metric(C, where="device")
    assert ei.value.code == _capi.MCD_ERR_NO_DEVICE and "no HIP device" in str(ei.value)
