"""The dense metric's factors taken on the device (csrc/k_metric_factor.hip; mcd_hmc_set_metric_factor, mcd_metric_factor with
MCD_HMC_FACTOR_DEVICE): the stand-alone factor against the textbook bounds of tests/metric_factor_cases.py, the handle's metric and U^-1
against the host-factored handle, the factor as the sampler uses it (the momenta of a transition), and the warm-up whose window
covariance never leaves the device.  Problems, metrics and helpers are those of tests/test_gpu_dense_metric.py and
tests/test_gpu_metric_across.py."""
import ctypes

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi

import metric_factor_cases as K
from test_gpu_dense_metric import (crude_inv_mass, diagonal_run, golden_problem, leapfrog_fixture, metric_for, posterior_states, same_bits,
                                   synthetic_problem)
from test_gpu_metric_across import normal_draws, safe_eps

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
NAME12 = "12-leaves-variable-rate"


# ---- 1. the stand-alone factor ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", K.DIMS)
@pytest.mark.parametrize("family", K.FAMILIES)
def test_device_factors_meet_the_bounds_and_the_structure(gpu, family, dim):
    C = K.matrix(family, dim)
    sym, U, W = M.factor_metric(C, where="device")
    K.check_factors(C, sym, U, W, f"device, {family}, dim {dim}")
    again = M.factor_metric(C, where="device")
    assert same_bits(again, (sym, U, W))                                          # the same bits on every call


@pytest.mark.parametrize("case", K.refusal_cases(), ids=lambda c: c[0])
def test_device_refusals_are_the_hosts(gpu, case):
    assert K.check_refusal(case, "device") == K.check_refusal(case, "host")       # the same offender, the same message


def test_limits_on_the_device(gpu):
    with pytest.raises(M.McdError) as ei:
        M.factor_metric(np.eye(_capi.MCD_HMC_DENSE_ACROSS_MAX_DIM + 1), where="device")
    assert ei.value.code == _capi.MCD_ERR_UNSUPPORTED
    with pytest.raises(M.McdError) as ei:
        M.factor_metric(np.eye(3), where="device", device_id=4096)
    assert ei.value.code == _capi.MCD_ERR_INVALID_ARG


# ---- 2. the handle ------------------------------------------------------------------------------------------------------------------------
def handle_problem(golden, dim):
    """(likelihood, prior, calibrations available, states, form) of the three handles: dim 37 and 388 per chain, 513 across the chains."""
    if dim == 513:
        _, lik, pf, st = synthetic_problem(171, 3, sparse=True)
        return lik, pf, False, st, "across_chains"
    return leapfrog_fixture(golden, NAME12 if dim == 37 else "synthetic-129") + ("per_chain",)


def new_handle(lik, pf, cal, st, form, where=None):
    lf = M.Leapfrog(lik, pf, cal, st.heights.shape[0])
    lf.set_metric_form(form)
    if where:
        lf.set_metric_factor(where)
    lf.set_state(st)
    return lf


@pytest.mark.parametrize("dim", [37, 388, 513])
def test_a_device_factored_handle(gpu, golden, dim):
    lik, pf, cal, st, form = handle_problem(golden, dim)
    B = st.heights.shape[0]
    never = new_handle(lik, pf, cal, st, form)
    assert never.dim == dim and never.metric_factor == "host"
    q0, _, g0 = never.position()
    inv_mass = crude_inv_mass(q0)
    eps = safe_eps(g0, np.diag(inv_mass), B)
    want = diagonal_run(never, st, inv_mass, eps)
    C = metric_for(q0)
    host = new_handle(lik, pf, cal, st, form)
    dev = new_handle(lik, pf, cal, st, form, "device")
    assert dev.metric_factor == "device" and dev.metric() is None
    host.set_metric(C)
    dev.set_metric(C)
    stored = dev.metric()
    assert np.array_equal(stored, host.metric()) and np.array_equal(stored, 0.5 * (C + C.T)) and np.array_equal(stored, stored.T)
    _, _, W_dev = M.factor_metric(C, where="device")
    _, _, W_host = M.factor_metric(C, where="host")
    uinv = dev._metric_uinv()
    assert np.array_equal(uinv, W_dev) and not np.any(np.signbit(uinv[np.triu_indices(dim, 1)]))
    assert np.array_equal(host._metric_uinv(), W_host)
    assert np.max(np.abs(W_dev - W_host) / np.sqrt(np.outer(np.diag(W_host), np.diag(W_host)))) <= 1e-6    # the same matrix, other last bits
    # a value that is no choice is refused; the choice stays
    with pytest.raises(M.McdError) as ei:
        _capi.check(_capi.lib().mcd_hmc_set_metric_factor(dev._h, 2))
    assert ei.value.code == _capi.MCD_ERR_INVALID_ARG and dev.metric_factor == "device"
    with pytest.raises(ValueError):
        dev.set_metric_factor("gpu")
    # a refused matrix leaves metric, U^-1 and state as they were
    before = dev.position()
    k = dim - 2
    with pytest.raises(M.McdError) as ei:
        dev.set_metric(K.indefinite_matrix(dim, k))
    assert ei.value.code == _capi.MCD_ERR_INVALID_ARG and "mcd_hmc_set_metric" in str(ei.value) and f"pivot {k}" in str(ei.value)
    with pytest.raises(M.McdError) as eh:
        host.set_metric(K.indefinite_matrix(dim, k))
    assert str(eh.value) == str(ei.value)                                        # today's wording
    assert np.array_equal(dev.metric(), stored) and np.array_equal(dev._metric_uinv(), W_dev) and same_bits(dev.position(), before)
    # the dense metric runs, then clear_metric gives back the handle that never had one
    a, d = dev.nuts(eps, None, max_depth=3, seed=41, transition=3)
    assert np.all(np.isfinite(a)) and not np.array_equal(dev.position()[0], want[2])
    dev.clear_metric()
    assert dev.metric() is None and dev.metric_factor == "device" and dev.metric_form == form
    assert same_bits(diagonal_run(dev, st, inv_mass, eps), want)


# ---- 3. the factor as the sampler uses it -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [37, 513])
def test_momenta_of_a_device_factored_handle(gpu, golden, dim):
    """test_nuts_at_dim_513_momenta_state_and_sub_batch (tests/test_gpu_metric_across.py) on a device-factored handle: -H at the start of a
    transition is value - 1/2 p^T C p with p = U^-T z from numpy's own Cholesky factor; a wrong triangle would be off by O(kin)."""
    lik, pf, cal, st, form = handle_problem(golden, dim)
    B, seed = st.heights.shape[0], 77
    lf = new_handle(lik, pf, cal, st, form, "device")
    q0, _, g0 = lf.position()
    # metric_for's C = S R S with the scales S floored at a thousandth of the largest: the 37 coordinates of the 12-leaves fixture span six
    # orders of magnitude, cond(metric_for) = 2.4e12 there, and the bound below is only a test (tol < 1e-3 kin) while cond(C) < about 1e9
    s = np.sqrt(crude_inv_mass(q0))
    s = np.maximum(s, 1e-3 * s.max())
    k = np.arange(dim)
    C = s[:, None] * 0.5 ** np.abs(k[:, None] - k[None, :]) * s[None, :]
    C = 0.5 * (C + C.T)
    U = np.linalg.cholesky(C)
    kappa = np.linalg.cond(C)
    eps = safe_eps(g0, C, B)
    lf.set_metric(C)
    lf.record_begin(period=1, capacity=4)
    for transition in range(2):
        value = lf.position()[1]
        lf.nuts(eps, None, max_depth=3, seed=seed, transition=transition)
        joint0 = lf.record_fetch()[5][-1, :, 5]                                  # -H at the start of the transition
        for b in range(B):
            p = np.linalg.solve(U.T, normal_draws(seed, b, transition, dim))
            kin = 0.5 * float(p @ (C @ p))
            tol = 64 * dim * U53 * kappa * (abs(value[b]) + kin)
            print(f"dim {dim}, transition {transition}, chain {b}: |joint0 - ref| {abs(joint0[b] - (value[b] - kin)):.2e}, bound {tol:.2e}, "
                  f"kin {kin:.1f}, cond {kappa:.2e}")
            assert abs(joint0[b] - (value[b] - kin)) <= tol
            assert tol < 1e-3 * kin
    lf.record_end()
    assert np.all(np.any(lf.position()[0] != q0, axis=1))


# ---- 4. the warm-up -----------------------------------------------------------------------------------------------------------------------
def warmup_on_both(lik, pf, cal, st, form, mask, im0, eps0, window, max_depth):
    B = st.heights.shape[0]
    kw = dict(windows=1, window=window, delta=0.65, max_depth=max_depth, seed=11)
    out = {}
    for where in ("host", "device"):
        lf = new_handle(lik, pf, cal, st, form, where)
        lf.record_begin(period=1, capacity=2 * window)
        eps, C, alpha = lf.nuts_warmup_dense(eps0, im0, **kw)
        it, sc, H, R, post, nuts = lf.record_fetch()
        lf.record_end()
        assert it.tolist() == list(range(1, 2 * window + 1))
        Q = np.array([M.to_vector(mask, M.State(sc[k, b, 0], sc[k, b, 1], sc[k, b, 2], H[k, b], sc[k, b, 3], sc[k, b, 4], R[k, b]))
                      for k in range(window) for b in range(B)])
        out[where] = (lf, eps, C, alpha, Q)
    (_, _, C_host, _, Q_host), (dev, eps, C, alpha, Q) = out["host"], out["device"]
    # the first window runs under the diagonal metric; covariance kernel and shrinkage are the same arithmetic: the same bits
    assert np.array_equal(Q, Q_host) and np.all(np.isfinite(Q)) and not np.array_equal(Q[-B:], Q[:B])
    assert np.array_equal(C, C_host)
    assert np.array_equal(C, C.T) and np.array_equal(dev.metric(), C) and dev.metric_factor == "device"
    ref = M.shrunk_covariance(Q)
    err = np.max(np.abs(C - ref) / np.sqrt(np.outer(np.diag(ref), np.diag(ref))))
    print(f"device-factored warm-up, dim {dev.dim}: max |C - ref| / sqrt(C_ii C_jj) = {err:.2e}, eps {eps.min():.3g} .. {eps.max():.3g}")
    assert err <= 1e-11
    assert np.array_equal(dev._metric_uinv(), M.factor_metric(C, where="device")[2])      # the closing window ran on the factor of this C
    assert np.all(np.isfinite(eps)) and np.all(np.isfinite(alpha)) and np.all((eps > 1e-3) & (eps < 1.0))
    # (the step sizes of the two handles are not compared: the closing window runs on factors that differ in the last bits)
    end = dev.position()
    dev.set_state(st)
    eps2, C2, alpha2 = dev.nuts_warmup_dense(eps0, im0, **kw)
    assert np.array_equal(eps2, eps) and np.array_equal(C2, C) and np.array_equal(alpha2, alpha) and same_bits(dev.position(), end)
    return dev


def test_warmup_factored_on_the_device(gpu, golden):
    _, topo, pf, lik, *_ = golden_problem(golden, NAME12)
    st = posterior_states(golden, NAME12, 64)
    probe = new_handle(lik, pf, True, st, "per_chain")
    dev = warmup_on_both(lik, pf, True, st, "per_chain", M.get_mask(True, topo), crude_inv_mass(probe.position()[0]), 0.02, window=20, max_depth=6)
    assert dev.dim == 37
    phases = (ctypes.c_double * 4)()
    f = _capi.lib().mcd_hmc_warmup_phases_
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    _capi.check(f(dev._h, phases))
    assert all(p >= 0 for p in phases) and phases[0] > 0 and phases[3] > 0         # the four slots, slot 0 the device factorisation


def test_warmup_factored_on_the_device_at_dim_513(gpu):
    B = 4
    topo, lik, pf, st = synthetic_problem(171, B, sparse=True)
    probe = new_handle(lik, pf, False, st, "across_chains")
    q0, _, g0 = probe.position()
    im0 = crude_inv_mass(q0)
    dev = warmup_on_both(lik, pf, False, st, "across_chains", M.get_mask(False, topo), im0, safe_eps(g0, np.diag(im0), B), window=4, max_depth=2)
    assert dev.dim == 513 and dev.metric_form == "across_chains"
