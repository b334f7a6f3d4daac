"""The marginal-likelihood kernels (csrc/k_marginal.hip) against the numpy restatement, on plain arrays and on the recorder's ring, and the whole
route -- power-posterior chains, device recorder, estimators -- on a fixture whose ln Z is estimated twice, independently."""
import ctypes as C

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi
from mcmc_date_amd import diagnostics as D
from test_marginal_host import analytic_ll

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)


def close(dev: D.MarginalLikelihoodEstimate, ref: D.MarginalLikelihoodEstimate):
    """Every finite output within 1e-11 max(1, |value|), variances within 1e-10 relative, the same NaN pattern: at most 2^16 terms of a few
    hundred in fp64 plus a few ulp of exp / log."""
    a = np.concatenate([dev.point[:, [0, 2, 3, 4]].ravel(), dev.replicate.ravel(), [dev.ln_z_ss, dev.se_ss, dev.ln_z_ti, dev.se_ti]])
    b = np.concatenate([ref.point[:, [0, 2, 3, 4]].ravel(), ref.replicate.ravel(), [ref.ln_z_ss, ref.se_ss, ref.ln_z_ti, ref.se_ti]])
    assert np.array_equal(np.isnan(a), np.isnan(b))
    fin = ~np.isnan(b)
    err = np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))
    print("max scaled error", err.max())
    assert np.all(err <= 1e-11), err.max()
    va, vb = dev.point[:, 1], ref.point[:, 1]
    assert np.array_equal(np.isnan(va), np.isnan(vb))
    fin = ~np.isnan(vb)
    print("max relative error of a variance", np.max(np.abs(va[fin] - vb[fin]) / np.maximum(vb[fin], 1e-300)))
    assert np.all(np.abs(va[fin] - vb[fin]) <= 1e-10 * np.abs(vb[fin]))


def same_bits(a: D.MarginalLikelihoodEstimate, b: D.MarginalLikelihoodEstimate):
    f = lambda e: np.concatenate([e.point.ravel(), e.replicate.ravel(), [e.ln_z_ss, e.se_ss, e.ln_z_ti, e.se_ti]]).view(np.uint64)
    assert np.array_equal(f(a), f(b))


@pytest.mark.parametrize("n,K,Cr", [(1, 2, 2), (65, 3, 1), (200, 16, 16), (257, 128, 4)])
def test_estimate_against_the_restatement(gpu, n, K, Cr):
    import torch

    ll, betas = analytic_ll(n, K, Cr, seed=1)                 # (200, 16, 16): the arrays of the host test's analytic case
    ref = D.marginal_likelihood(ll, betas)
    host = D.marginal_likelihood_device(ll, betas)
    close(host, ref)
    assert host.point.shape == (K, 5) and host.replicate.shape == (Cr, 2)
    dev = D.marginal_likelihood_device(torch.from_numpy(ll).to(gpu), betas)
    same_bits(host, dev)
    same_bits(host, D.marginal_likelihood_device(ll, betas))  # a fixed order of every sum
    if Cr == 1:
        assert np.isnan(host.se_ss) and np.isnan(host.se_ti)
    # a NaN: its point, its replicate and the totals, nothing else
    bad = ll.copy()
    bad[n // 2, (Cr - 1) * K + 1] = np.nan
    close(D.marginal_likelihood_device(bad, betas), D.marginal_likelihood(bad, betas))
    # a constant: returned exactly
    const = D.marginal_likelihood_device(np.full((n, K * Cr), -3.5), betas)
    assert np.array_equal(const.point[:, 0], np.full(K, -3.5)) and np.array_equal(const.point[:, 1], np.zeros(K))
    close(const, D.marginal_likelihood(np.full((n, K * Cr), -3.5), betas))
    if Cr > 1:
        assert const.se_ss == 0.0 and const.se_ti == 0.0
    # NULL outputs are skipped
    out = np.empty(4)
    b = np.ascontiguousarray(betas)
    _capi.check(_capi.lib().mcd_ml_estimate(n, K * Cr, C.c_void_p(ll.ctypes.data), 0, 0, K, b.ctypes.data_as(_dp), None, None, out.ctypes.data_as(_dp)))
    assert out[0] == host.ln_z_ss and out[2] == host.ln_z_ti


def test_estimate_refusals(gpu):
    ll = np.zeros((4, 6))
    # not starting at 0, not ending at 1, not increasing (twice), a NaN, a single point, a batch that is no multiple of the points
    for betas in ([0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0, 1.0, 1.0], [0.0, 0.5, 0.4, 0.6, 0.8, 1.0], [0.0, np.nan, 1.0], [1.0], [0.0, 0.2, 0.4, 1.0]):
        with pytest.raises(M.McdError) as e:
            D.marginal_likelihood_device(ll, np.array(betas))
        assert e.value.code == _capi.MCD_ERR_INVALID_ARG, (betas, e.value)
    with pytest.raises(M.McdError) as e:
        D.marginal_likelihood_device(np.zeros((1, 2)), np.array([0.0, 1.0]))      # one value per point
    assert e.value.code == _capi.MCD_ERR_INVALID_ARG
    with pytest.raises(M.McdError) as e:
        D.marginal_likelihood_device(np.zeros((1, 8194)), np.linspace(0.0, 1.0, 4097))
    assert e.value.code == _capi.MCD_ERR_INVALID_ARG


def fixture_sampler(golden, B, seed, inflate=1.0):
    fx = golden["12-leaves-variable-rate"]
    topo = M.Topology(fx["parent"])
    cal = [M.Calibration(f"c{i}", int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for i, r in enumerate(fx["cal"])]
    con = [M.Constraint(f"k{i}", int(r[0]), int(r[1]), r[2]) for i, r in enumerate(fx["con"])]
    ht = float(fx["prior_ht"])
    ps, _ = M.proposals(topo, [], calibrations_available=len(cal) > 0)
    n = fx["mu"].size
    lik = M.MvnLikelihood(M.Full(fx["mu"], np.asarray(fx["sigma_inv"]) / inflate, float(fx["logdet"]) + n * np.log(inflate))).bind_tree(topo)
    smp = M.Sampler(lik, M.PriorFunction(ht, "UncorrelatedGamma", cal, con, [], topo), ps, B, seed=seed)
    x0 = M.init_with(topo, fx["mean_lengths"])
    x0.time_height = ht
    smp.set_state(M.StateBatch.from_states([x0] * B))
    return smp


def test_record_marginal_on_a_wrapping_window(gpu, golden):
    """23 nodes, K = 4 points x 4 replicates, a ring of 16 samples: 10 recorded, 6 fetched, 10 more -- the 14 waiting samples wrap around the
    ring's end.  mcd_mh_record_marginal on them = mcd_ml_estimate on their fetched ln likelihoods, bit for bit (the same arithmetic in the
    same order), = the numpy restatement within the kernels' bound; the recorder is as it was (a twin handle that never asked fetches the
    same samples); a window that reaches back before set_power is refused and writes nothing."""
    K, Cr = 4, 4
    B = K * Cr
    betas = D.power_posterior_points(K)
    fetched = []
    for ask in (True, False):
        smp = fixture_sampler(golden, B, seed=3)
        smp.set_power(np.tile(betas, Cr))
        smp.record_begin(2, 16)
        smp.run(20)
        smp.record_fetch(6)
        smp.run(20)
        assert smp.record_count() == 14
        if ask:
            est = smp.record_marginal(betas)
            assert est.n_samples == 14
            same_bits(est, smp.record_marginal(betas))
            part = smp.record_marginal(betas, skip=3, n=9)
        fetched.append(smp.record_fetch())
        if ask:
            assert smp.record_count() == 0
        smp.record_end()
    (it, sc, H, R, post, beta), other = fetched
    assert all(np.array_equal(x, y) for x, y in zip(fetched[0], other))
    assert np.array_equal(it, 2 * np.arange(7, 21)) and np.array_equal(beta, np.tile(np.tile(betas, Cr), (14, 1)))
    ll = np.ascontiguousarray(post[:, :, 1])
    same_bits(est, D.marginal_likelihood_device(ll, betas))
    same_bits(part, D.marginal_likelihood_device(ll[3:12], betas))
    close(est, D.marginal_likelihood(ll, betas))
    # samples from before set_power in the window
    smp = fixture_sampler(golden, B, seed=3)
    smp.record_begin(2, 16)
    smp.run(4)
    smp.set_power(np.tile(betas, Cr))
    smp.run(20)
    point, rep, out = np.full((K, 5), 7.0), np.full((Cr, 2), 7.0), np.full(4, 7.0)
    used = C.c_int64(-1)
    rc = _capi.lib().mcd_mh_record_marginal(smp._h, K, betas.ctypes.data_as(_dp), 0, -1, C.byref(used), point.ctypes.data_as(_dp), rep.ctypes.data_as(_dp),
                                            out.ctypes.data_as(_dp))
    msg = _capi.lib().mcd_last_error().decode()
    assert rc == _capi.MCD_ERR_INVALID_ARG and "sample" in msg and "chain" in msg and "mcd_mh_set_power" in msg, msg
    assert used.value == 0 and np.all(point == 7.0) and np.all(rep == 7.0) and np.all(out == 7.0)
    good = smp.record_marginal(betas, skip=2)                 # the window behind them
    assert good.n_samples == 10 and np.isfinite(good.ln_z_ss)
    # refused before any launch: betas and window errors, no recorder
    for args in ((np.array([0.0, 0.5, 1.0]), 0, None), (betas, 12, None), (betas, 0, 13), (betas[::-1].copy(), 0, None)):
        with pytest.raises(M.McdError) as e:
            smp.record_marginal(*args)
        assert e.value.code == _capi.MCD_ERR_INVALID_ARG
    assert smp.record_count() == 12
    smp.record_end()
    with pytest.raises(M.McdError):
        smp.record_marginal(betas)


INFLATE = 1e5
N_ITER = 600


def test_end_to_end_two_independent_estimates(gpu, golden):
    """12-leaves fixture, the prior of the sampler tests, the covariance inflated by f = 1e5: under the prior-only CPU twin (32 chains, the
    repetitive burn-in, 300 samples each) ln likelihood has the standard deviation 0.79, inside [0.5, 1.5].  ln Z twice with different
    seeds: 16 points x 16 replicates, and 2 points x 128 replicates (plain Monte Carlo over the prior); the stepping-stone estimates agree
    within 4 combined standard errors, which are at most 0.1 nats; inside the first run stepping stones and trapezoid agree within their
    errors plus the trapezoid's bias bound (trapezoid against Simpson's rule on the same point means).  600 iterations per run after the
    repetitive burn-in; measured on the device: combined standard error 0.0026 nats (0.0024 at 2000 iterations), difference 0.0020, the
    bias bound 0.0007."""
    est = {}
    for K, Cr, seed in ((16, 16, 21), (2, 128, 22)):
        smp = fixture_sampler(golden, K * Cr, seed=seed, inflate=INFLATE)
        ml = M.MarginalLikelihood(smp, n_points=K)
        ml.burn_in()
        est[K] = ml.run(N_ITER, period=2)
        assert est[K].n_samples == N_ITER // 2 and "factor resident in LDS" in smp.last_path()
        print(K, "points:", est[K].ln_z_ss, "+-", est[K].se_ss, "trapezoid", est[K].ln_z_ti, "+-", est[K].se_ti)
    a, b = est[16], est[2]
    combined = np.sqrt(a.se_ss ** 2 + b.se_ss ** 2)
    print("difference", a.ln_z_ss - b.ln_z_ss, "combined standard error", combined)
    assert combined <= 0.1, combined
    assert abs(a.ln_z_ss - b.ln_z_ss) <= 4 * combined, (a.ln_z_ss, b.ln_z_ss, combined)
    # Simpson's rule on the unevenly spaced point means, pairs of intervals (16 points: 15 intervals, the last one by the trapezoid)
    x, y = D.power_posterior_points(16), a.point[:, 0]
    simpson = 0.0
    for i in range(0, 14, 2):
        h0, h1 = x[i + 1] - x[i], x[i + 2] - x[i + 1]
        simpson += (h0 + h1) / 6 * ((2 - h1 / h0) * y[i] + (h0 + h1) ** 2 / (h0 * h1) * y[i + 1] + (2 - h0 / h1) * y[i + 2])
    simpson += (x[15] - x[14]) * (y[14] + y[15]) / 2
    bias = abs(a.ln_z_ti - simpson)
    print("trapezoid", a.ln_z_ti, "Simpson", simpson, "bias bound", bias)
    assert abs(a.ln_z_ss - a.ln_z_ti) <= 4 * np.sqrt(a.se_ss ** 2 + a.se_ti ** 2) + bias

