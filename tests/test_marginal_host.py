"""The numpy restatement of the marginal-likelihood estimators (diagnostics.marginal_likelihood: the reference of csrc/k_marginal.hip's tests)
on a model whose marginal likelihood is known, and against its own definitions; the argument checks of marginal.MarginalLikelihood."""
import numpy as np
import pytest

from mcmc_date_amd import diagnostics as D
from mcmc_date_amd.marginal import MarginalLikelihood

# theta ~ N(0, 1), ll(theta) = c - theta^2 / (2 s2): the power posterior at beta is N(0, 1 / (1 + beta / s2)), Z = exp(c) / sqrt(1 + 1 / s2)
C0, S2 = -3.7, 0.25
TRUTH = C0 - 0.5 * np.log(1.0 + 1.0 / S2)


def analytic_ll(n, K, C, seed, betas=None):
    """ll [n, K C] sampled exactly from the power posteriors; chain g at point g % K."""
    betas = D.power_posterior_points(K) if betas is None else betas
    rng = np.random.default_rng(seed)
    ll = np.empty((n, K * C))
    for g in range(K * C):
        theta = rng.standard_normal(n) / np.sqrt(1.0 + betas[g % K] / S2)
        ll[:, g] = C0 - theta ** 2 / (2.0 * S2)
    return ll, betas


def test_points():
    b = D.power_posterior_points(16)
    assert b[0] == 0.0 and b[-1] == 1.0 and np.all(np.diff(b) > 0) and b.shape == (16,)
    assert np.allclose(b, (np.arange(16) / 15.0) ** (1 / 0.3), rtol=1e-15)
    assert np.array_equal(D.power_posterior_points(2), [0.0, 1.0])
    assert np.allclose(D.power_posterior_points(5, alpha=1.0), [0, 0.25, 0.5, 0.75, 1.0])
    for bad in (1, 0):
        with pytest.raises(ValueError):
            D.power_posterior_points(bad)
    with pytest.raises(ValueError):
        D.power_posterior_points(8, alpha=0.0)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_analytic_case(seed):
    """K = 16 points, 16 replicates, 200 exact samples per chain: the stepping-stone estimate within 4 standard errors of the truth
    -4.5047 (observed |z| <= 1.5, se 0.005 .. 0.007), the trapezoid within 4 of the trapezoid of the exact means (it carries a
    discretisation bias against the truth), both standard errors at most 0.02."""
    ll, betas = analytic_ll(200, 16, 16, seed)
    e = D.marginal_likelihood(ll, betas)
    assert abs(TRUTH - (-4.5047)) < 1e-4
    assert e.se_ss <= 0.02 and abs(e.ln_z_ss - TRUTH) <= 4 * e.se_ss, (e.ln_z_ss, e.se_ss)
    exact_means = C0 - 1.0 / (2.0 * S2 * (1.0 + betas / S2))
    trapezoid = (np.diff(betas) * (exact_means[:-1] + exact_means[1:]) / 2).sum()
    assert e.se_ti <= 0.02 and abs(e.ln_z_ti - trapezoid) <= 4 * e.se_ti, (e.ln_z_ti, trapezoid, e.se_ti)
    assert e.point.shape == (16, 5) and e.replicate.shape == (16, 2) and e.n_samples == 200


def test_definitions_by_loops():
    """Every output recomputed from its definition with plain loops over single chains."""
    n, K, C = 37, 5, 3
    ll, betas = analytic_ll(n, K, C, seed=4)
    e = D.marginal_likelihood(ll, betas)
    delta = np.diff(betas)
    rep = np.zeros((C, 2))
    lnr = np.zeros(K - 1)
    for r in range(C):
        for p in range(K - 1):
            x, x1 = ll[:, r * K + p], ll[:, r * K + p + 1]
            rep[r, 0] += np.log(np.mean(np.exp(delta[p] * x)))
            rep[r, 1] += delta[p] * (x.mean() + x1.mean()) / 2
    for p in range(K):
        x = ll[:, p::K].ravel()
        assert np.allclose(e.point[p, :4], [x.mean(), x.var(ddof=1), x.min(), x.max()], rtol=1e-12)
        if p < K - 1:
            lnr[p] = np.log(np.mean(np.exp(delta[p] * x)))
    assert np.allclose(e.replicate, rep, rtol=1e-12) and np.allclose(e.point[:K - 1, 4], lnr, rtol=1e-12) and np.isnan(e.point[K - 1, 4])
    assert np.isclose(e.ln_z_ss, lnr.sum(), rtol=1e-13)
    assert np.isclose(e.ln_z_ti, (delta * (e.point[:-1, 0] + e.point[1:, 0]) / 2).sum(), rtol=1e-13)
    assert np.isclose(e.se_ss, rep[:, 0].std(ddof=1) / np.sqrt(C), rtol=1e-12) and np.isclose(e.se_ti, rep[:, 1].std(ddof=1) / np.sqrt(C), rtol=1e-12)


def test_two_points_are_plain_monte_carlo_over_the_prior():
    rng = np.random.default_rng(5)
    ll = -3.0 + rng.standard_normal((50, 2 * 7))
    e = D.marginal_likelihood(ll, [0.0, 1.0])
    prior = ll[:, 0::2]
    assert np.isclose(e.ln_z_ss, np.log(np.mean(np.exp(prior))), rtol=1e-13)
    assert np.allclose(e.replicate[:, 0], np.log(np.mean(np.exp(prior), axis=0)), rtol=1e-13)
    # large magnitudes do not overflow: the maximum is taken out of the exponential
    e2 = D.marginal_likelihood(ll - 5000.0, [0.0, 1.0])
    assert np.isclose(e2.ln_z_ss, e.ln_z_ss - 5000.0, rtol=1e-13)


def test_constant_ll_is_returned_exactly():
    # exponents and value representable so that every product and sum is exact: ln Z = ll, bit for bit
    e = D.marginal_likelihood(np.full((9, 4 * 3), -3.5), [0.0, 0.25, 0.5, 1.0])
    assert e.ln_z_ss == -3.5 and e.ln_z_ti == -3.5 and e.se_ss == 0.0 and e.se_ti == 0.0
    assert np.array_equal(e.point[:, 0], np.full(4, -3.5)) and np.array_equal(e.point[:, 1], np.zeros(4))
    # any value, any points: the means are the value exactly, the standard errors 0 exactly, ln Z to the rounding of sum delta_p
    b = D.power_posterior_points(16)
    e = D.marginal_likelihood(np.full((201, 16 * 5), -3.7), b)
    assert np.array_equal(e.point[:, 0], np.full(16, -3.7)) and np.array_equal(e.point[:, 1], np.zeros(16))
    assert e.se_ss == 0.0 and e.se_ti == 0.0
    assert abs(e.ln_z_ss + 3.7) <= 16 * 4e-16 and abs(e.ln_z_ti + 3.7) <= 16 * 4e-16


def test_nan_and_single_replicate():
    ll, betas = analytic_ll(20, 4, 3, seed=6)
    e0 = D.marginal_likelihood(ll, betas)
    ll[7, 1 * 4 + 2] = np.nan                                 # point 2, replicate 1
    e = D.marginal_likelihood(ll, betas)
    assert np.all(np.isnan(e.point[2])) and np.array_equal(e.point[[0, 1, 3], :4], e0.point[[0, 1, 3], :4])
    assert np.array_equal(e.point[[0, 1], 4], e0.point[[0, 1], 4])
    assert np.all(np.isnan(e.replicate[1])) and np.array_equal(e.replicate[[0, 2]], e0.replicate[[0, 2]])
    assert all(np.isnan(v) for v in (e.ln_z_ss, e.se_ss, e.ln_z_ti, e.se_ti))
    # a NaN at the last point touches no stepping stone but both trapezoid sums
    ll, betas = analytic_ll(20, 4, 3, seed=6)
    ll[0, 3] = np.nan
    e = D.marginal_likelihood(ll, betas)
    assert e.ln_z_ss == e0.ln_z_ss and e.se_ss == e0.se_ss and np.isnan(e.ln_z_ti) and np.isnan(e.se_ti)
    # one replicate: estimates, no standard errors
    ll, betas = analytic_ll(20, 4, 1, seed=7)
    e = D.marginal_likelihood(ll, betas)
    assert np.isfinite(e.ln_z_ss) and np.isfinite(e.ln_z_ti) and np.isnan(e.se_ss) and np.isnan(e.se_ti)


def test_refusals():
    ll = np.zeros((4, 6))
    for betas in ([0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0, 0.5, 0.5, 1.0], [0.0, 0.7, 0.5, 1.0], [0.0, np.nan, 1.0], [1.0], [0.0, 0.2, 0.4, 1.0]):
        with pytest.raises(ValueError):
            D.marginal_likelihood(ll, betas)
    with pytest.raises(ValueError):
        D.marginal_likelihood(np.zeros(6), [0.0, 1.0])
    with pytest.raises(ValueError):
        D.marginal_likelihood(np.zeros((1, 2)), [0.0, 1.0])   # one value per point


class FakeSampler:
    def __init__(self, batch, first_chain=0):
        self.batch, self.first_chain, self.power = batch, first_chain, None

    def set_power(self, beta):
        self.power = np.array(beta)


def test_marginal_likelihood_checks_and_assigns_the_points():
    s = FakeSampler(12)
    ml = MarginalLikelihood(s, n_points=4, alpha=0.5)
    assert ml.replicates == 3 and np.array_equal(ml.betas, D.power_posterior_points(4, 0.5))
    assert np.array_equal(s.power, np.tile(ml.betas, 3))
    s = FakeSampler(8, first_chain=16)                         # a shard that begins at a whole group
    assert np.array_equal(MarginalLikelihood(s, 4).chain_beta, np.tile(D.power_posterior_points(4), 2))
    for batch, first, K in ((10, 0, 4), (8, 2, 4), (8, 0, 1), (8192, 0, 8192)):
        s = FakeSampler(batch, first)
        with pytest.raises(ValueError):
            MarginalLikelihood(s, K)
        assert s.power is None
