"""The numpy restatement of the convergence diagnostics (mcmc_date_amd.diagnostics: split_rhat, ess, summary) against known answers, so that
the GPU tests, which compare the kernels with this restatement, do not compare the code with itself.  No device."""
import math

import numpy as np
import pytest

from mcmc_date_amd import diagnostics as D


def ar1(phi, n=2000, B=64, burn=200, seed=7):
    """x_i = phi x_{i-1} + eps, B chains, the first `burn` samples discarded: [n, B]."""
    rng = np.random.default_rng(seed)
    eps = rng.standard_normal((n + burn, B))
    x = np.empty_like(eps)
    x[0] = eps[0]
    for i in range(1, n + burn):
        x[i] = phi * x[i - 1] + eps[i]
    return x[burn:]


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ar1_effective_sample_size_and_rhat(phi):
    x = ar1(phi)
    n, B = x.shape
    e, last, pmin = D.ess(x, 255, details=True)
    want = (1 - phi) / (1 + phi)
    print(f"phi {phi}: ess / (n B) = {float(e) / (n * B):.4f} (theory {want:.4f}), rhat {float(D.split_rhat(x)):.4f}, last lag {float(last)}, min |P_k| {float(pmin):.2e}")
    assert abs(float(e) / (n * B) / want - 1) < 0.05
    assert abs(float(D.split_rhat(x)) - 1) < 0.02
    assert 1 <= float(last) < 255                       # Geyer's rule ended the sum, not the cap


def test_shifted_means_raise_rhat():
    x = ar1(0.0, n=400, B=8)
    x = x + np.arange(8)[None, :] * 2.0
    assert float(D.split_rhat(x)) > 1.5
    # ... and a trend inside every chain too: that is what halving the chains is for
    y = ar1(0.0, n=400, B=8) + np.linspace(0, 6, 400)[:, None]
    assert float(D.split_rhat(y)) > 1.5


def test_degenerate_inputs_are_nan():
    x = ar1(0.3, n=40, B=4)
    q = np.stack([x, np.full_like(x, 2.5)], axis=2)
    r = D.split_rhat(q)
    e = D.ess(q, 5)
    assert np.isfinite(r[0]) and np.isnan(r[1]) and np.isfinite(e[0]) and np.isnan(e[1])
    assert np.isnan(D.split_rhat(x[:3])) and np.isfinite(D.split_rhat(x[:4]))
    s = D.summary(q[:3], max_lag=0)
    assert np.isnan(s.rhat).all() and np.isnan(s.ess).all() and np.array_equal(s.mean, q[:3].reshape(-1, 2).mean(axis=0))
    for bad in (4, 0, 21):                              # even, zero, above n_h - 1
        with pytest.raises(ValueError):
            D.ess(x, bad)


def test_odd_n_drops_the_oldest_sample():
    x = ar1(0.5, n=41, B=6)
    x[0] += 100.0                                       # the oldest sample: must not enter rhat or ess
    assert np.array_equal(D.split_rhat(x), D.split_rhat(x[1:]))
    assert np.array_equal(D.ess(x, 9), D.ess(x[1:], 9))
    s, t = D.summary(x[:, :, None], 9), D.summary(x[1:, :, None], 9)
    assert np.array_equal(s.pooled[:, 6:], t.pooled[:, 6:]) and s.maximum[0] > 90 and t.maximum[0] < 20


def test_summary_follows_the_definitions():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((33, 5, 4)) * [1.0, 10.0, 0.1, 3.0] + [0.0, 5.0, -2.0, 1e3]
    x[7, 2, 3] = np.nan
    s = D.summary(x, max_lag=7)
    l = 33 * 5
    flat = x.reshape(l, 4)
    srt = np.sort(flat[:, :3], axis=0)
    i, m = math.floor(0.025 * l), math.floor(0.95 * l)
    assert np.array_equal(s.ci_lower[:3], srt[i]) and np.array_equal(s.ci_upper[:3], srt[i + m - 1])
    assert np.array_equal(s.minimum[:3], srt[0]) and np.array_equal(s.maximum[:3], srt[-1])
    assert np.allclose(s.mean[:3], flat[:, :3].mean(axis=0)) and np.allclose(s.variance[:3], flat[:, :3].var(axis=0))
    assert np.isnan(s.pooled[3]).all() and np.isnan(s.per_chain[:, 3]).all() and np.isfinite(s.pooled[:3]).all()
    assert np.allclose(s.per_chain[:, :3, 1], x[:, :, :3].var(axis=0, ddof=1)) and s.per_chain.shape == (5, 4, 4)
    # the definitions, written out for one quantity
    y = x[1:, :, 0]
    seq = np.concatenate([y[:16], y[16:]], axis=1)
    W = seq.var(axis=0, ddof=1).mean()
    varp = 15 / 16 * W + seq.mean(axis=0).var(ddof=1)
    assert np.isclose(s.rhat[0], math.sqrt(varp / W), rtol=1e-13)
