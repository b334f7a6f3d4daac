"""mcd_trace_summary (csrc/k_summary.hip) on crafted arrays against the numpy restatement diagnostics.summary, which tests/test_diagnostics.py
checks against known answers.

Tolerances (none of them comes from what the kernels return):
  * minimum, maximum and the two order statistics are elements of the input: equal as numbers, no tolerance;
  * the mean lies within l 2^-52 max|x| of math.fsum(x) / l -- the worst case of ANY summation order of l values;
  * variances within relative 1e-10 of the two-pass value in math.fsum, on columns with |mean| / sd <= 1e4 (the two-pass form loses
    nothing to the mean; sum x^2 - (sum x)^2 / l would lose 1e8 x 2^-53 ~ 1e-8 at 1e4: one such column is there to catch it);
  * rhat within relative 1e-9, ess within relative 1e-8 and the last lag equal, on the same well-conditioned finite columns (W is a sum
    of squared deviations from a mean: on a column whose spread is 1e-14 of its mean, as "low 8 bits" below, the rounding of the mean
    alone moves W by per cent in either implementation), ess only where every |P_k| the reference examined is above 1e-9 (a P_k at
    rounding distance from 0 may stop Geyer's sum in one implementation and not in the other); at most 2 % of the quantities may be
    excluded that way;
  * a NaN anywhere in a column makes every output of that column NaN and no other column's."""
import ctypes as C
import math

import numpy as np
import pytest

from mcmc_date_amd import _capi
from mcmc_date_amd import diagnostics as D

pytestmark = pytest.mark.gpu


def ar1_columns(n, B, Q, seed=7, burn=200):
    """[n, B, Q]: AR(1) series x_i = phi x_{i-1} + eps per chain and column, phi cycling through 0, 0.5, 0.9, scaled and shifted."""
    rng = np.random.default_rng(seed)
    phi = np.array([0.0, 0.5, 0.9])[np.arange(Q) % 3]
    eps = rng.standard_normal((n + burn, B, Q))
    x = np.empty_like(eps)
    x[0] = eps[0]
    for i in range(1, n + burn):
        x[i] = phi * x[i - 1] + eps[i]
    return x[burn:] * (1.0 + np.arange(Q) % 5) + (np.arange(Q) % 7 - 3.0)


def fsum_mean_var(col):
    l = len(col)
    m = math.fsum(col) / l
    return m, math.fsum((col - m) ** 2) / l


def check(x, max_lag, got, label=""):
    """got (device) against the restatement and the fsum values on x [n, B, Q]; returns the reference."""
    n, B, Q = x.shape
    l = n * B
    ref = D.summary(x, max_lag)
    assert got.pooled.shape == (Q, 9) and got.per_chain.shape == (B, Q, 4)
    assert np.array_equal(got.pooled[:, 2:6], ref.pooled[:, 2:6], equal_nan=True), label
    assert np.array_equal(got.per_chain[:, :, 2:], ref.per_chain[:, :, 2:], equal_nan=True), label
    assert np.array_equal(np.isnan(got.pooled), np.isnan(ref.pooled)), label
    good = np.zeros(Q, bool)
    for q in range(Q):
        col = x[:, :, q].reshape(-1)
        if not np.isfinite(col).all():
            continue
        m, v = fsum_mean_var(col)
        err = abs(got.mean[q] - m)
        assert err <= l * 2.0 ** -52 * np.abs(col).max(), (label, q, err)
        good[q] = v > 0 and abs(m) <= 1e4 * math.sqrt(v)
        if good[q]:
            assert abs(got.variance[q] - v) <= 1e-10 * v, (label, q, got.variance[q], v)
            for b in range(B):
                mb, vb = fsum_mean_var(x[:, b, q])
                assert abs(got.per_chain[b, q, 0] - mb) <= n * 2.0 ** -52 * np.abs(x[:, b, q]).max()
                if n > 1 and vb > 0 and abs(mb) <= 1e4 * math.sqrt(vb):
                    assert abs(got.per_chain[b, q, 1] - vb * n / (n - 1)) <= 1e-10 * vb * n / (n - 1), (label, q, b)
    g = np.nonzero(good)[0]
    assert len(g) > 0
    print(f"{label}: max rel rhat error {np.nanmax(np.abs(got.rhat[g] / ref.rhat[g] - 1), initial=0):.2e}")
    assert np.allclose(got.rhat[g], ref.rhat[g], rtol=1e-9, atol=0, equal_nan=True), label
    if max_lag:
        keep = g[ref.min_abs_p[g] > 1e-9]
        assert len(g) - len(keep) <= 0.02 * Q, (label, len(g) - len(keep))
        print(f"{label}: max rel ess error {np.nanmax(np.abs(got.ess[keep] / ref.ess[keep] - 1), initial=0):.2e}, smallest |P_k| {ref.min_abs_p[g].min():.2e}")
        assert np.allclose(got.ess[keep], ref.ess[keep], rtol=1e-8, atol=0, equal_nan=True), label
        assert np.array_equal(got.last_lag[keep], ref.last_lag[keep], equal_nan=True), label
        assert np.isfinite(got.ess[keep]).any()
    else:
        assert np.isnan(got.ess).all() and np.isnan(got.last_lag).all()
    return ref


@pytest.mark.parametrize("n,B,Q,ldq,max_lag", [(7, 3, 1, 1, 1), (64, 5, 65, 72, 31), (33, 17, 130, 136, 15), (257, 2, 64, 64, 127)])
def test_tail_shapes(gpu, n, B, Q, ldq, max_lag):
    X = np.full((n, B, ldq), 1e300)                      # the padding beyond Q must never be read into a result
    X[:, :, :Q] = ar1_columns(n, B, Q)
    if Q > 3:
        X[:, :, 3] = 0.98e4 * 2.0 + X[:, :, 3] / np.std(X[:, :, 3]) * 2.0  # mean ~ 1e4 sd: the sum x^2 form would show here
    got = D.trace_summary(X, max_lag, q=Q)
    check(X[:, :, :Q], max_lag, got, f"{n}x{B}x{Q}")
    got0 = D.trace_summary(X, 0, q=Q)                     # no effective sample size: everything else the same bits
    assert np.array_equal(got0.pooled[:, :7], got.pooled[:, :7], equal_nan=True) and np.isnan(got0.pooled[:, 7:]).all()


@pytest.fixture(scope="module")
def adversarial():
    """[520, 4, 16]: n_h = 260 carries max_lag = 255; columns 0-7 AR(1), then the adversarial ones."""
    n, B = 520, 4
    l = n * B
    rng = np.random.default_rng(11)
    x = np.empty((n, B, 16))
    x[:, :, :8] = ar1_columns(n, B, 8, seed=5)
    x[:, :, 8] = 2.5                                                        # all equal
    x[:, :, 9] = np.where(rng.random((n, B)) < 0.05, 3.0, 1.0)              # two distinct values, the rarer one around the upper rank
    low = (np.float64(1.0).view(np.uint64) & ~np.uint64(255)) | rng.integers(0, 256, (n, B)).astype(np.uint64)
    x[:, :, 10] = low.view(np.float64)                                      # differ in the lowest 8 bits only
    x[:, :, 11] = np.where(rng.random((n, B)) < 0.5, -1.5, 1.5)             # differ in the sign only
    inf = rng.standard_normal((n, B))
    u = rng.random((n, B))
    inf[u < 0.04] = -np.inf
    inf[u > 0.93] = np.inf
    x[:, :, 12] = inf                                                       # both ranks fall on infinities
    x[:, :, 13] = rng.integers(-50, 50, (n, B)) * 5e-324                    # denormals of both signs
    x[:, :, 14] = np.arange(l, 0, -1, dtype=np.float64).reshape(n, B)       # a descending ramp
    x[:, :, 15] = rng.standard_normal((n, B))
    x[301, 2, 15] = np.nan                                                  # one NaN
    return x


def test_selection_adversarial(gpu, adversarial):
    x = adversarial
    got = D.trace_summary(x, 255)
    ref = check(x, 255, got, "adversarial")
    assert np.isnan(got.pooled[15]).all() and np.isnan(got.per_chain[:, 15]).all() and np.isfinite(got.pooled[14]).all()
    assert got.ci_lower[12] == -np.inf and got.ci_upper[12] == np.inf and got.ci_upper[9] == 3.0 and got.ci_lower[11] == -1.5
    assert np.isnan(got.rhat[8]) and np.isnan(got.ess[8]) and got.variance[8] == 0.0 and got.mean[8] == 2.5
    assert (ref.last_lag[:8] >= 1).all()
    # every returned order statistic is an element of its column, bit for bit
    for q in range(15):
        col = x[:, :, q].reshape(-1)
        for j in (2, 3, 4, 5):
            assert (np.abs(col) == abs(got.pooled[q, j])).any() and (col == got.pooled[q, j]).any()
        if q not in (8,):
            bits = set(col.view(np.uint64).tolist())
            assert all(np.float64(got.pooled[q, j]).view(np.uint64) in bits or got.pooled[q, j] == 0 for j in (2, 3, 4, 5))


def test_device_and_host_input_and_two_calls_give_the_same_bits(gpu, adversarial):
    import torch

    x = adversarial
    a = D.trace_summary(x, 255)
    b = D.trace_summary(x, 255)
    c = D.trace_summary(torch.from_numpy(x).to(gpu), 255)
    for other in (b, c):
        assert np.array_equal(a.pooled.view(np.uint64), other.pooled.view(np.uint64))
        assert np.array_equal(a.per_chain.view(np.uint64), other.per_chain.view(np.uint64))


def test_refusals(gpu):
    L = _capi.lib()
    x = np.zeros((40, 2, 3))
    out = np.empty((3, 9))
    dp = C.POINTER(C.c_double)

    def call(n, B, q, ldq, lag):
        return L.mcd_trace_summary(n, B, q, ldq, C.c_void_p(x.ctypes.data), 0, 0, lag, out.ctypes.data_as(dp), None)

    assert call(40, 2, 3, 3, 19) == _capi.MCD_OK
    for args, word in (((40, 2, 3, 3, 4), "odd"), ((40, 2, 3, 3, 21), "split sequences"), ((40, 2, 3, 2, 3), "ldq"),
                       ((1 << 31, 2, 1, 1, 3), "2^32"), ((40, 2, 3, 3, 257), "MCD_SUMMARY_MAX_LAG")):
        assert call(*args) == _capi.MCD_ERR_INVALID_ARG, args
        assert word in L.mcd_last_error().decode(), (args, L.mcd_last_error().decode())
    with pytest.raises(_capi.McdError, match="odd"):
        D.trace_summary(x, 2)
