"""csrc/k_hmc_cov.hip on its own (mcd_hmc_cov_ through hmc._hmc_cov): the covariance the dense warm-up takes its metric from, at sample
counts on both sides of the 32-sample chunk -- one sample, two, a chunk less one, a chunk, several chunks with a ragged last one -- and at
dims on both sides of the 16 x 16 tile and of the mean kernel's 64 threads, on columns whose mean is thousands of standard deviations
from 0 (where a sum of squares would show).

Held to the bounds of tests/metric_product_cases.py (two-pass sums, one accumulator, references in long double), plus: cov == cov.T bit
for bit, the same bits on every call, an all-zero covariance of one sample, a NaN contained in its own row, column and mean, and the
warm-up's metric being exactly keep cov + floor I of this kernel's covariance of the recorded window.

Measured on the MI355X, worst error / bound over the shapes: mean 0.320 (n 2, dim 65), covariance 0.187 (n 2, dim 15); from 31 samples
on, mean <= 0.090 and covariance <= 0.025 (numpy's two-pass fp64: 0.09 and 0.021, tests/test_metric_product_host.py)."""
import numpy as np
import pytest

import mcmc_date_amd as M
import metric_product_cases as P
from mcmc_date_amd.hmc import _hmc_cov
from test_gpu_dense_metric import crude_inv_mass, golden_problem, posterior_states

pytestmark = pytest.mark.gpu

SHAPES = [(1, 17), (1, 130), (2, 15), (2, 65), (31, 16), (32, 1), (32, 17), (33, 17), (33, 130), (65, 130), (100, 65), (100, 15), (65, 16)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("n,dim", SHAPES)
def test_mean_and_covariance_within_their_bounds(gpu, n, dim):
    Q, offset = P.cov_inputs(n, dim)
    mean, cov = _hmc_cov(Q)
    P.check_cov(mean, cov, Q, offset, f"n {n}, dim {dim}")
    assert np.array_equal(bits(cov), bits(cov.T))
    mean2, cov2 = _hmc_cov(Q)
    assert np.array_equal(bits(mean2), bits(mean)) and np.array_equal(bits(cov2), bits(cov))
    if n == 1:
        assert np.all(cov == 0.0) and np.array_equal(mean, Q[0])


@pytest.mark.parametrize("n,dim,s,c", [(33, 35, 32, 16), (100, 65, 40, 64), (2, 17, 0, 0)])
def test_a_nan_stays_in_its_row_column_and_mean(gpu, n, dim, s, c):
    Q, _ = P.cov_inputs(n, dim)
    mean0, cov0 = _hmc_cov(Q)
    Q[s, c] = np.nan
    mean, cov = _hmc_cov(Q)
    hit = np.zeros((dim, dim), bool)
    hit[c, :] = hit[:, c] = True
    assert np.array_equal(np.isnan(cov), hit) and np.array_equal(np.isnan(mean), np.arange(dim) == c)
    # the other entries never read column c: the bits of the call without the NaN
    assert np.array_equal(bits(cov[~hit]), bits(cov0[~hit])) and np.array_equal(bits(np.delete(mean, c)), bits(np.delete(mean0, c)))


def test_the_warmup_metric_is_this_covariance_of_its_window(gpu, golden):
    """mcd_hmc_nuts_warmup_dense through the handle: 6 chains x a window of 7 = 42 positions (a chunk and a ragged one), one adapting
    window; C = keep cov + floor I of mcd_hmc_cov_'s covariance of the recorded positions, to the bit (set_metric's symmetrisation changes
    nothing of an exactly symmetric matrix)."""
    name = "12-leaves-variable-rate"
    _, topo, pf, lik, *_ = golden_problem(golden, name)
    Bc, windows, window = 6, 1, 7
    st = posterior_states(golden, name, Bc)
    mask = M.get_mask(True, topo)
    lf = M.Leapfrog(lik, pf, True, Bc)
    lf.set_state(st)
    q0 = lf.position()[0]
    lf.record_begin(period=1, capacity=(windows + 1) * window)
    eps, C, alpha = lf.nuts_warmup_dense(0.02, crude_inv_mass(q0), windows=windows, window=window, delta=0.65, max_depth=5, seed=11)
    it, sc, H, R, post, nuts = lf.record_fetch()
    lf.record_end()
    Q = np.array([M.to_vector(mask, M.State(sc[k, b, 0], sc[k, b, 1], sc[k, b, 2], H[k, b], sc[k, b, 3], sc[k, b, 4], R[k, b]))
                  for k in range(window) for b in range(Bc)])
    n = Bc * window
    assert Q.shape == (n, lf.dim) and n % 32 != 0 and np.all(np.isfinite(Q))
    assert not np.array_equal(Q[-Bc:], Q[:Bc])                                  # the chains moved inside the window
    mean, cov = _hmc_cov(Q)
    want = (n / (n + 5.0)) * cov
    want[np.diag_indices(lf.dim)] += 1e-3 * (5.0 / (n + 5.0))
    sym = 0.5 * (want + want.T)
    sym[np.diag_indices(lf.dim)] = np.diag(want)
    assert np.array_equal(bits(sym), bits(want))
    assert np.array_equal(C, sym) and np.array_equal(lf.metric(), C)
    ref = M.shrunk_covariance(Q)
    assert np.max(np.abs(C - ref) / np.sqrt(np.outer(np.diag(ref), np.diag(ref)))) <= 1e-11
