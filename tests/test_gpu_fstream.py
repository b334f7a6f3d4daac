"""The column sweep's forward factor streams (mcd_set_option "MCD_FSTREAM": 0 = padded, register-staged; 1 = compact,
register-staged; 2 = compact by LDS-DMA) must give the same bits: the compact layouts read the stored zeros on and above the
diagonal from a zero unit, the multiply-adds are the same ones in the same order, non-finite inputs included."""
import numpy as np
import pytest

import mcmc_date_amd as M
import oracle as O
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

BATCHES = (1, 40, 512, 600, 5000)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def close(a, ref):
    return np.max(np.abs(a - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-10


def per_stream(knobs, fn):
    out = {}
    M.set_logpdf_form("sweep")                       # (large batches would otherwise take the multiply or row-split form)
    try:
        for fs in (0, 1, 2):
            knobs.setenv("MCD_FSTREAM", str(fs))
            out[fs] = fn()
    finally:
        M.set_logpdf_form("auto")
    return out


@pytest.mark.parametrize("n", [64, 140, 192, 200, 255, 256, 300])      # (140, 200: the sweep stops before the last chunks)
def test_logpdf_streams_agree(gpu, n, knobs):
    mu, sigma = S.random_spd_problem(n, seed=3 * n)
    P = np.linalg.inv(sigma)
    logdet = np.linalg.slogdet(sigma)[1]
    lik = M.MvnLikelihood.from_covariance(mu, sigma)
    X = S.sample_chains(mu, sigma, max(BATCHES), seed=n)
    Xbad = X[:40].copy()
    Xbad[1, n // 2] = np.inf
    Xbad[2, 0] = -np.inf
    Xbad[3, n - 1] = np.nan
    Xbad[4, :] = np.inf
    ref = O.logpdf_full_batch(mu, P, logdet, X[:64])
    out = per_stream(knobs, lambda: ([np.asarray(lik.logpdf(X[:B])) for B in BATCHES], np.asarray(lik.logpdf(Xbad))))
    for fs in (1, 2):
        for a, b in zip(out[fs][0], out[0][0]):
            assert np.array_equal(bits(a), bits(b)), (fs, len(a))
        assert np.array_equal(bits(out[fs][1]), bits(out[0][1])), fs
    for o in out[2][0]:
        assert close(o[:64], ref[: len(o)])
    assert not np.isfinite(out[2][1][1:5]).any() and np.isfinite(out[2][1][5:]).all()


@pytest.mark.parametrize("n_leaves", [33, 72, 97, 102, 129, 151])     # N = 63, 141, 191, 201, 255, 299
def test_tree_logpdf_streams_agree(gpu, n_leaves, knobs):
    topo = S.random_topology(n_leaves, seed=n_leaves)
    n = topo.n_nodes - 2
    mu, sigma = S.random_spd_problem(n, seed=n)
    P = np.linalg.inv(sigma)
    logdet = np.linalg.slogdet(sigma)[1]
    tl = M.MvnLikelihood(M.Full(mu, P, logdet)).bind_tree(topo)
    sts = {B: S.random_states(topo, B, seed=B + n) for B in BATCHES}
    bad = S.random_states(topo, 40, seed=7)
    bad.heights[1, 3] = np.inf
    bad.rates[2, 5] = np.nan
    bad.rates[3, 0] = -np.inf
    out = per_stream(knobs, lambda: ([np.asarray(tl.loglik(sts[B])[0]) for B in BATCHES], np.asarray(tl.loglik(bad)[0])))
    for fs in (1, 2):
        for a, b in zip(out[fs][0], out[0][0]):
            assert np.array_equal(bits(a), bits(b)), (fs, len(a))
        assert np.array_equal(bits(out[fs][1]), bits(out[0][1])), fs
    st = sts[40]
    ref, _ = O.tree_loglik_full_batch(topo.parent, st.heights, st.rates, st.time_height, st.rate_mean, mu, P, logdet)
    assert close(out[2][0][1], ref)
