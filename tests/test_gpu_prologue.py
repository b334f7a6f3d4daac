"""The start of the column sweep's likelihood launch (k_logpdf.hip, k_tree_logpdf.hip; compact stream by LDS-DMA, the default up to
512 chains at 129 .. 256 dimensions): the kernels take their leading arguments as preloaded scalars, the compute waves issue every load
of x, mu and 1/diag before the first use, and the loaders request the first NS-1 chunks of the factor back to back and wait, with a
counted vmcnt, for chunk 0 only.  None of it may change a bit of the result: the default stream against the register-staged ones
(MCD_FSTREAM = 0, 1), against the CPU oracle within tests/test_gpu_parity.py's bound for synthetic problems, with two loader waves
instead of four (another counted wait), replayed from a graph that alternates two batches, and with a non-finite input."""
import functools

import numpy as np
import pytest

import mcmc_date_amd as M
import oracle as O
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CHAINS = (1, 3, 5)                        # an odd batch leaves one compute wave of the last workgroup on clamped input


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def parity_tol(n, kappa, logdet, ref):
    """tests/test_gpu_parity.py, synthetic Sigma: 64 N eps cond(Sigma) max(1, q)"""
    q = -2.0 * (ref + 0.9189385332046727 * n) - logdet
    return 64 * n * EPS * kappa * np.maximum(1.0, q)


@functools.lru_cache(maxsize=None)
def raw_problem(n, batch):
    mu, sigma = S.random_spd_problem(n, seed=5 * n)
    P = np.linalg.inv(sigma)
    logdet = np.linalg.slogdet(sigma)[1]
    X = S.sample_chains(mu, sigma, batch, seed=n + 1)
    ref = O.logpdf_full_batch(mu, P, logdet, X)
    return mu, sigma, X, ref, parity_tol(n, np.linalg.cond(sigma), logdet, ref)


def sweep_per_stream(knobs, fn):
    """fn() under the default stream (key None) and under MCD_FSTREAM = 0 and 1, on the sweep (N = 256 with few chains would take the row split)"""
    out = {}
    M.set_logpdf_form("sweep")
    try:
        out[None] = fn()
        for fs in (0, 1):
            knobs.setenv("MCD_FSTREAM", str(fs))
            out[fs] = fn()
    finally:
        M.set_logpdf_form("auto")
    return out


@pytest.mark.parametrize("n", [129, 140, 192, 200, 256])     # R = 3 from its first dimension; sweeps that stop before the last chunks; R = 4 full
def test_rawx_default_stream(gpu, n, knobs):
    batches = CHAINS + ((512,) if n == 256 else ())
    mu, sigma, X, ref, tol = raw_problem(n, max(batches))
    lik = M.MvnLikelihood.from_covariance(mu, sigma)
    out = sweep_per_stream(knobs, lambda: [np.asarray(lik.logpdf(X[:B])) for B in batches])
    for i, B in enumerate(batches):
        for fs in (0, 1):
            assert np.array_equal(bits(out[None][i]), bits(out[fs][i])), (fs, B)
        err = np.abs(out[None][i] - ref[:B])
        assert np.all(err <= tol[:B]), (B, err.max(), tol[:B].min())


@pytest.mark.parametrize("n_leaves", [66, 129])               # N = 129, 255
def test_tree_default_stream(gpu, n_leaves, knobs):
    topo = S.random_topology(n_leaves, seed=n_leaves)
    n = topo.n_nodes - 2
    mu, sigma = S.random_spd_problem(n, seed=n)
    P = np.linalg.inv(sigma)
    logdet = np.linalg.slogdet(sigma)[1]
    kappa = np.linalg.cond(sigma)
    tl = M.MvnLikelihood(M.Full(mu, P, logdet)).bind_tree(topo)
    sts = {B: S.random_states(topo, B, seed=B + n) for B in CHAINS}
    out = sweep_per_stream(knobs, lambda: [tuple(np.asarray(a) for a in tl.loglik(sts[B])) for B in CHAINS])
    for i, B in enumerate(CHAINS):
        for fs in (0, 1):
            assert np.array_equal(bits(out[None][i][0]), bits(out[fs][i][0])), (fs, B)
            assert np.array_equal(bits(out[None][i][1]), bits(out[fs][i][1])), (fs, B)
        st = sts[B]
        ref, refj = O.tree_loglik_full_batch(topo.parent, st.heights, st.rates, st.time_height, st.rate_mean, mu, P, logdet)
        err = np.abs(out[None][i][0] - ref)
        tol = parity_tol(n, kappa, logdet, ref)
        assert np.all(err <= tol), (B, err.max(), tol.min())
        assert np.allclose(out[None][i][1], refj, rtol=1e-12, atol=1e-12)


def test_two_loader_waves(gpu, knobs):
    """fc_dma_min, the counted wait for chunk 0, differs per loader count: a wave of two issues twice the LDS-DMAs of a wave of four"""
    mu, sigma, X, ref, tol = raw_problem(256, 512)
    lik = M.MvnLikelihood.from_covariance(mu, sigma)
    M.set_logpdf_form("sweep")
    try:
        four = np.asarray(lik.logpdf(X[:3]))
        knobs.setenv("MCD_LOADERS", "2")
        two = np.asarray(lik.logpdf(X[:3]))
    finally:
        M.set_logpdf_form("auto")
    assert np.array_equal(bits(two), bits(four))
    assert np.all(np.abs(four - ref[:3]) <= tol[:3])


def test_graph_replay_alternating_batches(gpu):
    """50 launches back to back from one graph, two input batches taking turns: a chunk of one launch read from a slot that the next
    launch's up-front requests had already refilled would show as a result that is not the eager one of its batch"""
    import torch

    n, B = 256, 512
    mu, sigma, X0, _, _ = raw_problem(n, B)
    X1 = S.sample_chains(mu, sigma, B, seed=977)
    lik = M.MvnLikelihood.from_covariance(mu, sigma, device=0)
    X = [torch.as_tensor(x, device=gpu) for x in (X0, X1)]
    eager = [lik.logpdf(x).cpu().numpy() for x in X]
    assert not np.array_equal(bits(eager[0]), bits(eager[1]))
    ll = [torch.zeros(B, dtype=torch.float64, device=gpu) for _ in range(2)]
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        lik.logpdf_into(X[0], ll[0])
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        for i in range(50):
            lik.logpdf_into(X[i & 1], ll[i & 1])
    for rep in range(4):
        for o in ll:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for i in range(2):
            assert np.array_equal(bits(ll[i].cpu().numpy()), bits(eager[i])), (rep, i)


def test_non_finite_row(gpu):
    """a non-finite x poisons its own chain only, also when the value sits in a row block whose x is loaded with the others"""
    mu, sigma, X, _, _ = raw_problem(256, 512)
    lik = M.MvnLikelihood.from_covariance(mu, sigma)
    Xb = X[:5].copy()
    Xb[2, 100] = np.inf
    M.set_logpdf_form("sweep")
    try:
        good = np.asarray(lik.logpdf(X[:5]))
        bad = np.asarray(lik.logpdf(Xb))
    finally:
        M.set_logpdf_form("auto")
    assert np.isnan(bad[2])
    keep = [0, 1, 3, 4]
    assert np.isfinite(good).all() and np.array_equal(bits(bad[keep]), bits(good[keep]))
