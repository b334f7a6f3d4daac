"""The stripe geometry of the inverse stream (csrc/stripe_device.hpp: k_logpdf_stripe): z = W (x - mu) with every wave of a workgroup
multiplying a share of W of its own, loaded by that wave into LDS that only it reads, two chains per workgroup, one barrier at the end.
It is held to the substitution sweep by tolerance (1e-12 relative, the bound between forms) and to the CPU oracle by the project's
bound for synthetic problems (both as in tests/test_gpu_inverse_stream.py); everything else is bit for bit: a chain's value does not
depend on the batch, on its place in the batch (first or second chain of its workgroup), on its neighbour being non-finite, on host
against device-resident input, or on the launch (eager, graph replay, what ran before).  mcd_set_option("MCD_FSTREAM", 3) under form
"sweep" forces the stream outside the window in which it is the default.

Bit policy of the number of stripe waves: it is a build-time constant (csrc/stripe_device.hpp: kStripeWaves); the library holds one
kernel per R, so there is no run-time knob that could change a bit."""
import functools

import numpy as np
import pytest

import mcmc_date_amd as M
import oracle as O
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
NS = (129, 140, 192, 193, 241, 256)       # the first R = 3 size, early-stopping sweeps, both sides of the R = 3 / 4 edge, the window
BATCHES = (1, 2, 3, 129, 512)             # an odd batch: the last workgroup has one real chain
LN_SQRT_2PI = 0.9189385332046727


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@functools.lru_cache(maxsize=None)
def problem(n):
    """operands, 512 chains, the oracle's values and the bound 64 N eps cond(Sigma) max(1, q) of tests/test_gpu_parity.py"""
    mu, sigma = S.random_spd_problem(n, seed=5 * n)
    P = np.linalg.inv(sigma)
    logdet = np.linalg.slogdet(sigma)[1]
    X = S.sample_chains(mu, sigma, 512, seed=n + 1)
    ref = O.logpdf_full_batch(mu, P, logdet, X)
    q = -2.0 * (ref + LN_SQRT_2PI * n) - logdet
    for a in (mu, sigma, X, ref):
        a.setflags(write=False)
    return mu, sigma, X, ref, 64 * n * EPS * np.linalg.cond(sigma) * np.maximum(1.0, q)


@functools.lru_cache(maxsize=None)
def handle(n):
    mu, sigma, _, _, _ = problem(n)
    return M.MvnLikelihood.from_covariance(mu, sigma, device=0)


def sweep(lik, X):
    """the handle's form "sweep": substitution, or the inverse stream under MCD_FSTREAM = 3"""
    lik.set_form("sweep")
    try:
        return np.asarray(lik.logpdf(X))
    finally:
        lik.set_form("auto")


@functools.lru_cache(maxsize=None)
def stripe_all(n):
    """the 512 chains through the stripe kernel (called with the knob set)"""
    return sweep(handle(n), problem(n)[2])


# 1. against the substitution sweep and the oracle; a chain's bits across the batches
@pytest.mark.parametrize("n", NS)
def test_stripe_values_and_batches(gpu, n, knobs):
    mu, sigma, X, ref, tol = problem(n)
    lik = handle(n)
    sub = sweep(lik, X)
    knobs.setenv("MCD_FSTREAM", "3")
    full = stripe_all(n)
    print(n, "max |stripe - oracle|", np.abs(full - ref).max(), "bound", tol.min(), "max rel stripe - substitution", rel(full, sub).max())
    assert np.all(np.abs(full - ref) <= tol)
    assert np.max(rel(full, sub)) <= 1e-12
    if n == 256:
        assert not np.array_equal(bits(full), bits(sub))                 # really the other algebra
    for B in BATCHES:
        assert np.array_equal(bits(sweep(lik, X[:B])), bits(full[:B])), (n, B)


# 2. a permutation of the batch rows that moves chains between even and odd positions
@pytest.mark.parametrize("n", NS)
def test_stripe_position_in_the_batch(gpu, n, knobs):
    _, _, X, _, _ = problem(n)
    knobs.setenv("MCD_FSTREAM", "3")
    full = stripe_all(n)
    perm = np.roll(np.arange(129), 1)                                    # every chain changes parity; the last workgroup's chain too
    perm[[5, 40]] = perm[[40, 5]]
    got = sweep(handle(n), X[perm])
    assert np.array_equal(bits(got), bits(full[perm]))


# 3. a NaN or Inf in chain 2 i leaves chain 2 i + 1, and every other chain, with its bits
@pytest.mark.parametrize("n", NS)
def test_stripe_non_finite_neighbour(gpu, n, knobs):
    _, _, X, _, _ = problem(n)
    knobs.setenv("MCD_FSTREAM", "3")
    full = stripe_all(n)
    Xb = X[:129].copy()
    Xb[2, n // 2] = np.inf
    Xb[6, 0] = np.nan
    Xb[9, n - 1] = -np.inf                                               # an odd position: its even partner keeps its bits too
    Xb[128, :] = np.inf                                                  # the chain that has a workgroup to itself
    poisoned = [2, 6, 9, 128]
    keep = np.setdiff1d(np.arange(129), poisoned)
    bad = sweep(handle(n), Xb)
    assert not np.isfinite(bad[poisoned]).any()
    assert np.array_equal(bits(bad[keep]), bits(full[keep]))


# 4. two different batches launched alternately, eagerly and through a captured graph: stale ring contents, a launch that ends with
#    DMA in flight
@pytest.mark.parametrize("n,B", [(129, 3), (192, 129), (256, 512)])
def test_stripe_alternating_launches(gpu, n, B, knobs):
    import torch

    mu, sigma, X0, _, _ = problem(n)
    X0 = X0[:B]
    X1 = X0[::-1] + 0.125 * np.sqrt(np.diag(sigma))
    lik = handle(n)
    knobs.setenv("MCD_FSTREAM", "3")
    alone = [stripe_all(n)[:B], sweep(lik, np.ascontiguousarray(X1))]
    assert not np.array_equal(bits(alone[0]), bits(alone[1]))
    lik.set_form("sweep")
    try:
        X = [torch.as_tensor(np.ascontiguousarray(x), device=gpu) for x in (X0, X1)]
        ll = [torch.zeros(B, dtype=torch.float64, device=gpu) for _ in range(2)]
        for i in range(6):                                               # eagerly, back to back on one stream
            lik.logpdf_into(X[i & 1], ll[i & 1])
        torch.cuda.synchronize()
        for i in range(2):
            assert np.array_equal(bits(ll[i].cpu().numpy()), bits(alone[i])), ("eager", i)
        st = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(st):
            lik.logpdf_into(X[0], ll[0])
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for i in range(20):
                lik.logpdf_into(X[i & 1], ll[i & 1])
        for rep in range(3):
            for o in ll:
                o.zero_()
            g.replay()
            torch.cuda.synchronize()
            for i in range(2):
                assert np.array_equal(bits(ll[i].cpu().numpy()), bits(alone[i])), ("graph", rep, i)
    finally:
        lik.set_form("auto")


# 5. host pointer against device-resident input with a padded leading dimension
@pytest.mark.parametrize("n,B", [(140, 3), (193, 129), (256, 512)])
def test_stripe_device_resident_padded(gpu, n, B, knobs):
    import torch

    _, _, X, _, _ = problem(n)
    knobs.setenv("MCD_FSTREAM", "3")
    full = stripe_all(n)
    lik = handle(n)
    ld = n + 3
    Xd = torch.full((B, ld), np.nan, dtype=torch.float64, device=gpu)
    Xd[:, :n] = torch.as_tensor(X[:B], device=gpu)
    out = torch.zeros(B, dtype=torch.float64, device=gpu)
    lik.set_form("sweep")
    try:
        M._capi.check(M._capi.lib().mcd_mvn_logpdf_batch(lik._h, Xd.data_ptr(), ld, B, 1, None, out.data_ptr()))
        torch.cuda.synchronize()
    finally:
        lik.set_form("auto")
    assert np.array_equal(bits(out.cpu().numpy()), bits(full[:B]))


# 6. the window's default is this kernel, whatever MCD_LOADERS says
def test_stripe_is_the_window_default(gpu, knobs):
    _, _, X, _, _ = problem(256)
    lik = handle(256)
    auto = np.asarray(lik.logpdf(X))
    knobs.setenv("MCD_LOADERS", "2")
    two = np.asarray(lik.logpdf(X))
    knobs.delenv("MCD_LOADERS")
    knobs.setenv("MCD_FSTREAM", "3")
    assert np.array_equal(bits(auto), bits(stripe_all(256))) and np.array_equal(bits(two), bits(auto))
