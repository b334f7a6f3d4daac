"""The prologue of the stripe kernel (csrc/stripe_device.hpp: k_logpdf_stripe): x, mu and 1/diag are loaded once per workgroup -- row
block k by stripe wave k mod S -- and r = x - mu, t = r / diag go to the other waves through an exchange area in LDS behind one barrier
(MCD_STRIPE_PROLOGUE = 1, the default), or every wave loads them for itself (MCD_STRIPE_PROLOGUE = 0, the form before).  Both form r and
t with the same operations and every addition keeps its operands and its order, so everything here is bit for bit: shared against
private at every size at which the code takes another path, launches that alternate two batches (stale exchange contents), non-finite
values in rows another wave owns, and the window's default.  mcd_set_option("MCD_FSTREAM", 3) under form "sweep" forces the stream
outside its window, as in tests/test_gpu_stripe_inverse.py."""
import functools

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

NS = (129, 140, 192, 193, 241, 256)       # R = 3 (stripe wave 3 owns no row block) and R = 4; early-stopping sweeps; a padded last row block
BATCHES = (1, 2, 3, 129)                  # an odd batch: the last workgroup has one real chain
CHAINS = 130


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@functools.lru_cache(maxsize=None)
def problem(n):
    mu, sigma = S.random_spd_problem(n, seed=7 * n)
    X = S.sample_chains(mu, sigma, CHAINS, seed=n + 2)
    for a in (mu, sigma, X):
        a.setflags(write=False)
    return mu, sigma, X


@functools.lru_cache(maxsize=None)
def handle(n):
    mu, sigma, _ = problem(n)
    return M.MvnLikelihood.from_covariance(mu, sigma, device=0)


def stripe(knobs, n, X, prologue):
    """X through the stripe kernel with the shared (1) or the private (0) prologue, or the default (None)"""
    lik = handle(n)
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_PROLOGUE", prologue)
    lik.set_form("sweep")
    try:
        return np.asarray(lik.logpdf(np.ascontiguousarray(X)))
    finally:
        lik.set_form("auto")


_PRIVATE = {}


def private(knobs, n):
    """the 130 chains with every wave loading for itself: the reference of every test, computed once per size"""
    if n not in _PRIVATE:
        out = stripe(knobs, n, problem(n)[2], 0)
        assert np.isfinite(out).all()
        out.setflags(write=False)
        _PRIVATE[n] = out
    return _PRIVATE[n]


# 1. shared against private at every size and batch
@pytest.mark.parametrize("n", NS)
def test_prologue_sizes(gpu, n, knobs):
    _, _, X = problem(n)
    ref = private(knobs, n)
    for B in BATCHES:
        one = stripe(knobs, n, X[:B], 1)
        zero = stripe(knobs, n, X[:B], 0)
        assert np.array_equal(bits(one), bits(zero)), (n, B)
        assert np.array_equal(bits(one), bits(ref[:B])), (n, B)
    assert np.array_equal(bits(stripe(knobs, n, X, 1)), bits(ref))      # 130 chains: more than one workgroup per XCD, none padded


# 2. two batches that differ in every row block, launched alternately: the exchange area of a launch holds the other batch's r and t
@pytest.mark.parametrize("n,B", [(129, 3), (256, 130)])
def test_prologue_alternating_launches(gpu, n, B, knobs):
    import torch

    _, sigma, X0 = problem(n)
    X0 = X0[:B]
    X1 = np.ascontiguousarray(X0[::-1] + 0.125 * np.sqrt(np.diag(sigma)))
    assert all((X0[:, 64 * k:64 * k + 64] != X1[:, 64 * k:64 * k + 64]).any() for k in range((n + 63) // 64))
    alone = [private(knobs, n)[:B], stripe(knobs, n, X1, 0)]
    assert not np.array_equal(bits(alone[0]), bits(alone[1]))
    assert np.array_equal(bits(stripe(knobs, n, X1, 1)), bits(alone[1]))
    lik = handle(n)
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_PROLOGUE", "1")
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


# 3. Inf or NaN in one chain of a pair, at the first and the last row of every row block (each is loaded by one wave and read by the
#    others): the partner chain and every other chain keep their bits
@pytest.mark.parametrize("n", NS)
def test_prologue_non_finite_rows(gpu, n, knobs):
    _, _, X = problem(n)
    ref = private(knobs, n)
    B = 41                                                               # the last chain has a workgroup to itself
    Xb = X[:B].copy()
    poisoned = []
    chain = 2
    for k in range((n + 63) // 64):
        for row, v in ((64 * k, np.inf), (min(64 * k + 63, n - 1), np.nan)):
            Xb[chain, row] = v                                           # an even position ...
            Xb[chain + 3, row] = -v if np.isinf(v) else v                # ... and an odd one, in another pair
            poisoned += [chain, chain + 3]
            chain += 4
    assert chain + 3 < B - 1
    Xb[B - 1, n - 1] = np.nan
    poisoned.append(B - 1)
    keep = np.setdiff1d(np.arange(B), poisoned)
    for prologue in (1, 0):
        bad = stripe(knobs, n, Xb, prologue)
        assert not np.isfinite(bad[poisoned]).any(), prologue
        assert np.array_equal(bits(bad[keep]), bits(ref[:B][keep])), prologue


# 4. a device-resident X with a padded leading dimension whose padding is NaN
@pytest.mark.parametrize("n,B", [(140, 3), (193, 129), (256, 130)])
def test_prologue_device_resident_padded(gpu, n, B, knobs):
    import torch

    _, _, X = problem(n)
    ref = private(knobs, n)
    lik = handle(n)
    ld = n + 3
    Xd = torch.full((B, ld), np.nan, dtype=torch.float64, device=gpu)
    Xd[:, :n] = torch.as_tensor(X[:B], device=gpu)
    out = torch.zeros(B, dtype=torch.float64, device=gpu)
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_PROLOGUE", "1")
    lik.set_form("sweep")
    try:
        M._capi.check(M._capi.lib().mcd_mvn_logpdf_batch(lik._h, Xd.data_ptr(), ld, B, 1, None, out.data_ptr()))
        torch.cuda.synchronize()
    finally:
        lik.set_form("auto")
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref[:B]))


# 5. the window's default (240 < N <= 256, 129 .. 512 chains, form auto) is the shared prologue
def test_prologue_default_is_shared(gpu, knobs):
    _, _, X = problem(256)
    ref = private(knobs, 256)
    knobs.delenv("MCD_FSTREAM")
    knobs.delenv("MCD_STRIPE_PROLOGUE")
    assert M.get_option("MCD_STRIPE_PROLOGUE") is None
    lik = handle(256)
    auto = np.asarray(lik.logpdf(X))
    knobs.setenv("MCD_STRIPE_PROLOGUE", "1")
    one = np.asarray(lik.logpdf(X))
    assert np.array_equal(bits(auto), bits(one)) and np.array_equal(bits(auto), bits(ref))
