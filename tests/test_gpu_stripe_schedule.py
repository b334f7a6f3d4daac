"""The schedule of the stripe kernel (csrc/stripe_device.hpp: k_logpdf_stripe): MCD_STRIPE_SCHED = 1, the default, reads the column
broadcasts of r out of the exchange area in LDS instead of selecting lanes, and reads the units and broadcasts of group g + 1 before it
multiplies group g; MCD_STRIPE_SCHED = 0 keeps the loop of the round before, and the private prologue (MCD_STRIPE_PROLOGUE = 0) has that
loop only.  No addition changes its operands or its place, so everything here is bit for bit: the schedules against each other at every
size at which the code takes another path, two factors launched alternately (a ring read before its covering wait would return the
other factor's unit of the launch before, an exchange read before the barrier the other launch's r), non-finite values in rows
another wave loaded, and the window's default.
mcd_set_option("MCD_FSTREAM", 3) under form "sweep" forces the stream outside its window, as in tests/test_gpu_stripe_prologue.py."""
import functools

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

NS = (129, 140, 192, 193, 241, 256)       # R = 3 and R = 4; early-stopping sweeps; a padded last row block
BATCHES = (1, 2, 3, 130)                  # one real chain in the last workgroup; more than one workgroup per XCD
CHAINS = 130


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@functools.lru_cache(maxsize=None)
def problem(n, other=0):
    mu, sigma = S.random_spd_problem(n, seed=7 * n + other)
    X = S.sample_chains(mu, sigma, CHAINS, seed=n + 2 + other)
    for a in (mu, sigma, X):
        a.setflags(write=False)
    return mu, sigma, X


@functools.lru_cache(maxsize=None)
def handle(n, other=0):
    mu, sigma, _ = problem(n, other)
    return M.MvnLikelihood.from_covariance(mu, sigma, device=0)


def stripe(knobs, n, X, sched, prologue=1, other=0):
    """X through the stripe kernel under schedule sched (None: the default) with the shared (1) or the private (0) prologue"""
    lik = handle(n, other)
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_SCHED", sched)
    knobs.setenv("MCD_STRIPE_PROLOGUE", prologue)
    lik.set_form("sweep")
    try:
        return np.asarray(lik.logpdf(np.ascontiguousarray(X)))
    finally:
        lik.set_form("auto")


_OLD = {}


def old(knobs, n, other=0):
    """the 130 chains under the schedule of the round before (shared prologue): the reference of every test, computed once per factor"""
    if (n, other) not in _OLD:
        out = stripe(knobs, n, problem(n, other)[2], 0, other=other)
        assert np.isfinite(out).all()
        out.setflags(write=False)
        _OLD[n, other] = out
    return _OLD[n, other]


# 1. the new schedule against the old one and against the private prologue, at every size and batch
@pytest.mark.parametrize("n", NS)
def test_schedules_agree(gpu, n, knobs):
    _, _, X = problem(n)
    ref = old(knobs, n)
    for B in BATCHES:
        new = stripe(knobs, n, X[:B], 1)
        zero = stripe(knobs, n, X[:B], 0)
        private = stripe(knobs, n, X[:B], 1, prologue=0)
        assert np.array_equal(bits(new), bits(zero)), (n, B)
        assert np.array_equal(bits(new), bits(private)), (n, B)
        assert np.array_equal(bits(new), bits(ref[:B])), (n, B)


# 2. two factors of one size launched alternately on one stream: every ring slot of a launch holds the other factor's unit
@pytest.mark.parametrize("n", (129, 256))
def test_stale_ring(gpu, n, knobs):
    import torch

    B = CHAINS
    alone = [old(knobs, n, o) for o in (0, 1)]
    assert not np.array_equal(bits(alone[0]), bits(alone[1]))
    for o in (0, 1):
        assert np.array_equal(bits(stripe(knobs, n, problem(n, o)[2], 1, other=o)), bits(alone[o]))
    liks = [handle(n, o) for o in (0, 1)]
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_SCHED", "1")
    knobs.setenv("MCD_STRIPE_PROLOGUE", "1")
    for lik in liks:
        lik.set_form("sweep")
    try:
        X = [torch.as_tensor(np.ascontiguousarray(problem(n, o)[2]), device=gpu) for o in (0, 1)]
        ll = [torch.zeros(B, dtype=torch.float64, device=gpu) for _ in range(2)]
        for i in range(6):                                               # eagerly, back to back on one stream
            liks[i & 1].logpdf_into(X[i & 1], ll[i & 1])
        torch.cuda.synchronize()
        for i in range(2):
            assert np.array_equal(bits(ll[i].cpu().numpy()), bits(alone[i])), ("eager", i)
        st = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(st):
            for i in range(2):
                liks[i].logpdf_into(X[i], ll[i])
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for i in range(6):
                liks[i & 1].logpdf_into(X[i & 1], ll[i & 1])
        for rep in range(2):
            for o in ll:
                o.zero_()
            g.replay()
            torch.cuda.synchronize()
            for i in range(2):
                assert np.array_equal(bits(ll[i].cpu().numpy()), bits(alone[i])), ("graph", rep, i)
    finally:
        for lik in liks:
            lik.set_form("auto")


# 3. Inf or NaN in one chain of a pair, in every row block (each is loaded by one wave and read by the others): the neighbouring chain
#    keeps its bits under both schedules and the bad chain is non-finite under both
@pytest.mark.parametrize("n", (193, 256))
def test_non_finite_neighbour(gpu, n, knobs):
    _, _, X = problem(n)
    ref = old(knobs, n)
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
    keep = np.setdiff1d(np.arange(B), poisoned)
    assert all(c ^ 1 in keep for c in poisoned)                          # every bad chain's neighbour is a good one
    for sched in (1, 0):
        bad = stripe(knobs, n, Xb, sched)
        assert not np.isfinite(bad[poisoned]).any(), sched
        assert np.array_equal(bits(bad[keep]), bits(ref[:B][keep])), sched


# 4. the window's default (240 < N <= 256, 129 .. 512 chains, form auto) is the new schedule
@pytest.mark.parametrize("B", (129, 512))
def test_window_default(gpu, B, knobs):
    mu, sigma, _ = problem(256)
    X = S.sample_chains(mu, sigma, B, seed=11)
    lik = handle(256)
    knobs.setenv("MCD_STRIPE_SCHED", "1")
    one = np.asarray(lik.logpdf(X))
    knobs.setenv("MCD_STRIPE_SCHED", "0")
    zero = np.asarray(lik.logpdf(X))
    knobs.delenv("MCD_STRIPE_SCHED")
    knobs.delenv("MCD_FSTREAM")
    knobs.delenv("MCD_STRIPE_PROLOGUE")
    assert M.get_option("MCD_STRIPE_SCHED") is None
    auto = np.asarray(lik.logpdf(X))
    assert np.isfinite(auto).all()
    assert np.array_equal(bits(auto), bits(one)) and np.array_equal(bits(auto), bits(zero))
    assert M.get_option("MCD_STRIPE_SCHED") is None
