"""The per-chain finish of the stripe kernel (csrc/stripe_device.hpp: k_logpdf_stripe_fin, MCD_STRIPE_FINISH = 1, the default where
schedule 2 runs): behind the hand-over barrier each of the workgroup's two chains is finished by a wave of its own, and c and logdet
are fetched at entry.  MCD_STRIPE_FINISH = 0 keeps wave 0 finishing both.  No operand
and no order of an addition changes, so everything here is bit for bit.  Every launch that is meant to take the new finish asks the
library which one it takes (finish()), so no case can pass on the other kernel.  What the change could newly break is a chain's place
in its workgroup -- the two chains are finished by different waves --, a hand-over slot read before the barrier, and the chain beyond
the batch.  The helpers follow tests/test_gpu_stripe_direct.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

NS = (177, 192, 241, 256)                 # R = 3 and R = 4, whole sweeps (schedule 2); 177 and 241 have a padded last row block
BATCHES = (1, 2, 3, 130)                  # a workgroup whose second chain is beyond the batch; more than one workgroup per XCD
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


def _hook(name, n):
    f = getattr(C.CDLL(M._capi.LIB_PATH), name)
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int]
    return f((n + 63) // 64, 16 * ((n + 15) // 16))


def finish(n):
    """the finish a stripe launch at size n takes under the options as they stand: 1 a wave per chain, 0 wave 0 alone"""
    return _hook("mcd_stripe_finish_selftest_", n)


def launched(n):
    """... and its kernel: -1 the private prologue, 0 .. 2 the schedule"""
    return _hook("mcd_stripe_schedule_selftest_", n)


def stripe(knobs, n, X, fin, sched=2, prologue=1, other=0):
    """X through the stripe kernel under MCD_STRIPE_FINISH = fin, schedule sched and the shared (1) or the private (0) prologue"""
    lik = handle(n, other)
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_SCHED", sched)
    knobs.setenv("MCD_STRIPE_PROLOGUE", prologue)
    knobs.setenv("MCD_STRIPE_FINISH", fin)
    whole = int(prologue) != 0 and int(sched) == 2
    assert launched(n) == (-1 if int(prologue) == 0 else int(sched)), (n, sched, prologue)
    assert finish(n) == (1 if whole and int(fin) != 0 else 0), (n, fin, sched, prologue, finish(n))
    lik.set_form("sweep")
    try:
        return np.asarray(lik.logpdf(np.ascontiguousarray(X)))
    finally:
        lik.set_form("auto")


_OLD = {}


def old(knobs, n, other=0):
    """the 130 chains under the old finish (schedule 2, shared prologue): the reference of every test, computed once per factor"""
    if (n, other) not in _OLD:
        out = stripe(knobs, n, problem(n, other)[2], 0, other=other)
        assert np.isfinite(out).all()
        out.setflags(write=False)
        _OLD[n, other] = out
    return _OLD[n, other]


# 1. the new finish against the old one, against schedules 1 and 0 and against the private prologue, at every size and batch
@pytest.mark.parametrize("n", NS)
def test_new_against_old(gpu, n, knobs):
    _, _, X = problem(n)
    ref = old(knobs, n)
    for B in BATCHES:
        new = stripe(knobs, n, X[:B], 1)
        assert np.array_equal(bits(new), bits(stripe(knobs, n, X[:B], 0))), (n, B)
        assert np.array_equal(bits(new), bits(stripe(knobs, n, X[:B], 1, sched=1))), (n, B)
        assert np.array_equal(bits(new), bits(stripe(knobs, n, X[:B], 1, sched=0))), (n, B)
        assert np.array_equal(bits(new), bits(stripe(knobs, n, X[:B], 1, prologue=0))), (n, B)
        assert np.array_equal(bits(new), bits(ref[:B])), (n, B)


# 2. a chain's place in its workgroup: the same vector in both places gives the same bits, and a batch shifted by one chain -- every
#    chain changes its place and its finishing wave -- gives each chain the bits it had
@pytest.mark.parametrize("n", NS)
def test_place_in_the_workgroup(gpu, n, knobs):
    _, _, X = problem(n)
    ref = old(knobs, n)
    twice = np.repeat(X[:33], 2, axis=0)                                 # rows 2 i and 2 i + 1 are chain i
    out = stripe(knobs, n, twice, 1)
    assert np.array_equal(bits(out[0::2]), bits(out[1::2])), n
    assert np.array_equal(bits(out[0::2]), bits(ref[:33])), n
    for B in (2, 3, CHAINS):                                             # X[1:B]: an even and an odd number of chains
        assert np.array_equal(bits(stripe(knobs, n, X[1:B], 1)), bits(ref[1:B])), (n, B)


# 3. two factors of one size launched alternately on one stream, under both finishes: a hand-over slot read before the barrier would
#    return the other factor's partial sums (or, under the other finish, the other layout's)
@pytest.mark.parametrize("n", (192, 256))
def test_stale_hand_over(gpu, n, knobs):
    import torch

    B = CHAINS
    alone = [old(knobs, n, o) for o in (0, 1)]
    assert not np.array_equal(bits(alone[0]), bits(alone[1]))
    for o in (0, 1):
        assert np.array_equal(bits(stripe(knobs, n, problem(n, o)[2], 1, other=o)), bits(alone[o]))
    liks = [handle(n, o) for o in (0, 1)]
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_SCHED", "2")
    knobs.setenv("MCD_STRIPE_PROLOGUE", "1")
    for lik in liks:
        lik.set_form("sweep")
    try:
        X = [torch.as_tensor(np.ascontiguousarray(problem(n, o)[2]), device=gpu) for o in (0, 1)]
        ll = [torch.zeros(B, dtype=torch.float64, device=gpu) for _ in range(4)]
        for i in range(12):                                              # eagerly, back to back: factor i & 1, finish (i >> 1) & 1
            knobs.setenv("MCD_STRIPE_FINISH", (i >> 1) & 1)
            assert finish(n) == (i >> 1) & 1 and launched(n) == 2
            liks[i & 1].logpdf_into(X[i & 1], ll[i & 3])
        torch.cuda.synchronize()
        for j in range(4):
            assert np.array_equal(bits(ll[j].cpu().numpy()), bits(alone[j & 1])), ("eager", j)
        st = torch.cuda.Stream(device=gpu)
        knobs.setenv("MCD_STRIPE_FINISH", "1")
        assert finish(n) == 1
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


# 4. Inf and NaN in the second chain of a workgroup only, in row block 2, which neither finishing wave loaded or owns: the first chain
#    keeps its finite bits and the second has the old finish's bits
@pytest.mark.parametrize("n", (192, 256))
def test_non_finite_second_chain(gpu, n, knobs):
    _, _, X = problem(n)
    ref = old(knobs, n)
    B = 9
    Xb = X[:B].copy()
    Xb[3, 128] = np.inf
    Xb[5, min(191, n - 1)] = np.nan
    Xb[7, 130] = -np.inf
    bad = [3, 5, 7]
    keep = np.setdiff1d(np.arange(B), bad)
    want = stripe(knobs, n, Xb, 0)
    got = stripe(knobs, n, Xb, 1)
    assert not np.isfinite(want[bad]).any()
    assert np.array_equal(bits(got), bits(want)), n
    assert np.array_equal(bits(got[keep]), bits(ref[:B][keep])), n


# 5. with nothing set, the window's default (form auto, 129 .. 512 chains, N = 256) takes the new finish and agrees with the
#    substitution sweep to the bound between forms (1e-12 relative: tests/test_gpu_inverse_stream.py)
@pytest.mark.parametrize("B", (129, 512))
def test_window_default(gpu, B, knobs):
    mu, sigma, _ = problem(256)
    X = S.sample_chains(mu, sigma, B, seed=11)
    lik = handle(256)
    knobs.setenv("MCD_STRIPE_FINISH", "0")
    oldfin = np.asarray(lik.logpdf(X))
    for name in ("MCD_STRIPE_FINISH", "MCD_STRIPE_SCHED", "MCD_STRIPE_PROLOGUE", "MCD_FSTREAM"):
        knobs.delenv(name)
        assert M.get_option(name) is None
    assert launched(256) == 2 and finish(256) == 1                       # the default is the new finish on schedule 2's kernel
    auto = np.asarray(lik.logpdf(X))
    assert np.isfinite(auto).all()
    assert np.array_equal(bits(auto), bits(oldfin))
    lik.set_form("sweep")
    try:
        sub = np.asarray(lik.logpdf(X))
    finally:
        lik.set_form("auto")
    assert not np.array_equal(bits(auto), bits(sub))                     # really the other stream
    assert np.max(np.abs(auto - sub) / np.maximum(1.0, np.abs(sub))) <= 1e-12
