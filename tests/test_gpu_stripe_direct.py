"""Schedule 2 of the stripe kernel (csrc/stripe_device.hpp, csrc/stripe_plan.hpp: k_logpdf_stripe<R, S, true, 2>): the off-diagonal
units of the inverse stream go straight from memory into the registers that multiply them, the diagonal parts stay on LDS-DMA, and
one plan counts the waits over both kinds.  No operand and no order of an addition changes, so everything here is bit for bit.
Schedule 2 runs whole sweeps only (stripe_plan.hpp: stripe_schedule): of the sizes below 177, 192 (R = 3), 241 and 256 (R = 4)
launch it, and at 129, 140 and 193, where the sweep stops early, MCD_STRIPE_SCHED = 2 launches schedule 1.  Every test asks the
library which kernel its launches take (launched()), so a size that is meant to exercise schedule 2 cannot pass on another kernel.
The cases: schedule 2 against schedules 1 and 0 and against the private prologue at every size at which the code takes another path;
two factors launched alternately (a register slot or ring slot read before its covering wait would return the other factor's unit);
non-finite values in rows another wave loaded; the window's default.  The helpers follow tests/test_gpu_stripe_schedule.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

NS = (129, 140, 177, 192, 193, 241, 256)  # R = 3 and R = 4; early-stopping sweeps; a padded last row block
WHOLE = (177, 192, 241, 256)              # the sizes whose sweep does not stop early: schedule 2's kernel runs there
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


def launched(n):
    """the kernel a stripe launch at size n takes under the options as they stand: -1 the private prologue, 0 .. 2 the schedule"""
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_schedule_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int]
    return f((n + 63) // 64, 16 * ((n + 15) // 16))


def stripe(knobs, n, X, sched, prologue=1, other=0):
    """X through the stripe kernel under schedule sched with the shared (1) or the private (0) prologue"""
    lik = handle(n, other)
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_SCHED", sched)
    knobs.setenv("MCD_STRIPE_PROLOGUE", prologue)
    want = -1 if int(prologue) == 0 else int(sched) if int(sched) != 2 or n in WHOLE else 1
    assert launched(n) == want, (n, sched, prologue, launched(n))
    lik.set_form("sweep")
    try:
        return np.asarray(lik.logpdf(np.ascontiguousarray(X)))
    finally:
        lik.set_form("auto")


_OLD = {}


def old(knobs, n, other=0):
    """the 130 chains under schedule 0 (shared prologue): the reference of every test, computed once per factor"""
    if (n, other) not in _OLD:
        out = stripe(knobs, n, problem(n, other)[2], 0, other=other)
        assert np.isfinite(out).all()
        out.setflags(write=False)
        _OLD[n, other] = out
    return _OLD[n, other]


# 1. schedule 2 against 1 and 0 and against the private prologue, at every size and batch
@pytest.mark.parametrize("n", NS)
def test_schedules_agree(gpu, n, knobs):
    _, _, X = problem(n)
    ref = old(knobs, n)
    for B in BATCHES:
        two = stripe(knobs, n, X[:B], 2)
        one = stripe(knobs, n, X[:B], 1)
        zero = stripe(knobs, n, X[:B], 0)
        private = stripe(knobs, n, X[:B], 2, prologue=0)
        assert np.array_equal(bits(two), bits(one)), (n, B)
        assert np.array_equal(bits(two), bits(zero)), (n, B)
        assert np.array_equal(bits(two), bits(private)), (n, B)
        assert np.array_equal(bits(two), bits(ref[:B])), (n, B)


# 2. two factors of one size launched alternately on one stream: every register slot and ring slot of a launch held the other factor's
#    unit.  192 (R = 3) and 256 (R = 4) run schedule 2's kernels; 129 stops early and runs schedule 1 under the same option.
@pytest.mark.parametrize("n", (129, 192, 256))
def test_stale_slots(gpu, n, knobs):
    import torch

    B = CHAINS
    alone = [old(knobs, n, o) for o in (0, 1)]
    assert not np.array_equal(bits(alone[0]), bits(alone[1]))
    for o in (0, 1):
        assert np.array_equal(bits(stripe(knobs, n, problem(n, o)[2], 2, other=o)), bits(alone[o]))
    liks = [handle(n, o) for o in (0, 1)]
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_SCHED", "2")
    knobs.setenv("MCD_STRIPE_PROLOGUE", "1")
    assert launched(n) == (2 if n in WHOLE else 1)
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
#    keeps its bits and the bad chain is non-finite.  192 (R = 3) and 256 (R = 4) run schedule 2's kernels, 193 stops early (schedule 1).
@pytest.mark.parametrize("n", (192, 193, 256))
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
    for sched in (2, 1):
        bad = stripe(knobs, n, Xb, sched)
        assert not np.isfinite(bad[poisoned]).any(), sched
        assert np.array_equal(bits(bad[keep]), bits(ref[:B][keep])), sched


# 4. the window's default (240 < N <= 256, 129 .. 512 chains, form auto) computes what every schedule computes
@pytest.mark.parametrize("B", (129, 512))
def test_window_default(gpu, B, knobs):
    mu, sigma, _ = problem(256)
    X = S.sample_chains(mu, sigma, B, seed=11)
    lik = handle(256)
    out = {}
    for sched in ("2", "1", "0"):
        knobs.setenv("MCD_STRIPE_SCHED", sched)
        out[sched] = np.asarray(lik.logpdf(X))
    knobs.delenv("MCD_STRIPE_SCHED")
    knobs.delenv("MCD_FSTREAM")
    knobs.delenv("MCD_STRIPE_PROLOGUE")
    assert M.get_option("MCD_STRIPE_SCHED") is None
    assert launched(256) == 2                                            # the default is schedule 2's kernel
    auto = np.asarray(lik.logpdf(X))
    assert np.isfinite(auto).all()
    for sched in out:
        assert np.array_equal(bits(auto), bits(out[sched])), sched
    assert M.get_option("MCD_STRIPE_SCHED") is None
