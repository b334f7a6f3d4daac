"""k_logpdf_stripe_reg (csrc/stripe_device.hpp: stripe_wave_reg, MCD_STRIPE_DIAG = 1): the per-chain-finish stripe kernel with the
diagonal parts of the inverse stream loaded straight into registers -- a lane above its pair's threshold reads the part at a shifted
address, the other lanes read a unit of zeros that stands behind the stream on the device -- and with no ring in LDS, only the exchange
area and the hand-over of the partial sums.  MCD_STRIPE_DIAG = 0 keeps the ring's kernel.  No operand and no order of an addition
changes, so everything here is bit for bit (uint64 views).  Every launch that is meant to take the new kernel asks the library which
one it takes (diag()), so no case can pass on the other kernel.  What the change could newly break: a lane's address (every size and
batch against three older kernels), the zero lanes (non-finite x where a zero meets it: 0 x inf must stay NaN), the zero unit and the
hand-over area of another factor or size, and a chain's place in its workgroup.  The helpers follow tests/test_gpu_stripe_finish.py."""
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
    mu, sigma = S.random_spd_problem(n, seed=5 * n + other)
    X = S.sample_chains(mu, sigma, CHAINS, seed=n + 3 + other)
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


def diag(n):
    """where a stripe launch at size n takes the diagonal parts from under the options as they stand: 1 register loads, 0 the ring"""
    return _hook("mcd_stripe_diag_selftest_", n)


def diag_at(n, batch):
    """... for that many chains: with MCD_STRIPE_DIAG unset the batch decides"""
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_diag_batch_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_longlong]
    return f((n + 63) // 64, 16 * ((n + 15) // 16), batch)


def finish(n):
    return _hook("mcd_stripe_finish_selftest_", n)


def launched(n):
    return _hook("mcd_stripe_schedule_selftest_", n)


def stripe(knobs, n, X, dg, sched=2, prologue=1, other=0):
    """X through the stripe kernel under MCD_STRIPE_DIAG = dg, schedule sched and the shared (1) or the private (0) prologue"""
    lik = handle(n, other)
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_SCHED", sched)
    knobs.setenv("MCD_STRIPE_PROLOGUE", prologue)
    knobs.setenv("MCD_STRIPE_FINISH", 1)
    knobs.setenv("MCD_STRIPE_DIAG", dg)
    whole = int(prologue) != 0 and int(sched) == 2
    assert launched(n) == (-1 if int(prologue) == 0 else int(sched)), (n, sched, prologue)
    assert finish(n) == (1 if whole else 0) and diag(n) == (1 if whole and int(dg) != 0 else 0), (n, dg, sched, prologue, diag(n))
    lik.set_form("sweep")
    try:
        return np.asarray(lik.logpdf(np.ascontiguousarray(X)))
    finally:
        lik.set_form("auto")


_OLD = {}


def old(knobs, n, other=0):
    """the 130 chains through the ring's kernel (MCD_STRIPE_DIAG = 0): the reference of every test, computed once per factor"""
    if (n, other) not in _OLD:
        out = stripe(knobs, n, problem(n, other)[2], 0, other=other)
        assert np.isfinite(out).all()
        out.setflags(write=False)
        _OLD[n, other] = out
    return _OLD[n, other]


# 1. the new kernel against the ring's, against schedules 1 and 0 and against the private prologue, at every size and batch
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


# 2. non-finite x where a zero lane meets it.  A column's entries on and above the diagonal are zeros the stream does not store: the
#    lanes that would hold them read the zero unit and multiply it, so 0 x inf = NaN reaches those rows as under the ring, where the
#    lanes read a unit of zeros in LDS.  A kernel that skipped the lanes would give -inf or a finite value instead of NaN.  One bad
#    value per chain, the other chain of its workgroup untouched: that one keeps its finite bits.
@pytest.mark.parametrize("n", NS)
def test_non_finite_meets_a_zero_lane(gpu, n, knobs):
    _, _, X = problem(n)
    ref = old(knobs, n)
    B = 14
    Xb = X[:B].copy()
    cases = {1: (n - 1, np.inf),             # the last column: every lane of it is a zero lane
             2: (64 + 5, np.inf),            # a middle row block, the 7-unit part (columns 64 .. 79) ...
             5: (64 + 16 + 5, np.inf),       # ... the 5-unit part ...
             6: (64 + 32 + 5, -np.inf),      # ... the 3-unit part ...
             9: (64 + 48 + 5, np.inf),       # ... and the 1-unit part
             10: (64 + 33, np.nan)}
    for chain, (j, v) in cases.items():
        Xb[chain, j] = v
    bad = sorted(cases)
    keep = np.setdiff1d(np.arange(B), bad)
    assert all((c ^ 1) in keep for c in bad)                             # each bad chain's neighbour in the workgroup is a good one
    want = stripe(knobs, n, Xb, 0)
    got = stripe(knobs, n, Xb, 1)
    assert np.isnan(want[bad]).all()                                     # 0 x inf under the ring: NaN, not an infinity
    assert np.array_equal(bits(got), bits(want)), (n, got[bad], want[bad])
    assert np.array_equal(bits(got[keep]), bits(ref[:B][keep])), n
    assert np.array_equal(bits(got), bits(stripe(knobs, n, Xb, 1, sched=1))), n


# 3. two factors launched alternately on one stream under both values of the option, of one size and of different sizes (R = 3 and
#    R = 4: another zero unit, another hand-over area): a zero unit or a hand-over slot that is stale or misplaced would show
@pytest.mark.parametrize("pair", (((256, 0), (256, 1)), ((192, 0), (256, 0)), ((241, 0), (177, 0))))
def test_alternating_factors(gpu, pair, knobs):
    import torch

    alone = [old(knobs, n, o) for n, o in pair]
    for (n, o), ref in zip(pair, alone):
        assert np.array_equal(bits(stripe(knobs, n, problem(n, o)[2], 1, other=o)), bits(ref))
    liks = [handle(n, o) for n, o in pair]
    knobs.setenv("MCD_FSTREAM", "3")
    knobs.setenv("MCD_STRIPE_SCHED", "2")
    knobs.setenv("MCD_STRIPE_PROLOGUE", "1")
    knobs.setenv("MCD_STRIPE_FINISH", "1")
    for lik in liks:
        lik.set_form("sweep")
    try:
        X = [torch.as_tensor(np.ascontiguousarray(problem(n, o)[2]), device=gpu) for n, o in pair]
        ll = [torch.zeros(CHAINS, dtype=torch.float64, device=gpu) for _ in range(4)]
        for i in range(12):                                              # back to back: factor i & 1, MCD_STRIPE_DIAG = (i >> 1) & 1
            knobs.setenv("MCD_STRIPE_DIAG", (i >> 1) & 1)
            assert all(diag(n) == (i >> 1) & 1 and finish(n) == 1 for n, _ in pair)
            liks[i & 1].logpdf_into(X[i & 1], ll[i & 3])
        torch.cuda.synchronize()
        for j in range(4):
            assert np.array_equal(bits(ll[j].cpu().numpy()), bits(alone[j & 1])), (pair, j)
    finally:
        for lik in liks:
            lik.set_form("auto")


# 4. a chain's place in its workgroup: the same vector in both places gives the same bits, and a batch shifted by one chain -- every
#    chain changes its place and its finishing wave -- gives each chain the bits it had
@pytest.mark.parametrize("n", NS)
def test_place_in_the_workgroup(gpu, n, knobs):
    _, _, X = problem(n)
    ref = old(knobs, n)
    twice = np.repeat(X[:33], 2, axis=0)
    out = stripe(knobs, n, twice, 1)
    assert np.array_equal(bits(out[0::2]), bits(out[1::2])), n
    assert np.array_equal(bits(out[0::2]), bits(ref[:33])), n
    for B in (2, 3, CHAINS):
        assert np.array_equal(bits(stripe(knobs, n, X[1:B], 1)), bits(ref[1:B])), (n, B)


# 5. with nothing set, the window's default (form auto, N = 256) takes the kernel the library reports and has the ring's bits
@pytest.mark.parametrize("B", (129, 512))
def test_window_default(gpu, B, knobs):
    mu, sigma, _ = problem(256)
    X = S.sample_chains(mu, sigma, B, seed=13)
    lik = handle(256)
    knobs.setenv("MCD_STRIPE_DIAG", "0")
    assert diag(256) == 0 and diag_at(256, B) == 0 and finish(256) == 1
    ring = np.asarray(lik.logpdf(X))
    knobs.setenv("MCD_STRIPE_DIAG", "1")
    assert diag(256) == 1 and diag_at(256, B) == 1
    reg = np.asarray(lik.logpdf(X))
    for name in ("MCD_STRIPE_DIAG", "MCD_STRIPE_FINISH", "MCD_STRIPE_SCHED", "MCD_STRIPE_PROLOGUE", "MCD_FSTREAM"):
        knobs.delenv(name)
        assert M.get_option(name) is None
    assert launched(256) == 2 and finish(256) == 1 and diag_at(256, B) in (0, 1) and diag(256) == diag_at(256, 512)
    auto = np.asarray(lik.logpdf(X))
    assert np.isfinite(auto).all()
    assert np.array_equal(bits(auto), bits(ring)) and np.array_equal(bits(reg), bits(ring))
    lik.set_form("sweep")
    try:
        sub = np.asarray(lik.logpdf(X))
    finally:
        lik.set_form("auto")
    assert not np.array_equal(bits(auto), bits(sub))                     # really the inverse stream
