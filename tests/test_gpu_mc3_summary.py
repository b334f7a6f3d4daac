"""Sampler.record_summary_mc3 / mcd_mh_record_summary_mc3: the recorder's summaries under Metropolis-coupled MCMC, where the temperatures
move between the chains of a group and the summary follows ONE temperature through the swaps (csrc/k_mc3_summary.hip gathers the rung's
sequence of every group out of the ring, csrc/k_summary.hip summarises it).

References, all on the arrays that record_fetch returns AFTERWARDS, laid out by test_gpu_mh_summary.quantities:
  * diagnostics.rung_trace / replica_flow, the numpy restatement of the gather and of the flow counts (tests/test_mc3_summary_host.py checks
    it against hand-built tables): holder, visits and round_trips must be EQUAL;
  * diagnostics.trace_summary(device=True) of that trace: the same kernels on the same doubles, so pooled and per_group must be the same
    BITS, NaNs included -- there is no tolerance to choose;
  * diagnostics.summary of that trace under the rules and tolerances of test_gpu_mh_summary.compare (its cap on the quantities left out of
    the effective-sample-size comparison, 2 % of Q, included).  For case 1's seeds the CPU twin (oracle.MhChains under MC3, the same
    schedule and swap draws) leaves 0 of the 42 comparable quantities out, at both rungs.
Every case asserts the launch structure its runs took."""
import ctypes as C
import types

import numpy as np
import pytest

import mcmc_date_amd as M
import test_gpu_mh_summary as TS
from mcmc_date_amd import _capi, monitor
from mcmc_date_amd import diagnostics as D

pytestmark = pytest.mark.gpu

LADDER4 = [1.0, 0.9, 0.8, 0.7]


def make_case(name, B):
    """test_gpu_mh_summary.Case with another number of chains"""
    from mcmc_date_amd import synthetic as S

    case = TS.Case(name)
    if TS.CASES[name][0] == "golden":
        case.s0 = case.s0.slice(0, B)
    else:
        case.s0 = S.random_states(case.topo, B, seed=5)
        case.s0.time_birth_rate = np.full(B, 1.0); case.s0.time_death_rate = np.full(B, 0.8); case.s0.rate_variance = np.full(B, 0.3)
    case.B = B
    return case


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(got, want, label):
    assert np.array_equal(bits(got.pooled), bits(want.pooled)), label
    assert np.array_equal(bits(got.per_chain), bits(want.per_chain)), label


def check_against_fetched(got, fetched, ladder, rung, max_lag, label):
    """(a) and (c): the device's summary, holder and flow against the restatement on the fetched window; returns the rung's trace"""
    x, beta = TS.quantities(fetched), fetched[5]
    tr, holder = D.rung_trace(x, beta, ladder[rung], len(ladder))
    assert got.n_samples == len(x) and got.per_chain.shape == (x.shape[1] // len(ladder), x.shape[2], 4), label
    assert got.holder.dtype == np.int32 and np.array_equal(got.holder, holder), label
    visits, trips = D.replica_flow(beta, ladder)
    assert np.array_equal(got.visits, visits) and np.array_equal(got.round_trips, trips), label
    assert np.array_equal(got.visits.sum(axis=1), np.full(x.shape[1], len(x))), label
    same_bits(got, D.trace_summary(tr, max_lag, device=True, per_chain=True), label)
    return tr, holder


def run_periods(case, mc3s, sched, lo, hi):
    """periods lo .. hi - 1 of two iterations each with a swap phase behind every one, on every (sampler, MC3) pair alike"""
    for k in range(lo, hi):
        for smp, mc3 in mc3s:
            smp.run_schedule(sched[2 * k:2 * k + 2])
            mc3.swap()


def test_cold_and_hottest_sequence_in_a_wrapped_ring(gpu):
    case = make_case("1-chain-lds", 8)
    smp, twin = case.sampler(seed=5), case.sampler(seed=5)
    pairs = [(s, M.MC3(s, n_chains=4, swap_period=2, n_swaps=3, betas=LADDER4, seed=11)) for s in (smp, twin)]
    for s, mc3 in pairs:
        s.record_begin(2, 32)
        for _ in range(24):
            mc3.run(2)
        assert len(s.record_fetch(16)[0]) == 16
        for _ in range(16):
            mc3.run(2)
        case.check_path(s)
        assert s.record_count() == 24                         # slots 16 .. 31, then 0 .. 7
    mc3 = pairs[0][1]
    got = {r: mc3.record_summary(rung=r, skip=1, max_lag=7, per_group=True, flow=True) for r in (0, 3)}
    again = {r: smp.record_summary_mc3(rung=r, skip=1, n=23, max_lag=7, per_group=True, flow=True) for r in (0, 3)}
    ages = monitor.summarize_recorded(smp, burn_in=1 / 24, max_lag=7, rung=0)
    with pytest.raises(_capi.McdError, match="Metropolis-coupled") as e:      # the chains themselves are still refused
        smp.record_summary()
    code = e.value.code
    del e
    assert code == _capi.MCD_ERR_UNSUPPORTED
    assert smp.record_count() == 24
    f, ft = smp.record_fetch(), twin.record_fetch()
    for a, b in zip(f, ft):                                  # (f) nothing a fetch can see was disturbed
        assert np.array_equal(a, b) and len(a) == 24
    assert np.array_equal(f[0], 2 * np.arange(17, 41))
    window = tuple(a[1:] for a in f)
    nn = case.topo.n_nodes
    for r in (0, 3):
        label = f"path 1, rung {r}"
        assert got[r].n_samples == 23 and got[r].max_lag == 7
        tr, holder = check_against_fetched(got[r], window, LADDER4, r, 7, label)                 # (a), (c)
        TS.compare(got[r], tr, 7, label)                                                         # (b)
        for fld in ("pooled", "per_chain"):                                                      # (e)
            assert np.array_equal(bits(getattr(got[r], fld)), bits(getattr(again[r], fld))), (label, fld)
        for fld in ("holder", "visits", "round_trips"):
            assert np.array_equal(getattr(got[r], fld), getattr(again[r], fld)), (label, fld)
    moved = [len(set(got[0].holder[:, g])) > 1 for g in range(2)]                                # (d)
    assert any(moved), "the cold chain of no group changed inside the window (no swap with rung 0 was accepted): the test shows nothing"
    assert not np.array_equal(got[0].pooled[:2 * nn], got[3].pooled[:2 * nn])                    # two rungs, two sequences
    assert np.array_equal(bits(np.stack([ages.mean, ages.variance, ages.minimum, ages.maximum, ages.ci_lower, ages.ci_upper, ages.rhat, ages.ess], axis=1)),
                          bits(got[0].ages[:, :8]))
    for s in (smp, twin):
        s.record_end()


def test_rows_longer_than_a_wave(gpu):
    case = make_case("2-chain-streamed", 6)
    ladder = [1.0, 0.9]
    smp = case.sampler()
    mc3 = M.MC3(smp, n_chains=2, swap_period=2, n_swaps=1, betas=ladder, seed=3)
    nn = case.topo.n_nodes
    assert nn == 257 and 2 * nn + 9 == 8 * 64 + 11
    smp.record_begin(2, 12)
    run_periods(case, [(smp, mc3)], case.schedule(24), 0, 12)
    case.check_path(smp)
    got = {r: smp.record_summary_mc3(rung=r, max_lag=3, per_group=True, flow=True) for r in (0, 1)}
    again = smp.record_summary_mc3(rung=1, max_lag=3, per_group=True, flow=True)
    assert np.array_equal(bits(got[1].pooled), bits(again.pooled)) and np.array_equal(bits(got[1].per_chain), bits(again.per_chain))    # (e)
    assert np.array_equal(got[1].holder, again.holder) and np.array_equal(got[1].visits, again.visits)
    f = smp.record_fetch()
    assert len(f[0]) == 12
    for r in (0, 1):
        assert got[r].max_lag == 3
        check_against_fetched(got[r], f, ladder, r, 3, f"path 2, rung {r}")                      # (a), (c)
    assert np.array_equal(got[0].holder + got[1].holder, np.ones((12, 3), np.int32))             # two rungs share a group's two chains
    smp.record_end()


def test_widest_ladder_over_sparse_records(gpu):
    case = make_case("9-dense-leave-the-segment", 16)
    ladder = [0.97 ** i for i in range(16)]
    smp = case.sampler()
    mc3 = M.MC3(smp, n_chains=16, swap_period=2, n_swaps=15, betas=ladder, seed=3)
    smp.record_begin(2, 10)
    run_periods(case, [(smp, mc3)], case.schedule(20), 0, 10)
    case.check_path(smp)
    got = {r: smp.record_summary_mc3(rung=r, max_lag=0, per_group=True, flow=True) for r in (0, 15)}
    f = smp.record_fetch()
    for r in (0, 15):
        assert got[r].max_lag == 0
        tr, _ = check_against_fetched(got[r], f, np.array(ladder), r, 0, f"path 9, rung {r}")    # (a), (c)
        # one group: R-hat over its two halves, no effective sample size -- the NaN pattern of the numpy reference
        ref = D.summary(tr, 0)
        assert np.array_equal(np.isnan(got[r].pooled), np.isnan(ref.pooled))
        assert np.isnan(got[r].pooled[:, 7:]).all() and np.isfinite(got[r].pooled[:, 6]).any()
    smp.record_end()


def test_refusals_leave_the_recorder_alone(gpu):
    case = make_case("1-chain-lds", 8)
    L = _capi.lib()
    Q = 2 * case.topo.n_nodes + 9
    sched = case.schedule(8)

    def refused(smp, code, word, **kw):
        with pytest.raises(_capi.McdError, match=word) as e:
            smp.record_summary_mc3(**kw)
        got = e.value.code
        del e
        assert got == code, (got, code)

    smp, twin = case.sampler(seed=5), case.sampler(seed=5)
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "mcd_mh_record_summary_mc3: no recorder is active", n=4)
    for s in (smp, twin):
        s.record_begin(2, 16)
        s.run_schedule(sched)                                # four samples from before the ladder exists: every beta is 1
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "not initialised")
    pairs = [(s, M.MC3(s, n_chains=4, swap_period=2, n_swaps=3, betas=LADDER4, seed=11)) for s in (smp, twin)]
    for s, mc3 in pairs:
        for _ in range(6):
            mc3.run(2)
    case.check_path(smp)
    assert smp.record_count() == 10
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "rung 4", rung=4, skip=4)
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "rung -1", rung=-1, skip=4)
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "10 samples are waiting", skip=10)
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "ends past the 10 waiting", skip=4, n=7, max_lag=1)
    # a window that reaches back before the ladder: found by the gather on the device, and nothing but *n_used is written
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    pooled, pg = np.full((Q, 9), -7.5), np.full((2, Q, 4), -7.5)
    holder, visits, trips = np.full((10, 2), -7, np.int32), np.full((8, 4), -7, np.int64), np.full(8, -7, np.int64)
    used = C.c_int64(-1)
    rc = L.mcd_mh_record_summary_mc3(smp._h, 0, 0, -1, 3, C.byref(used), pooled.ctypes.data_as(dp), pg.ctypes.data_as(dp), holder.ctypes.data_as(ip),
                                     visits.ctypes.data_as(lp), trips.ctypes.data_as(lp))
    msg = L.mcd_last_error().decode()
    assert rc == _capi.MCD_ERR_INVALID_ARG and used.value == 0, (rc, msg)
    import re

    hit = re.search(r"sample (\d+) of group (\d+) has 4 chains at rung 0: the window holds samples recorded before mcd_mh_mc3_init", msg)
    assert hit and int(hit.group(1)) < 4 and int(hit.group(2)) < 2, msg
    assert (pooled == -7.5).all() and (pg == -7.5).all() and (holder == -7).all() and (visits == -7).all() and (trips == -7).all()
    refused(smp, _capi.MCD_ERR_INVALID_ARG, r"sample \d of group \d has 0 chains at rung 3", rung=3, skip=3)
    assert smp.record_summary_mc3(skip=4, max_lag=1).n_samples == 6          # the samples behind the ladder's start are fine
    # a handle whose chains are not whole groups: chains 2 .. 9 of 16 under groups of 4
    part = M.Sampler(case.lik, case.pf, case.ps, 8, seed=5, first_chain=2)
    part.set_state(case.s0)
    M.MC3(part, n_chains=4, swap_period=2, n_swaps=3, betas=LADDER4, seed=11,
          shard=types.SimpleNamespace(n_chains=16, world=2, size=8, lo=2), gather=lambda backend: None)
    part.record_begin(2, 4)
    part.run_schedule(sched[:4])
    refused(part, _capi.MCD_ERR_UNSUPPORTED, "not whole groups")
    assert part.record_count() == 2 and len(part.record_fetch()[0]) == 2
    part.record_end()
    # the old entry point keeps refusing a handle under MC3
    with pytest.raises(_capi.McdError, match="Metropolis-coupled") as e:
        smp.record_summary(skip=4)
    code = e.value.code
    del e
    assert code == _capi.MCD_ERR_UNSUPPORTED
    assert smp.record_count() == 10
    for a, b in zip(smp.record_fetch(), twin.record_fetch()):
        assert np.array_equal(a, b) and len(a) == 10
    for s in (smp, twin):
        s.record_end()
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "mcd_mh_record_summary_mc3: no recorder is active", n=4)
