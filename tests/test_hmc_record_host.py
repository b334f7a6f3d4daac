"""The sample recorder of the NUTS driver (mcd_hmc_record_*), the parts that need no device: the six entry points are declared in the header,
exported by the built library and bound with the header's arities; a NULL handle and bad arguments are refused before anything touches a
device; `Leapfrog.record_fetch` / `record_summary` pack what the C ABI writes into the arrays of `Sampler.record_*`; `monitor.record_nuts`
drives a driver in chunks -- one run and one fetch per chunk -- and numbers the transitions; and the ring arithmetic the C side uses
(slot of a sample, free slots, a window across the wrap) holds for every small ring."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi, hmc, monitor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"mcd_hmc_record_begin": 3, "mcd_hmc_record_count": 2, "mcd_hmc_record_fetch": 9, "mcd_hmc_record_end": 1,
         "mcd_hmc_record_quantities": 2, "mcd_hmc_record_summary": 8}


def _header_arity(header, name):
    m = re.search(r"^int " + name + r"\((.*?)\);", header, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/mcmcdate_mvn.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_record_calls_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "mcmcdate_mvn.h")).read()
    lib = _capi.lib()
    for name, n_args in ARITY.items():
        assert _header_arity(header, name) == n_args, name
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in _capi.SYMBOLS and len(_capi.SYMBOLS[name][1]) == n_args, name
    # the Metropolis-Hastings recorder's calls keep their arities beside them
    for name, n_args in (("mcd_mh_record_fetch", 9), ("mcd_mh_record_summary", 7)):
        assert _header_arity(header, name) == n_args == len(_capi.SYMBOLS[name][1])
    for method in ("record_begin", "record_count", "record_fetch", "record_end", "record_summary"):
        assert callable(getattr(M.Leapfrog, method))
    assert len(M.Leapfrog.NUTS_FIELDS) == 6 and len(M.Leapfrog.NUTS_STATS) == 4


def test_null_handles_and_bad_arguments_are_refused():
    L = _capi.lib()
    n = C.c_int64(5)
    x = np.zeros(16)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    ip = C.cast(p, C.POINTER(C.c_int64))
    for rc in (L.mcd_hmc_record_begin(None, 1, 4), L.mcd_hmc_record_begin(None, 0, 4), L.mcd_hmc_record_begin(None, 1, 0),
               L.mcd_hmc_record_count(None, C.byref(n)), L.mcd_hmc_record_fetch(None, 1, C.byref(n), ip, p, p, p, p, p),
               L.mcd_hmc_record_end(None), L.mcd_hmc_record_quantities(None, C.byref(n)),
               L.mcd_hmc_record_summary(None, 0, -1, 1, C.byref(n), p, p, p)):
        assert rc == _capi.MCD_ERR_INVALID_ARG
        assert b"mcd_hmc_record_" in L.mcd_last_error()
    assert np.all(x == 0.0)


class StubHandleLib:
    """The six calls as the C ABI specifies them, on a recorder that holds numbered samples: sample k of chain b is the number
    k + b / 10 in every field (plus 100 per scalar, 1000 per node), so a packed array says what was written where."""

    def __init__(self, batch, n_nodes, waiting):
        self.B, self.nn, self.waiting, self.fetched, self.period = batch, n_nodes, list(waiting), 0, 3
        self.summary_args = None

    def mcd_hmc_record_count(self, h, n):
        n._obj.value = len(self.waiting)
        return 0

    def mcd_hmc_record_quantities(self, h, q):
        q._obj.value = 2 * self.nn + 9
        return 0

    def mcd_hmc_record_fetch(self, h, max_samples, n_out, transition, sc, H, R, post, nuts):
        n = min(len(self.waiting), max_samples)
        B, nn = self.B, self.nn
        for i in range(n):
            k = self.waiting.pop(0)
            transition[i] = k * self.period
            for b in range(B):
                v, o = k + b / 10.0, i * B + b
                for f in range(5):
                    sc[o * 5 + f] = v + 100.0 * f
                for w in range(nn):
                    H[o * nn + w] = v + 1000.0 * w
                    R[o * nn + w] = -(v + 1000.0 * w)
                for f in range(3):
                    post[o * 3 + f] = v + 0.25 * f
                for f in range(6):
                    nuts[o * 6 + f] = 10.0 * f + b
        n_out._obj.value = n
        return 0

    def mcd_hmc_record_summary(self, h, skip, n, max_lag, used, pooled, per_chain, stats):
        self.summary_args = (skip, n, max_lag, bool(per_chain))
        Q = 2 * self.nn + 9
        for i in range(Q * 9):
            pooled[i] = float(i)
        for i in range(self.B * 4):
            stats[i] = 0.5 * i
        used._obj.value = (len(self.waiting) - skip) if n < 0 else n
        return 0


def _stub_leapfrog(monkeypatch, batch, n_nodes, waiting):
    stub = StubHandleLib(batch, n_nodes, waiting)
    monkeypatch.setattr(_capi, "lib", lambda: stub)
    lf = object.__new__(M.Leapfrog)

    class Topo:
        pass

    lf.topo = Topo()
    lf.topo.n_nodes = n_nodes
    lf.batch = batch
    lf._h = None
    return lf, stub


def test_fetch_packs_the_arrays_of_the_sampler_plus_the_diagnostics(monkeypatch):
    B, nn = 3, 4
    lf, stub = _stub_leapfrog(monkeypatch, B, nn, [5, 6, 7])
    it, sc, H, R, post, nuts = lf.record_fetch(2)
    assert it.dtype == np.int64 and np.array_equal(it, [15, 18]) and len(stub.waiting) == 1
    assert sc.shape == (2, B, 5) and H.shape == R.shape == (2, B, nn) and post.shape == (2, B, 3) and nuts.shape == (2, B, 6)
    v = np.array([5.0, 6.0])[:, None] + np.arange(B)[None, :] / 10.0
    for f in range(5):
        assert np.array_equal(sc[:, :, f], v + 100.0 * f)
    for w in range(nn):
        assert np.array_equal(H[:, :, w], v + 1000.0 * w) and np.array_equal(R[:, :, w], -H[:, :, w])
    assert np.array_equal(post[:, :, 2], v + 0.5)
    assert np.array_equal(nuts[0], 10.0 * np.arange(6)[None, :] + np.arange(B)[:, None])
    assert np.array_equal(lf.record_fetch()[0], [21]) and lf.record_fetch()[0].shape == (0,)
    # the trace of the monitor takes them as it takes the sampler's
    tr = monitor.Trace(it, sc[..., 0], sc[..., 1], sc[..., 2], H, sc[..., 3], sc[..., 4], R, post, None, nuts)
    assert tr.ages().shape == (2, B, nn) and tr.beta is None and tr.nuts is nuts


def test_summary_lowers_the_lag_cap_and_returns_the_diagnostics(monkeypatch):
    B, nn = 2, 3
    lf, stub = _stub_leapfrog(monkeypatch, B, nn, range(1, 11))
    got = lf.record_summary(skip=2, max_lag=255, per_chain=False)
    assert stub.summary_args == (2, -1, 3, False)               # 8 samples: odd, at most 8 // 2 - 1
    assert got.n_samples == 8 and got.max_lag == 3 and got.per_chain is None and got.n_nodes == nn
    assert got.pooled.shape == (2 * nn + 9, 9) and got.pooled[1, 0] == 9.0
    assert got.ages.shape == (nn, 9) and got.post.shape == (4, 9)
    assert got.nuts_stats.shape == (B, 4) and np.array_equal(got.nuts_stats[1], [2.0, 2.5, 3.0, 3.5])
    got = lf.record_summary(n=3, max_lag=9, per_chain=True)
    assert stub.summary_args == (0, 3, 0, True) and got.per_chain.shape == (B, 2 * nn + 9, 4)


class StubDriver:
    """What monitor.record_nuts needs of a driver, obeying the recorder's contract: transitions count from record_begin over consecutive
    calls, a call whose samples do not fit is refused."""

    def __init__(self, batch=2, n_nodes=3):
        self.batch, self.n_nodes = batch, n_nodes
        self.runs, self.fetches, self.begun, self.ended, self.rec = [], 0, [], 0, None

    def record_begin(self, period, capacity):
        assert self.rec is None
        self.rec = dict(period=period, capacity=capacity, it=0, waiting=[])
        self.begun.append((period, capacity))

    def nuts_run(self, n, eps, inv_mass, adapt=False, max_depth=8, seed=0, first_transition=0, chain_offset=0):
        r = self.rec
        adds = (r["it"] + n) // r["period"] - r["it"] // r["period"]
        assert len(r["waiting"]) + adds <= r["capacity"], "the run would overflow the recorder"
        assert not adapt
        for i in range(n):
            r["it"] += 1
            if r["it"] % r["period"] == 0:
                r["waiting"].append((r["it"], first_transition + i + 1))
        self.runs.append((n, first_transition))

    def record_fetch(self):
        w, self.rec["waiting"] = self.rec["waiting"], []
        self.fetches += 1
        n, B, nn = len(w), self.batch, self.n_nodes
        val = np.array([x[1] for x in w], float).reshape(n, 1) + np.arange(B)[None, :] / 10.0
        sc = np.stack([val + 100.0 * f for f in range(5)], axis=-1)
        H = np.repeat(val[:, :, None], nn, axis=2)
        return np.array([x[0] for x in w], np.int64), sc, H, -H, np.zeros((n, B, 3)), np.repeat(val[:, :, None], 6, axis=2)

    def record_end(self):
        assert self.rec is not None
        self.rec = None
        self.ended += 1


@pytest.mark.parametrize("n,period,chunk,first", [(23, 3, 5, 0), (23, 3, 7, 40), (10, 2, 256, 0), (7, 2, 2, 3), (5, 7, 3, 0), (0, 2, 4, 0), (17, 1, 4, 9)])
def test_record_nuts_drains_once_per_chunk_and_numbers_the_transitions(n, period, chunk, first):
    d = StubDriver()
    tr = monitor.record_nuts(d, n, 0.1, 1.0, period=period, chunk=chunk, first_transition=first)
    n_chunks = -(-n // chunk)
    assert len(d.runs) == n_chunks and d.fetches == n_chunks and d.begun == [(period, -(-chunk // period))] and d.ended == 1
    assert sum(k for k, _ in d.runs) == n and [f for _, f in d.runs] == [first + chunk * i for i in range(n_chunks)]
    want = first + period * np.arange(1, n // period + 1)
    assert tr.iteration.dtype == np.int64 and np.array_equal(tr.iteration, want)
    if len(want):
        b = np.arange(d.batch)[None, :] / 10.0
        assert np.array_equal(tr.time_birth_rate, want[:, None] + b) and np.array_equal(tr.rate_variance, want[:, None] + b + 400.0)
        assert tr.nuts.shape == (len(want), d.batch, 6) and tr.beta is None and np.array_equal(tr.rates, -tr.heights)


def test_record_nuts_ends_the_recorder_when_a_run_fails():
    class Failing(StubDriver):
        def nuts_run(self, *a, **k):
            raise RuntimeError("device lost")

    d = Failing()
    with pytest.raises(RuntimeError):
        monitor.record_nuts(d, 4, 0.1, 1.0, period=2, chunk=2)
    assert d.ended == 1 and d.rec is None


def test_ring_arithmetic():
    """The recorder's counts (csrc/recorder.cpp: one implementation behind mcd_mh_record_* and mcd_hmc_record_*): after `it` transitions
    it // period samples were taken, sample k lies in slot (k - 1) % capacity; a call of n transitions adds (it + n) // period - it // period;
    the window [skip, skip + m) of the waiting samples starts at slot (fetched + skip) % capacity.  Played against a list for every small
    ring: no waiting sample is ever overwritten by an accepted call.  At every step the library's own counts (mcd_record_ring_selftest_,
    computed by the struct every recorder call uses) must be the numbers of this model."""
    for period in (1, 2, 3):
        for cap in (1, 2, 4, 5):
            ring, it, fetched, taken = [None] * cap, 0, 0, 0
            rng = np.random.default_rng(period * 10 + cap)
            for _ in range(60):
                n = int(rng.integers(0, 2 * cap * period + 1))
                adds, free = (it + n) // period - it // period, cap - (it // period - fetched)
                assert _capi.record_ring_selftest(period, cap, it, fetched, n, 0) == (adds, free, it // period - fetched, fetched % cap)
                if adds <= free:
                    for _ in range(n):
                        it += 1
                        if it % period == 0:
                            taken += 1
                            slot = (taken - 1) % cap
                            assert ring[slot] is None, "a waiting sample was overwritten"
                            ring[slot] = taken
                    assert taken == it // period
                waiting = it // period - fetched
                assert 0 <= waiting <= cap
                if waiting:
                    skip = int(rng.integers(0, waiting))
                    m = int(rng.integers(1, waiting - skip + 1))
                    first = (fetched + skip) % cap
                    assert _capi.record_ring_selftest(period, cap, it, fetched, 0, skip) == (0, cap - waiting, waiting, first)
                    assert [ring[(first + i) % cap] for i in range(m)] == list(range(fetched + skip + 1, fetched + skip + m + 1))
                k = int(rng.integers(0, waiting + 1))
                for i in range(k):
                    assert ring[(fetched + i) % cap] == fetched + i + 1
                    ring[(fetched + i) % cap] = None
                fetched += k
