"""The sample recorder of the Metropolis-Hastings driver (mcd_mh_record_*), the parts that need no device: the four entry points are
declared in the header and exported by the built library, `monitor.Trace` keeps constructing without the new fields, and
`monitor.record` drives a sampler in chunks -- one run and one fetch per chunk -- and returns the iteration numbers of `monitor.collect`
whatever n_iter, period and chunk are."""
import os
import re

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi, monitor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD_CALLS = ["mcd_mh_record_begin", "mcd_mh_record_count", "mcd_mh_record_fetch", "mcd_mh_record_end"]


def test_record_calls_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "mcmcdate_mvn.h")).read()
    lib = _capi.lib()
    for name in RECORD_CALLS:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), f"{name} is not declared in include/mcmcdate_mvn.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in _capi.SYMBOLS
    n_args = {name: len(_capi.SYMBOLS[name][1]) for name in RECORD_CALLS}
    assert n_args == {"mcd_mh_record_begin": 3, "mcd_mh_record_count": 2, "mcd_mh_record_fetch": 9, "mcd_mh_record_end": 1}
    for method in ("record_begin", "record_count", "record_fetch", "record_end"):
        assert callable(getattr(M.Sampler, method))


def test_trace_constructs_without_the_recorders_fields():
    z = np.zeros((2, 3))
    t = monitor.Trace(np.array([2, 4]), z, z, z + 2.0, np.ones((2, 3, 5)), z, z, np.ones((2, 3, 5)))
    assert t.post is None and t.beta is None
    assert t.ages().shape == (2, 3, 5) and np.all(t.ages() == 2.0)
    t2 = monitor.Trace(np.array([2, 4]), z, z, z, np.ones((2, 3, 5)), z, z, np.ones((2, 3, 5)), post=np.zeros((2, 3, 3)), beta=np.ones((2, 3)))
    assert t2.post.shape == (2, 3, 3) and t2.beta.shape == (2, 3)


class StubSampler:
    """What monitor.record needs of a sampler, counting the calls; the 'state' of chain b at iteration i is the number i + b / 10, so a
    sample says which iteration it was taken at.  The recorder obeys the C ABI's contract: iterations count from record_begin over
    consecutive runs, a run whose samples do not fit is refused."""

    def __init__(self, batch=3, n_nodes=4, iterations_done=0):
        self.batch, self.n_nodes, self.iterations_done = batch, n_nodes, iterations_done
        self.runs, self.fetches, self.begun, self.ended = [], 0, [], 0
        self.rec = None

    def record_begin(self, period, capacity):
        assert self.rec is None
        self.rec = dict(period=period, capacity=capacity, it=0, waiting=[])
        self.begun.append((period, capacity))

    def run(self, n_iter, accumulate=False, chunk=256):
        assert chunk >= n_iter, "one call per chunk"
        r = self.rec
        adds = (r["it"] + n_iter) // r["period"] - r["it"] // r["period"]
        assert len(r["waiting"]) + adds <= r["capacity"], "the run would overflow the recorder"
        for _ in range(n_iter):
            r["it"] += 1
            self.iterations_done += 1
            if r["it"] % r["period"] == 0:
                r["waiting"].append((r["it"], self.iterations_done))
        self.runs.append((n_iter, accumulate))

    def record_fetch(self, max_samples=None):
        w, self.rec["waiting"] = self.rec["waiting"], []
        self.fetches += 1
        n, B, nn = len(w), self.batch, self.n_nodes
        val = np.array([x[1] for x in w], float).reshape(n, 1) + np.arange(B)[None, :] / 10.0
        sc = np.stack([val + 100.0 * f for f in range(5)], axis=-1)
        H = np.repeat(val[:, :, None], nn, axis=2)
        return np.array([x[0] for x in w], np.int64), sc, H, -H, np.zeros((n, B, 3)), np.ones((n, B))

    def record_end(self):
        assert self.rec is not None
        self.rec = None
        self.ended += 1


@pytest.mark.parametrize("n_iter,period,chunk,start", [(23, 3, 5, 0), (23, 3, 7, 40), (10, 2, 256, 0), (7, 2, 2, 3), (5, 7, 3, 0), (0, 2, 4, 0),
                                                       (17, 1, 4, 9), (12, 5, 12, 0)])
def test_record_drains_once_per_chunk_and_numbers_the_iterations(n_iter, period, chunk, start):
    s = StubSampler(iterations_done=start)
    tr = monitor.record(s, n_iter, period=period, accumulate=True, chunk=chunk)
    n_chunks = -(-n_iter // chunk)
    assert len(s.runs) == n_chunks and s.fetches == n_chunks and s.begun == [(period, -(-chunk // period))] and s.ended == 1
    assert sum(n for n, _ in s.runs) == n_iter and all(n <= chunk for n, _ in s.runs) and all(a for _, a in s.runs)
    assert s.iterations_done == start + n_iter
    want = start + period * np.arange(1, n_iter // period + 1)           # what monitor.collect numbers its samples
    assert tr.iteration.dtype == np.int64 and np.array_equal(tr.iteration, want)
    if len(want):
        assert tr.heights.shape == (len(want), s.batch, s.n_nodes) and tr.post.shape == (len(want), s.batch, 3) and tr.beta.shape == (len(want), s.batch)
        b = np.arange(s.batch)[None, :] / 10.0
        assert np.array_equal(tr.time_birth_rate, want[:, None] + b) and np.array_equal(tr.time_death_rate, want[:, None] + b + 100.0)
        assert np.array_equal(tr.time_height, want[:, None] + b + 200.0) and np.array_equal(tr.rate_mean, want[:, None] + b + 300.0)
        assert np.array_equal(tr.rate_variance, want[:, None] + b + 400.0)
        assert np.array_equal(tr.heights[:, :, 0], want[:, None] + b) and np.array_equal(tr.rates, -tr.heights)


def test_record_ends_the_recorder_when_a_run_fails():
    class Failing(StubSampler):
        def run(self, n_iter, accumulate=False, chunk=256):
            raise RuntimeError("device lost")

    s = Failing()
    with pytest.raises(RuntimeError):
        monitor.record(s, 4, period=2, chunk=2)
    assert s.ended == 1 and s.rec is None


def test_collect_and_record_agree_on_the_stub():
    class Collectable(StubSampler):
        def state(self):
            i = float(self.iterations_done)
            v = i + np.arange(self.batch) / 10.0
            H = np.repeat(v[:, None], self.n_nodes, axis=1)
            return M.StateBatch(H, -H, v + 200.0, v + 300.0, v, v + 100.0, v + 400.0)

        def run(self, n_iter, accumulate=False, chunk=256):
            if self.rec is None:
                self.iterations_done += n_iter
            else:
                super().run(n_iter, accumulate, chunk)

    a = monitor.collect(Collectable(iterations_done=6), 11, period=2)
    b = monitor.record(Collectable(iterations_done=6), 11, period=2, chunk=4)
    for f in ("iteration", "time_birth_rate", "time_death_rate", "time_height", "heights", "rate_mean", "rate_variance", "rates"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
