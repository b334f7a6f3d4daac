"""Sampler.record_summary / mcd_mh_record_summary: posterior summaries and convergence diagnostics of the samples waiting in the recorder's
ring, computed on the device where they lie (csrc/k_summary.hip, the ring front end).  The reference is diagnostics.summary (checked by
tests/test_diagnostics.py) on the arrays that record_fetch returns AFTERWARDS, laid out in the quantity order of the header: ages tH h_v,
rates, birth, death, tH, rMu, rVar, ln prior, ln likelihood, ln jacobianRootBranch, ln posterior.  Tolerances: those of
tests/test_gpu_summary.py (its docstring derives them).  Every case asserts the launch structure its run took."""
import math

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi, monitor
from mcmc_date_amd import diagnostics as D
from mcmc_date_amd import sampler as SM

pytestmark = pytest.mark.gpu

FIELDS = ("time_birth_rate", "time_death_rate", "time_height", "rate_mean", "rate_variance", "heights", "rates")
# name -> (likelihood, leaves or fixture, chains, MCD_MH_PATH_*)
CASES = {
    "1-chain-lds": ("golden", "12-leaves-variable-rate", 16, 1),
    "2-chain-streamed": ("dense", 129, 3, 2),
    "9-dense-leave-the-segment": ("sparse", 300, 17, 9),
}
S_STEPS = 12


class Case:
    """Tree, likelihood, prior, proposal table and initial states of one case, and samplers on them (as tests/test_gpu_mh_record.py)."""

    def __init__(self, name):
        from mcmc_date_amd import synthetic as S

        kind, what, self.B, self.path = CASES[name]
        B = self.B
        if kind == "golden":
            import os

            fx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", what + ".npz")))
            self.topo = topo = M.Topology(fx["parent"])
            cal = [M.Calibration(f"c{i}", int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for i, r in enumerate(fx["cal"])]
            con = [M.Constraint(f"k{i}", int(r[0]), int(r[1]), r[2]) for i, r in enumerate(fx["con"])]
            ht = float(fx["prior_ht"])
            self.lik = M.MvnLikelihood(M.Full(fx["mu"], fx["sigma_inv"], float(fx["logdet"]))).bind_tree(topo)
            self.pf = M.PriorFunction(ht, "UncorrelatedGamma", cal, con, [], topo)
            self.ps, _ = M.proposals(topo, [], calibrations_available=len(cal) > 0)
            x0 = M.init_with(topo, fx["mean_lengths"])
            if cal:
                x0.time_height = ht
            self.s0 = M.StateBatch.from_states([x0] * B)
        else:
            self.topo = topo = S.random_topology(what, seed=31)
            n = topo.n_nodes - 2
            if kind == "sparse":
                _, assoc = S.banded_precision(n, seed=n)
                self.lik = M.SparseLikelihood(M.Sparse(np.random.default_rng(1).uniform(0.01, 0.2, n), assoc, 0.0)).bind_tree(topo)
            else:
                mu, sigma = S.random_spd_problem(n, seed=n)
                self.lik = M.MvnLikelihood.from_covariance(mu, sigma).bind_tree(topo)
            inner = [v for v in range(1, topo.n_nodes) if (np.asarray(topo.parent) == v).any()]
            cal = [M.Calibration("root", 0, 0.9, 0.025, 1.3, 0.025), M.Calibration("c", int(inner[len(inner) // 2]), 1e-3, 0.025, 5.0, 0.025)]
            self.pf = M.PriorFunction(1.0, "UncorrelatedLogNormal", cal, [], [], topo)
            self.ps, _ = M.proposals(topo, [], calibrations_available=True)
            self.s0 = S.random_states(topo, B, seed=5)
            self.s0.time_birth_rate = np.full(B, 1.0); self.s0.time_death_rate = np.full(B, 0.8); self.s0.rate_variance = np.full(B, 0.3)

    def sampler(self, seed=77):
        smp = M.Sampler(self.lik, self.pf, self.ps, self.B, seed=seed)
        smp.set_state(self.s0)
        return smp

    def schedule(self, n_iter, S=S_STEPS, seed=4):
        tab = M.table_arrays(self.ps)
        dense = [i for i in range(len(self.ps)) if (tab["kind"][i] == SM.SCALE_SCALAR and tab["node"][i] in (SM.TIME_HEIGHT, SM.RATE_MEAN))
                 or tab["kind"][i] in (SM.SCALE_NORM_TREE, SM.SCALE_RATES_TREE_CONTRA, SM.SLIDE_ROOT_CONTRA, SM.SCALE_CONTRARILY)]
        rng = np.random.default_rng(seed)
        sched = rng.integers(0, len(self.ps), size=(n_iter, S)).astype(np.int32)
        pick = rng.random((n_iter, S)) < 0.125
        sched[pick] = rng.choice(dense, size=int(pick.sum()))
        return sched

    def check_path(self, smp):
        got = int(_capi.lib().mcd_mh_last_path(smp._h))
        assert got == self.path, f"meant for launch structure {self.path}, the run took {got}: {smp.last_path()}"


def quantities(fetched):
    """The fetched arrays as x [n, B, 2 n_nodes + 9] in the header's quantity order."""
    it, sc, H, R, post, beta = fetched
    ages = sc[:, :, 2][:, :, None] * H                                   # monitor.Trace.ages
    lnpost = (post[:, :, 0] + post[:, :, 1]) + post[:, :, 2]
    return np.concatenate([ages, R, sc, post, lnpost[:, :, None]], axis=2)


def fsum_mean_var(col):
    m = math.fsum(col) / len(col)
    return m, math.fsum((col - m) ** 2) / len(col)


def compare(got, x, max_lag, label):
    """pooled / per_chain of the device against the restatement on x [n, B, Q], under the rules of tests/test_gpu_summary.py."""
    n, B, Q = x.shape
    l = n * B
    ref = D.summary(x, max_lag)
    assert got.pooled.shape == (Q, 9)
    assert np.array_equal(got.pooled[:, 2:6], ref.pooled[:, 2:6], equal_nan=True), label
    assert np.array_equal(np.isnan(got.pooled), np.isnan(ref.pooled)), label
    good = np.zeros(Q, bool)
    for q in range(Q):
        col = x[:, :, q].reshape(-1)
        m, v = fsum_mean_var(col)
        assert abs(got.pooled[q, 0] - m) <= l * 2.0 ** -52 * np.abs(col).max(), (label, q)
        good[q] = v > 0 and abs(m) <= 1e4 * math.sqrt(v)
        if good[q]:
            assert abs(got.pooled[q, 1] - v) <= 1e-10 * v, (label, q, got.pooled[q, 1], v)
    g = np.nonzero(good)[0]
    assert len(g) > 0, label
    assert np.allclose(got.pooled[g, 6], ref.pooled[g, 6], rtol=1e-9, atol=0, equal_nan=True), label
    if max_lag:
        keep = g[ref.min_abs_p[g] > 1e-9]
        assert len(g) - len(keep) <= 0.02 * Q, (label, len(g) - len(keep))
        assert np.allclose(got.pooled[keep, 7], ref.pooled[keep, 7], rtol=1e-8, atol=0, equal_nan=True), label
        assert np.array_equal(got.pooled[keep, 8], ref.pooled[keep, 8], equal_nan=True), label
        assert np.isfinite(got.pooled[keep, 7]).any(), label
    if got.per_chain is not None:
        assert np.array_equal(got.per_chain[:, :, 2:], ref.per_chain[:, :, 2:]), label
        assert np.allclose(got.per_chain[:, g, :2], ref.per_chain[:, g, :2], rtol=1e-10, atol=0), label
    return ref


def test_summary_of_the_waiting_samples_and_nothing_disturbed(gpu):
    case = Case("1-chain-lds")
    sched = case.schedule(200)
    smp, twin = case.sampler(), case.sampler()
    for s in (smp, twin):
        s.record_begin(2, 100)
        s.run_schedule(sched, accumulate=True)
        case.check_path(s)
    got = smp.record_summary(skip=25, max_lag=35, per_chain=True)
    assert got.n_samples == 75 and got.max_lag == 35 and smp.record_count() == 100
    again = smp.record_summary(skip=25, n=75, max_lag=35, per_chain=True)
    assert np.array_equal(got.pooled.view(np.uint64), again.pooled.view(np.uint64)) and np.array_equal(got.per_chain, again.per_chain, equal_nan=True)
    f, ft = smp.record_fetch(), twin.record_fetch()
    for a, b in zip(f, ft):
        assert np.array_equal(a, b)
    x = quantities(f)[25:]
    assert x.shape == (75, 16, 2 * case.topo.n_nodes + 9)
    compare(got, x, 35, "path 1")
    nn = case.topo.n_nodes
    assert got.ages.shape == (nn, 9) and got.rates.shape == (nn, 9) and got.scalars.shape == (5, 9) and got.post.shape == (4, 9)
    assert np.array_equal(got.scalars[2, 2:4], [x[:, :, 2 * nn + 2].min(), x[:, :, 2 * nn + 2].max()])
    assert np.isnan(got.ages[:, 6]).any() and np.isfinite(got.ages[:, 6]).any()          # leaves: age 0, no rhat; inner nodes have one
    # the chains and everything else a later call can see are those of the twin that never asked for a summary
    s1, s2 = smp.state(), twin.state()
    for fld in FIELDS:
        assert np.array_equal(getattr(s1, fld), getattr(s2, fld)), fld
    assert np.array_equal(smp.posterior(), twin.posterior())
    assert all(np.array_equal(a, b) for a, b in zip(smp.age_sums()[:2], twin.age_sums()[:2])) and smp.age_sums()[2] == twin.age_sums()[2] == 200
    for s in (smp, twin):
        s.run_schedule(sched[:4])
    for a, b in zip(smp.record_fetch(), twin.record_fetch()):
        assert np.array_equal(a, b) and len(a) == 2
    smp.record_end()
    twin.record_end()


def test_window_that_wraps_around_the_ring(gpu):
    case = Case("1-chain-lds")
    sched = case.schedule(60)
    smp = case.sampler()
    smp.record_begin(1, 40)
    smp.run_schedule(sched[:30])
    assert len(smp.record_fetch(25)[0]) == 25
    smp.run_schedule(sched[30:])
    case.check_path(smp)
    assert smp.record_count() == 35                       # slots 25 .. 39, then 0 .. 19
    whole = smp.record_summary(max_lag=15, per_chain=True)
    part = smp.record_summary(skip=10, n=20, max_lag=9)    # slots 35 .. 39, 0 .. 14
    f = smp.record_fetch()
    assert np.array_equal(f[0], np.arange(26, 61))
    x = quantities(f)
    compare(whole, x, 15, "wrap, whole")
    compare(part, x[10:30], 9, "wrap, part")
    smp.record_end()


@pytest.mark.parametrize("name", ["2-chain-streamed", "9-dense-leave-the-segment"])
def test_wide_records(gpu, name):
    case = Case(name)
    smp = case.sampler()
    smp.record_begin(2, 9)
    smp.run_schedule(case.schedule(18))
    case.check_path(smp)
    nn = case.topo.n_nodes
    assert nn > 64 and (2 * nn + 9) % 64 != 0
    got = smp.record_summary(max_lag=3, per_chain=True)
    assert got.n_samples == 9 and got.max_lag == 3
    x = quantities(smp.record_fetch())
    compare(got, x, 3, name)
    smp.record_end()


def test_summarize_recorded_is_summarize_node_ages(gpu):
    case = Case("1-chain-lds")
    smp = case.sampler()
    smp.record_begin(2, 60)
    smp.run_schedule(case.schedule(120))
    case.check_path(smp)
    names = [f"n{v}" for v in range(case.topo.n_nodes)]
    got = monitor.summarize_recorded(smp, burn_in=0.25, names=names)
    assert smp.record_count() == 60
    it, sc, H, R, post, beta = smp.record_fetch()
    tr = monitor.Trace(it, sc[..., 0], sc[..., 1], sc[..., 2], H, sc[..., 3], sc[..., 4], R, post, beta)
    skip = 15
    ages = tr.ages()[skip:]
    want = monitor.summarize_node_ages(ages.reshape(-1, case.topo.n_nodes), burn_in=0.0, names=names)
    l = ages.shape[0] * ages.shape[1]
    for a, b in ((got.minimum, want.minimum), (got.maximum, want.maximum), (got.ci_lower, want.ci_lower), (got.ci_upper, want.ci_upper)):
        assert np.array_equal(a, b)
    for v in range(case.topo.n_nodes):
        col = ages[:, :, v].reshape(-1)
        m, var = fsum_mean_var(col)
        assert abs(got.mean[v] - m) <= l * 2.0 ** -52 * np.abs(col).max() and abs(want.mean[v] - m) <= l * 2.0 ** -52 * np.abs(col).max()
        if var > 0 and abs(m) <= 1e4 * math.sqrt(var):
            assert abs(got.variance[v] - var) <= 1e-10 * var
    ref = D.summary(ages, 21)
    inner = np.isfinite(ref.rhat)
    assert inner.any() and np.array_equal(np.isnan(got.rhat), ~inner)
    assert np.allclose(got.rhat[inner], ref.rhat[inner], rtol=1e-9, atol=0) and got.name == names and got.render().count("\n") == len(names) + 1
    assert got.ess.shape == got.rhat.shape and np.isfinite(got.ess[inner]).all()
    smp.record_end()


def test_refusals_leave_the_recorder_alone(gpu):
    import ctypes as C

    case = Case("1-chain-lds")
    L = _capi.lib()
    sched = case.schedule(20)

    def refused(smp, code, word, **kw):
        with pytest.raises(_capi.McdError, match=word) as e:
            smp.record_summary(**kw)
        got = e.value.code
        del e
        assert got == code, (got, code)

    smp, twin = case.sampler(), case.sampler()
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "no recorder is active")
    for s in (smp, twin):
        s.record_begin(2, 10)
        s.run_schedule(sched)
    case.check_path(smp)
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "10 samples are waiting", skip=10)
    refused(smp, _capi.MCD_ERR_INVALID_ARG, "ends past the 10 waiting", skip=4, n=7, max_lag=1)
    pooled = np.empty((2 * case.topo.n_nodes + 9, 9))
    used = C.c_int64(-1)
    rc = L.mcd_mh_record_summary(smp._h, 0, -1, 4, C.byref(used), pooled.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert rc == _capi.MCD_ERR_INVALID_ARG and "odd" in L.mcd_last_error().decode() and used.value == 0
    assert smp.record_count() == 10
    for a, b in zip(smp.record_fetch(4), twin.record_fetch(4)):
        assert np.array_equal(a, b)
    smp.set_temperatures(np.where(np.arange(case.B) == 3, 0.5, 1.0))
    refused(smp, _capi.MCD_ERR_UNSUPPORTED, "only cold chains")
    smp.set_temperatures(np.ones(case.B))
    assert smp.record_summary(max_lag=1).n_samples == 6
    M.MC3(smp, n_chains=4, swap_period=2, n_swaps=3, betas=[1.0, 0.9, 0.8, 0.7], seed=11)
    refused(smp, _capi.MCD_ERR_UNSUPPORTED, "Metropolis-coupled")
    assert smp.record_count() == 6
    for a, b in zip(smp.record_fetch(), twin.record_fetch()):
        assert np.array_equal(a, b) and len(a) == 6
    smp.record_end()
    twin.record_end()
