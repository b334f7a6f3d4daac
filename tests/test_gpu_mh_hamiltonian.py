"""The Hamiltonian proposal attached to the Metropolis-Hastings driver (mcd_mh_attach_hamiltonian): every iteration of mcd_mh_run begins
with one NUTS transition of every chain on the attached leapfrog handle.  The attached run is DEFINED as a composition of calls that
existed before it (hamiltonian_cases.compose: set_state / nuts / set_state / one iteration of an unattached run, through the host), and
every test compares it with that composition on twin handles, bit for bit."""
import numpy as np
import pytest

import mcmc_date_amd as M
from hamiltonian_cases import CASES, Case, compose, same_states
from mcmc_date_amd.hmc import NUTS_STREAM_DOMAIN

pytestmark = pytest.mark.gpu

N_ITER, MAX_DEPTH = 3, 3
UNSUPPORTED, INVALID = M._capi.MCD_ERR_UNSUPPORTED, M._capi.MCD_ERR_INVALID_ARG


def twins(case, **kw):
    """(attached sampler, its leapfrog handle, the composition's sampler, its leapfrog handle, eps, inv_mass)"""
    a, b = case.sampler(**kw), case.sampler(**kw)
    same_states(a.state(), b.state())
    la, lb = case.leapfrog(batch=a.batch), case.leapfrog(batch=a.batch)
    eps, im = case.nuts_inputs(lb, b)
    return a, la, b, lb, eps, im


def compare(case, a, b, got, want, stats=None):
    ta, ka = got
    tb, kb, _, asum, dsum = want
    case.check_path(a)
    assert ta.shape == tb.shape and np.array_equal(ta, tb, equal_nan=True) and np.array_equal(ka, kb)
    same_states(a.state(), b.state())
    assert np.array_equal(a.posterior(), b.posterior())
    assert all(np.array_equal(x, y) for x, y in zip(a.tuning(), b.tuning()))
    if stats is not None:
        n = tb.shape[0] // case.schedule(1).shape[1]
        assert stats["transitions"] == n
        assert np.array_equal(stats["alpha_sum"], asum) and np.all(asum > 0)
        assert np.array_equal(stats["depth_sum"], dsum) and np.all(dsum >= n) and np.all(dsum <= n * MAX_DEPTH)
        assert np.all(stats["leapfrog_steps"] >= dsum) and np.all(stats["leapfrog_steps"] <= n * (2 ** MAX_DEPTH - 1))
        assert np.all((stats["divergent"] >= 0) & (stats["divergent"] <= n))


@pytest.mark.parametrize("name", list(CASES))
def test_cycle_equals_the_composition(gpu, knobs, name):
    case = Case(name, knobs)
    a, la, b, lb, eps, im = twins(case)
    sched = case.schedule(N_ITER)
    a.attach_hamiltonian(la, eps, im, max_depth=MAX_DEPTH, first_transition=5)
    got = a.run_schedule(sched, trace=True)
    want = compose(b, lb, sched, eps, im, MAX_DEPTH, first_transition=5)
    compare(case, a, b, got, want, a.hamiltonian_stats())
    # the NUTS transitions moved the chains: the composition without them ends elsewhere
    c = case.sampler()
    c.run_schedule(sched)
    assert not np.array_equal(c.state().heights, a.state().heights)
    # reading the sums may clear them
    assert a.hamiltonian_stats(reset=True)["transitions"] == N_ITER
    z = a.hamiltonian_stats()
    assert z["transitions"] == 0 and not z["alpha_sum"].any() and not z["depth_sum"].any() and not z["leapfrog_steps"].any()


def test_cycle_with_the_dense_metric_of_the_attached_handle(gpu, knobs):
    case = Case("23-nodes-chain-lds", knobs)
    a, la, b, lb, eps, im = twins(case)
    rng = np.random.default_rng(8)
    G = rng.standard_normal((la.dim, la.dim)) * 0.05
    sd = np.sqrt(im)
    Cm = np.outer(sd, sd) * (np.eye(la.dim) + G @ G.T)
    Cm = 0.5 * (Cm + Cm.T)
    la.set_metric(Cm)
    lb.set_metric(Cm)
    sched = case.schedule(N_ITER)
    with pytest.raises(M.McdError, match="inv_mass must be NULL") as e:
        a.attach_hamiltonian(la, eps, im, max_depth=MAX_DEPTH)
    assert e.value.code == INVALID
    a.attach_hamiltonian(la, eps, None, max_depth=MAX_DEPTH)
    got = a.run_schedule(sched, trace=True)
    want = compose(b, lb, sched, eps, None, MAX_DEPTH)
    compare(case, a, b, got, want, a.hamiltonian_stats())
    # the metric is looked at again when a run starts
    la.clear_metric()
    s = a.state()
    with pytest.raises(M.McdError, match="dense metric") as e:
        a.run_schedule(sched)
    assert e.value.code == INVALID
    same_states(a.state(), s)


def test_split_calls_continue_the_transition_counter(gpu, knobs):
    case = Case("23-nodes-chain-lds", knobs)
    a, la, b, lb, eps, im = twins(case)
    sched = case.schedule(N_ITER)
    a.attach_hamiltonian(la, eps, im, max_depth=MAX_DEPTH)
    t1, k1 = a.run_schedule(sched[:2], trace=True)
    t2, k2 = a.run_schedule(sched[2:], trace=True)
    b.attach_hamiltonian(lb, eps, im, max_depth=MAX_DEPTH)
    tb, kb = b.run_schedule(sched, trace=True)
    assert np.array_equal(np.concatenate([t1, t2]), tb, equal_nan=True) and np.array_equal(np.concatenate([k1, k2]), kb)
    same_states(a.state(), b.state())
    assert np.array_equal(a.posterior(), b.posterior())
    sa, sb = a.hamiltonian_stats(), b.hamiltonian_stats()
    assert sa["transitions"] == sb["transitions"] == N_ITER and all(np.array_equal(sa[k], sb[k]) for k in sa if k != "transitions")
    # ... and both are the composition
    c = case.sampler()
    want = compose(c, case.leapfrog(), sched, eps, im, MAX_DEPTH)
    same_states(b.state(), c.state())
    assert np.array_equal(tb, want[0], equal_nan=True)


def test_chains_do_not_depend_on_the_batch_they_run_in(gpu, knobs):
    case = Case("23-nodes-chain-lds", knobs)
    big = case.sampler()
    small = case.sampler(batch=2, first_chain=2)
    same_states(small.state(), big.state().slice(2, 4))
    l6, l2 = case.leapfrog(), case.leapfrog(batch=2)
    eps, im = case.nuts_inputs(l6, big)
    sched = case.schedule(N_ITER)
    big.attach_hamiltonian(l6, eps, im, max_depth=MAX_DEPTH)
    small.attach_hamiltonian(l2, eps[2:4], im, max_depth=MAX_DEPTH, seed=big.seed ^ NUTS_STREAM_DOMAIN)
    tb, kb = big.run_schedule(sched, trace=True)
    ts, ks = small.run_schedule(sched, trace=True)
    assert np.array_equal(ts, tb[:, 2:4], equal_nan=True) and np.array_equal(ks, kb[:, 2:4])
    same_states(small.state(), big.state().slice(2, 4))
    assert np.array_equal(small.posterior(), big.posterior()[2:4])
    s6, s2 = big.hamiltonian_stats(), small.hamiltonian_stats()
    assert all(np.array_equal(s2[k], s6[k][2:4]) for k in s2 if k != "transitions")


@pytest.mark.parametrize("period", [1, 2])
def test_recorder_sees_the_complete_iterations(gpu, knobs, period):
    case = Case("23-nodes-chain-lds", knobs)
    a, la, b, lb, eps, im = twins(case)
    n_iter = 4
    sched = case.schedule(n_iter)
    a.attach_hamiltonian(la, eps, im, max_depth=MAX_DEPTH)
    a.record_begin(period, 4)
    a.run_schedule(sched)
    want = compose(b, lb, sched, eps, im, MAX_DEPTH)
    summary = a.record_summary()
    assert summary.n_samples == n_iter // period and np.all(np.isfinite(summary.ages[:, 0]))
    it, sc, H, R, post, beta = a.record_fetch()
    assert list(it) == list(range(period, n_iter + 1, period))
    for k, i in enumerate(it):
        s = want[2][i - 1]
        assert np.array_equal(H[k], s.heights) and np.array_equal(R[k], s.rates)
        assert np.array_equal(sc[k, :, 2], s.time_height) and np.array_equal(sc[k, :, 4], s.rate_variance)
    assert np.array_equal(post[-1], b.posterior()) and np.all(beta == 1.0)
    # a call whose samples do not fit is refused before anything is launched: both handles as they were
    a.run_schedule(sched)
    if period == 1:
        s_a, s_l = a.state(), la.state()
        stats = a.hamiltonian_stats()
        with pytest.raises(M.McdError, match="mcd_mh_run") as e:
            a.run_schedule(sched[:1])
        assert e.value.code == INVALID
        same_states(a.state(), s_a)
        same_states(la.state(), s_l)
        assert a.hamiltonian_stats()["transitions"] == stats["transitions"] == 2 * n_iter
    a.record_end()


def test_accumulate_adds_the_complete_iterations(gpu, knobs):
    case = Case("23-nodes-chain-lds", knobs)
    a, la, b, lb, eps, im = twins(case)
    sched = case.schedule(N_ITER)
    a.attach_hamiltonian(la, eps, im, max_depth=MAX_DEPTH)
    a.run_schedule(sched, accumulate=True)
    want = compose(b, lb, sched, eps, im, MAX_DEPTH, accumulate=True)
    (s1, q1, n1), (s2, q2, n2) = a.age_sums(), b.age_sums()
    assert n1 == n2 == N_ITER and np.array_equal(s1, s2) and np.array_equal(q1, q2)
    ages = sum(s.time_height[:, None] * s.heights for s in want[2])
    assert np.allclose(s1, ages, rtol=1e-14, atol=0)


def test_a_detached_sampler_runs_what_one_that_never_was_attached_runs(gpu, knobs):
    case = Case("23-nodes-chain-lds", knobs)
    a, b = case.sampler(), case.sampler()
    lf = case.leapfrog()
    eps, im = case.nuts_inputs(lf, a)
    a.attach_hamiltonian(lf, eps, im, max_depth=MAX_DEPTH)
    a.detach_hamiltonian()
    sched = case.schedule(5)
    ta, ka = a.run_schedule(sched, trace=True)
    tb, kb = b.run_schedule(sched, trace=True)
    assert np.array_equal(ta, tb, equal_nan=True) and np.array_equal(ka, kb)
    same_states(a.state(), b.state())
    assert np.array_equal(a.posterior(), b.posterior())
    with pytest.raises(M.McdError, match="no Hamiltonian proposal is attached"):
        a.hamiltonian_stats()
    with pytest.raises(M.McdError, match="no Hamiltonian proposal is attached"):
        a.detach_hamiltonian()
    a.attach_hamiltonian(lf, eps, im, max_depth=MAX_DEPTH)         # and it may be attached again


def test_refusals(gpu, knobs):
    case = Case("23-nodes-chain-lds", knobs)
    B = case.B
    lf = case.leapfrog()
    smp = case.sampler()
    eps, im = case.nuts_inputs(lf, smp)

    def refused(code, what, call, handles=()):
        before = [h.state() for h in handles]
        with pytest.raises(M.McdError, match=what) as e:
            call()
        assert e.value.code == code, e.value
        for h, s in zip(handles, before):
            same_states(h.state(), s)

    attach = lambda s, **kw: s.attach_hamiltonian(lf, kw.get("eps", eps), im, max_depth=kw.get("max_depth", MAX_DEPTH))
    # tempered targets, attach second
    hot = np.full(B, 1.0)
    hot[3] = 0.9
    t = case.sampler(burn=False)
    t.set_temperatures(hot)
    refused(UNSUPPORTED, "temperature", lambda: attach(t), (t, lf))
    t.set_temperatures(np.ones(B))
    attach(t)                                                        # (all cold again: allowed)
    p = case.sampler(burn=False)
    p.set_power(np.ones(B))
    refused(UNSUPPORTED, "power-posterior", lambda: attach(p), (p, lf))
    m3 = case.sampler(burn=False)
    M.MC3(m3, n_chains=2, n_swaps=1)
    refused(UNSUPPORTED, "Metropolis-coupled", lambda: attach(m3), (m3, lf))
    # ... and attach first
    attach(smp)
    refused(UNSUPPORTED, "Hamiltonian proposal is attached", lambda: smp.set_temperatures(hot), (smp, lf))
    smp.set_temperatures(np.ones(B))
    refused(UNSUPPORTED, "Hamiltonian proposal is attached", lambda: smp.set_power(np.ones(B)), (smp, lf))
    refused(UNSUPPORTED, "Hamiltonian proposal is attached", lambda: M.MC3(smp, n_chains=2, n_swaps=1), (smp, lf))
    refused(UNSUPPORTED, "Hamiltonian proposal is attached", lambda: M.MarginalLikelihood(smp, n_points=2), (smp, lf))
    # a second attach
    refused(INVALID, "attached to this handle already", lambda: attach(smp), (smp, lf))
    smp.detach_hamiltonian()
    # step sizes and depth
    for bad in (0.0, -0.1, np.inf, np.nan):
        e = eps.copy()
        e[1] = bad
        refused(INVALID, "step sizes", lambda: attach(smp, eps=e), (smp, lf))
    for bad in (0, 13):
        refused(INVALID, "max_depth", lambda: attach(smp, max_depth=bad), (smp, lf))
    # mismatching handles
    refused(INVALID, "different numbers of chains", lambda: smp.attach_hamiltonian(case.leapfrog(batch=8), eps, im), (smp,))
    # an active recorder on the leapfrog handle, at attach time and when a run starts
    lf.record_begin(1, 4)
    refused(INVALID, "active recorder", lambda: attach(smp), (smp, lf))
    lf.record_end()
    attach(smp)
    lf.record_begin(1, 4)
    refused(INVALID, "active recorder", lambda: smp.run(1), (smp, lf))
    lf.record_end()
    smp.run(1)
