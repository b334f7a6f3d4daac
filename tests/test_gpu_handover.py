"""The chains move between the Metropolis-Hastings driver and the leapfrog / NUTS driver ON THE DEVICE (mcd_hmc_take_state,
mcd_mh_take_state; csrc/k_handover.hip).  Each hand-over is compared bit for bit with the host round trip through the calls that existed
before it -- set_state of the other handle's state() -- on a twin handle, never with itself.

Both drivers lay their rows out with the leading dimension 8 ceil(n_nodes / 8), so no pair of handles made through the public interface
has different leading dimensions; the 259-node case (ld 264, five nodes short of it, more than one pass of a 256-thread workgroup over a row) is the
one that exercises the row addressing."""
import numpy as np
import pytest

import mcmc_date_amd as M
from hamiltonian_cases import CASES, FIELDS, Case, same_states

pytestmark = pytest.mark.gpu

HANDOVER_CASES = [c for c in CASES if "per-phase" not in c]


@pytest.fixture(params=HANDOVER_CASES)
def case(request, gpu, knobs):
    return Case(request.param, knobs)


def moved(case, smp):
    """A leapfrog handle whose chains are one NUTS transition away from the sampler's."""
    lf = case.leapfrog()
    eps, im = case.nuts_inputs(lf, smp)
    lf.nuts(eps, im, max_depth=3, seed=11, transition=0)
    return lf


def test_hmc_take_state_equals_set_state_of_the_samplers_state(case):
    smp = case.sampler()
    a, b = case.leapfrog(), case.leapfrog()
    a.take_state(smp)
    b.set_state(smp.state())
    same_states(a.state(), b.state())
    same_states(a.state(), smp.state())
    for x, y in zip(a.position(), b.position()):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)
    # ... and over a state the handle held before (nothing of it may survive)
    a.nuts(0.02, 1e-4, max_depth=2, seed=3, transition=0)
    a.take_state(smp)
    for x, y in zip(a.position(), b.position()):
        assert np.array_equal(x, y)


def test_mh_take_state_equals_set_state_of_the_leapfrogs_state(case):
    a, b = case.sampler(), case.sampler()
    lf = moved(case, a)
    assert not np.array_equal(lf.state().heights, a.state().heights)
    tuning = a.tuning()
    a.take_state(lf)
    b.set_state(lf.state())
    same_states(a.state(), b.state())
    same_states(a.state(), lf.state())
    assert np.all(np.isfinite(a.posterior())) and np.array_equal(a.posterior(), b.posterior())
    assert all(np.array_equal(x, y) for x, y in zip(tuning, a.tuning()))             # tuning parameters and counters are untouched
    # what a run derives when it starts (prior blocks, kept summands, the incremental z / q) is derived from the new states
    sched = case.schedule(2)
    ta, ka = a.run_schedule(sched, trace=True)
    tb, kb = b.run_schedule(sched, trace=True)
    case.check_path(a)
    assert np.array_equal(ta, tb, equal_nan=True) and np.array_equal(ka, kb)
    same_states(a.state(), b.state())
    assert np.array_equal(a.posterior(), b.posterior())
    assert all(np.array_equal(x, y) for x, y in zip(a.tuning(), b.tuning()))


def test_refusals_leave_both_handles_alone(gpu, knobs):
    case = Case("23-nodes-chain-lds", knobs)
    smp = case.sampler()
    lf = moved(case, smp)
    s_smp, s_lf = smp.state(), lf.state()

    def refused(call, what):
        with pytest.raises(M.McdError, match=what) as e:
            call()
        assert e.value.code == M._capi.MCD_ERR_INVALID_ARG
        same_states(smp.state(), s_smp)
        same_states(lf.state(), s_lf)

    # batch 6 against 8
    lf8 = case.leapfrog(batch=8)
    lf8.set_state(case.rows(0, 8))
    smp8 = case.sampler(batch=8, burn=False)
    refused(lambda: lf8.take_state(smp), "different numbers of chains")
    refused(lambda: smp.take_state(lf8), "different numbers of chains")
    refused(lambda: lf.take_state(smp8), "different numbers of chains")
    # another topology with as many nodes
    par = np.asarray(case.topo.parent)
    from mcmc_date_amd import synthetic as S

    other = next(t for t in (S.random_topology(12, seed=s) for s in range(20)) if not np.array_equal(np.asarray(t.parent), par))
    n = other.n_nodes - 2
    mu, sigma = S.random_spd_problem(n, seed=n)
    lik_o = M.MvnLikelihood.from_covariance(mu, sigma).bind_tree(other)
    pf_o = M.PriorFunction(1.0, "UncorrelatedLogNormal", [], [], [], other)
    lf_o = M.Leapfrog(lik_o, pf_o, True, 6)
    st_o = S.random_states(other, 6, seed=1)
    st_o.time_birth_rate = np.full(6, 1.0); st_o.time_death_rate = np.full(6, 0.8); st_o.rate_variance = np.full(6, 0.3)
    lf_o.set_state(st_o)
    refused(lambda: smp.take_state(lf_o), "different topologies")
    refused(lambda: lf_o.take_state(smp), "different topologies")
    # another number of nodes
    c67 = Case("67-nodes-chain-streamed", knobs)
    lf67 = c67.leapfrog(batch=6)
    refused(lambda: lf67.take_state(smp), "different numbers of nodes")
    # a source without a state
    empty = M.Sampler(case.lik, case.pf, case.ps, 6, seed=1)
    refused(lambda: lf.take_state(empty), "no state")
    refused(lambda: smp.take_state(case.leapfrog()), "no state")
