"""The power posterior prior x likelihood^beta of the Metropolis-Hastings driver (mcd_mh_set_power) on every launch structure that forms
an acceptance ratio: the chain kernel (k_mh_chain.hip), the streaming chain kernel (k_mh_chain_big.hip), the one-wave step kernel of the
two-launch path and the workgroup-per-chain step kernel (k_mh.hip), the segment kernels over a dense and over a sparse likelihood
(mh_segment_device.hpp: the pending dense proposal and the steps inside a segment)."""
import functools
import os

import numpy as np
import pytest

import mcmc_date_amd as M
import oracle as O
from mcmc_date_amd import _capi

pytestmark = pytest.mark.gpu

# shape -> (tree, chains, knobs, what last_path() must say)
SHAPES = {
    "chain_lds": ("12-leaves", 8, {}, "factor resident in LDS"),
    "streamed": ("257-nodes", 16, {}, "two chains per workgroup"),
    "two_launch": ("257-nodes", 16, {"MCD_MH_PER_PHASE": "1"}, "two launches per lock step"),
    "segments": ("599-nodes", 5, {}, "segments: "),
    "step_wg": ("599-nodes", 5, {"MCD_MH_SEGMENTS": "0"}, "workgroup-per-chain step kernel"),
    "sparse_segments": ("47-nodes-sparse", 8, {}, "segments over a sparse precision matrix"),
}
SEED = 13


@functools.lru_cache(maxsize=None)
def problem(tree, B):
    """Everything but the handles: topology, proposal table, likelihood operands, prior (device arguments and the twin's spec), the initial
    states and the schedule of the two calls (1 500 lock steps as 700 + 800; on the small trees whole iterations, at least one cycle each)."""
    from mcmc_date_amd import synthetic as S

    if tree.endswith("-nodes"):
        n_leaves, seed = {"257-nodes": (129, 7), "599-nodes": (300, 61)}[tree]
        topo = S.random_topology(n_leaves, seed=seed)
        mu, sigma = S.random_spd_problem(topo.n_nodes - 2, seed=seed)
        sigma_inv, logdet = np.linalg.inv(sigma), float(np.linalg.slogdet(sigma)[1])
        s0 = S.random_states(topo, B, seed=seed + 1)
        s0.time_birth_rate = np.full(B, 1.0); s0.time_death_rate = np.full(B, 0.8); s0.rate_variance = np.full(B, 0.3)
        cal = [M.Calibration("root", 0, 0.9, 0.025, 1.1, 0.025), M.Calibration("n", 5, 0.2, 0.025, None, 0.0)]
        con, br, ht = [], [], 1.0
        ps, _ = M.proposals(topo, [], calibrations_available=True)
        sched = M.cycle_schedule(ps, 1, np.random.default_rng(0))[:, :1500]
        assert sched.shape[1] == 1500
        calls = [sched[:, :700], sched[:, 700:]]
    else:
        name = {"12-leaves": "12-leaves-variable-rate", "47-nodes-sparse": "24-leaves-braces"}[tree]
        fx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))
        topo = M.Topology(fx["parent"])
        mu, sigma_inv, logdet = fx["mu"], np.asarray(fx["sigma_inv"]), float(fx["logdet"])
        cal = [M.Calibration(f"c{i}", int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for i, r in enumerate(fx["cal"])]
        con = [M.Constraint(f"k{i}", int(r[0]), int(r[1]), r[2]) for i, r in enumerate(fx["con"])]
        br = [M.Brace(f"b{i}", [int(n) for n in fx["brace_nodes"][fx["brace_ptr"][i]:fx["brace_ptr"][i + 1]]], float(s))
              for i, s in enumerate(fx["brace_sd"])]
        ht = float(fx["prior_ht"])
        ps, _ = M.proposals(topo, br, calibrations_available=len(cal) > 0)
        x0 = M.init_with(topo, fx["mean_lengths"])
        if cal:
            x0.time_height = ht
        s0 = M.StateBatch.from_states([x0] * B)
        per_iter = M.cycle_schedule(ps, 1, np.random.default_rng(0)).shape[1]
        k = -(-1500 // per_iter)
        sched = M.cycle_schedule(ps, k, np.random.default_rng(0))
        calls = [sched[:max(1, k * 7 // 15)], sched[max(1, k * 7 // 15):]]
    spec = O.PriorSpec(topo.parent, ht, "UncorrelatedGamma", [(c.node, c.lower, c.lower_p, c.upper, c.upper_p) for c in cal],
                       [(k.young, k.old, k.p) for k in con], [(b.nodes, b.sd) for b in br])
    return dict(topo=topo, ps=ps, mu=np.asarray(mu), sigma_inv=sigma_inv, logdet=logdet, prior=(ht, "UncorrelatedGamma", cal, con, br), spec=spec,
                s0=s0, calls=calls, sparse=tree.endswith("sparse"), sweep=tree == "257-nodes")


def sampler(P, B, mu=None, sigma_inv=None, logdet=None):
    """A handle over the problem's tree and prior in the problem's initial states; the likelihood's operands may be replaced."""
    mu = P["mu"] if mu is None else mu
    sigma_inv = P["sigma_inv"] if sigma_inv is None else sigma_inv
    logdet = P["logdet"] if logdet is None else logdet
    topo = P["topo"]
    if P["sparse"]:
        assoc = [((int(i), int(j)), float(sigma_inv[i, j])) for i in range(sigma_inv.shape[0]) for j in range(sigma_inv.shape[1])]
        lik = M.SparseLikelihood(M.Sparse(mu, assoc, logdet), device=0).bind_tree(topo)
    else:
        lik = M.MvnLikelihood(M.Full(mu, sigma_inv, logdet)).bind_tree(topo)
        if P["sweep"]:
            lik.mvn.set_form("sweep")
    ht, model, cal, con, br = P["prior"]
    smp = M.Sampler(lik, M.PriorFunction(ht, model, cal, con, br, topo), P["ps"], B, seed=SEED)
    smp.set_state(P["s0"])
    return smp


def run_calls(smp, calls, want=None):
    out = [smp.run_schedule(c, trace=True) for c in calls]
    if want is not None:
        assert want in smp.last_path(), smp.last_path()
    return np.concatenate([a for a, _ in out]), np.concatenate([k for _, k in out])


STATE_FIELDS = ("heights", "rates", "time_height", "rate_mean", "rate_variance", "time_birth_rate", "time_death_rate")


def same_states(s1, s2):
    for f in STATE_FIELDS:
        assert np.array_equal(getattr(s1, f), getattr(s2, f)), f


def set_knobs(knobs, env):
    for k, v in env.items():
        knobs.setenv(k, v)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_exponent_zero_ignores_the_likelihood_exactly(gpu, shape, knobs):
    """Two handles that differ in their likelihood alone -- (mu, Sigma) against (mu + shift, 7 Sigma) --, every exponent 0: the same chains bit
    for bit over 1 500 lock steps (two calls): ln acceptance ratios, decisions, states, ln priors, ln Jacobians, tuning, counters.  A site that
    let the ln likelihood into its ratio would part them at the first proposal."""
    tree, B, env, want = SHAPES[shape]
    set_knobs(knobs, env)
    P = problem(tree, B)
    n = P["mu"].size
    shift = 0.01 * np.abs(P["mu"]).mean() * np.cos(np.arange(n))
    runs = []
    for ops in ({}, dict(mu=P["mu"] + shift, sigma_inv=P["sigma_inv"] / 7.0, logdet=P["logdet"] + n * np.log(7.0))):
        smp = sampler(P, B, **ops)
        smp.set_power(np.zeros(B))
        a, k = run_calls(smp, P["calls"], want)
        runs.append((a, k, smp.state(), smp.posterior(), smp.tuning()))
    (a1, k1, s1, p1, t1), (a2, k2, s2, p2, t2) = runs
    assert np.array_equal(k1, k2)
    assert 0.02 < k1.mean() < 0.98, k1.mean()
    assert np.array_equal(a1, a2, equal_nan=True)
    same_states(s1, s2)
    assert np.array_equal(p1[:, [0, 2]], p2[:, [0, 2]])
    assert np.all(np.isfinite(p1[:, 1])) and np.all(np.isfinite(p2[:, 1])) and not np.array_equal(p1[:, 1], p2[:, 1])   # two likelihoods indeed
    assert all(np.array_equal(x, y) for x, y in zip(t1, t2))


POWERS = (1.0, 0.5, 0.25)


@functools.lru_cache(maxsize=None)
def twin_run(tree, B, beta):
    """The CPU twin (posterior heating, every temperature 1) over Sigma^-1 scaled by beta: its ln likelihood differences are beta times the
    unscaled ones, exactly up to the rounding of ln likelihood itself.  (traces, decisions, final twin) of the problem's two calls."""
    P = problem(tree, B)
    s0, n = P["s0"], P["mu"].size
    model = O.MhModel(P["topo"].parent, P["mu"], P["sigma_inv"] * beta, P["logdet"] - n * np.log(beta), P["spec"], M.table_arrays(P["ps"]))
    twin = O.MhChains(model, s0.time_birth_rate, s0.time_death_rate, s0.time_height, s0.heights, s0.rate_mean, s0.rate_variance, s0.rates, seed=SEED)
    out = [twin.run(c, trace=True) for c in P["calls"]]
    return np.concatenate([a for a, _ in out]), np.concatenate([k for _, k in out]), twin


@pytest.mark.parametrize("shape", list(SHAPES))
def test_power_of_two_exponents_against_the_cpu_twin(gpu, shape, knobs):
    """One device run with the exponents 1, 1/2, 1/4, 1, ... against the unchanged CPU twin: scaling Sigma^-1 by a power of two scales the
    quadratic form exactly, so chain b at exponent beta is the twin's chain b over Sigma / beta.  Identical decisions at every step, ln
    acceptance ratios within the twin's tolerance, final states within 1e-9."""
    tree, B, env, want = SHAPES[shape]
    set_knobs(knobs, env)
    P = problem(tree, B)
    beta = np.array([POWERS[b % 3] for b in range(B)])
    smp = sampler(P, B)
    smp.set_power(beta)
    tol = 1e-8 + 1e-12 * np.abs(smp.posterior()[:, :2]).max()
    ta, tk = run_calls(smp, P["calls"], want)
    s = smp.state()
    assert 0.02 < tk.mean() < 0.98
    for pw in POWERS:
        idx = np.flatnonzero(beta == pw)
        ra, rk, twin = twin_run(tree, B, pw)
        assert np.array_equal(tk[:, idx], rk[:, idx]), (pw, np.argwhere(tk[:, idx] != rk[:, idx])[:3])
        fin = np.isfinite(ra[:, idx])
        assert np.array_equal(np.isfinite(ta[:, idx]), fin)
        d = np.abs(ta[:, idx][fin] - ra[:, idx][fin])
        assert np.all(d <= tol + 1e-10 * np.abs(ra[:, idx][fin])), (pw, d.max())
        for a, b in ((s.time_birth_rate, twin.birth), (s.time_death_rate, twin.death), (s.time_height, twin.tH), (s.heights, twin.H),
                     (s.rate_mean, twin.rMu), (s.rate_variance, twin.rVar), (s.rates, twin.R)):
            assert np.allclose(a[idx], b[idx], rtol=1e-9, atol=0), pw


def refused(code, call, *args):
    with pytest.raises(M.McdError) as e:
        call(*args)
    assert e.value.code == code, e.value


def test_modes_and_refusals(gpu):
    """set_temperatures after set_power is today's driver again, bit for bit; refused calls leave the handle as it was."""
    tree, B, _, want = SHAPES["chain_lds"]
    P = problem(tree, B)
    calls = P["calls"][:1]
    plain = sampler(P, B)
    a0, k0 = run_calls(plain, calls, want)
    # back from the power posterior
    back = sampler(P, B)
    back.set_power(np.linspace(0.0, 1.0, B))
    back.set_temperatures(np.ones(B))
    a1, k1 = run_calls(back, calls, want)
    assert np.array_equal(a0, a1, equal_nan=True) and np.array_equal(k0, k1)
    same_states(plain.state(), back.state())
    assert np.array_equal(plain.posterior(), back.posterior())
    # the power posterior is another chain (the exponents reach the ratio)
    power = np.linspace(0.0, 1.0, B)
    cold = sampler(P, B)
    cold.set_power(power)
    a2, k2 = run_calls(cold, calls, want)
    assert not np.array_equal(k2, k0) and not np.array_equal(a2, a0, equal_nan=True)
    # refused values: outside [0, 1], NaN -- in either mode the handle runs on unchanged
    for base, ref in ((None, (a0, k0, plain)), (power, (a2, k2, cold))):
        smp = sampler(P, B)
        if base is not None:
            smp.set_power(base)
        for bad in (1.0 + 1e-12, -1e-300, np.nan, np.inf):
            v = np.full(B, 0.5)
            v[B - 1] = bad
            refused(_capi.MCD_ERR_INVALID_ARG, smp.set_power, v)
        a, k = run_calls(smp, calls, want)
        assert np.array_equal(a, ref[0], equal_nan=True) and np.array_equal(k, ref[1])
        same_states(smp.state(), ref[2].state())
    # Metropolis-coupled MCMC on the handle: refused, and the heated chains run on as without the attempt
    ladder = np.array([1.0, 0.8, 0.6, 0.4])
    dp = _capi._dp
    runs = []
    for attempt in (False, True):
        smp = sampler(P, B)
        if attempt:
            smp.set_power(np.full(B, 0.5))                     # (mcd_mh_mc3_init clears the mode)
        _capi.check(_capi.lib().mcd_mh_mc3_init(smp._h, 4, ladder.ctypes.data_as(dp), B, 5))
        if attempt:
            refused(_capi.MCD_ERR_UNSUPPORTED, smp.set_power, np.full(B, 0.5))
        a, k = run_calls(smp, calls, want)
        runs.append((a, k, smp.state()))
    assert np.array_equal(runs[0][0], runs[1][0], equal_nan=True) and np.array_equal(runs[0][1], runs[1][1])
    same_states(runs[0][2], runs[1][2])
