"""The dense metric of the device leapfrog and NUTS (mcd_hmc_set_metric, mcd_hmc_nuts_warmup_dense; csrc/metric_device.hpp, k_hmc.hip,
k_nuts.hip, k_hmc_cov.hip): the reference's `HTuneAllMasses` (app/Hamiltonian.hs:62-63).

With C = M^-1 = U U^T: momenta p = U^-T z, kinetic energy 1/2 p^T C p, drift q += eps (C p), U-turn (q+ - q-)^T C r >= 0 at both ends.
References: numpy on the handle's own gradient for one leapfrog step, the diagonal path for C = diag(v), the CPU twin of
tests/test_gpu_nuts.py with that algebra (momenta from numpy's own Cholesky factor) for whole transitions, hmc.shrunk_covariance of the
recorded positions for the warm-up, Metropolis-Hastings chains for the posterior.  Tolerances: where they are used."""
import dataclasses
import math

import numpy as np
import pytest

import mcmc_date_amd as M
import oracle as O
import test_gpu_nuts as TN
from mcmc_date_amd import _capi
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
_cache = {}


def golden_problem(golden, name):
    """(fx, topo, prior, likelihood, oracle prior, braces, time height) of a committed input."""
    if name not in _cache:
        fx = golden[name]
        topo = M.Topology(fx["parent"])
        cal, con, br = TN.tables(fx)
        ht = float(fx["prior_ht"])
        pf = M.PriorFunction(ht, "UncorrelatedGamma", cal, con, br, topo)
        lik = M.MvnLikelihood(M.Full(fx["mu"], fx["sigma_inv"], float(fx["logdet"]))).bind_tree(topo)
        spec = O.PriorSpec(fx["parent"], ht, "UncorrelatedGamma", [(c.node, c.lower, c.lower_p, c.upper, c.upper_p) for c in cal],
                           [(k.young, k.old, k.p) for k in con], [(b.nodes, b.sd) for b in br])
        _cache[name] = (fx, topo, pf, lik, spec, br, ht)
    return _cache[name]


def posterior_states(golden, name, B):
    """Typical posterior states, different per chain (the burn-in of tests/test_gpu_nuts.py:136-141)."""
    key = (name, B)
    if key not in _cache:
        fx, topo, pf, lik, _, br, ht = golden_problem(golden, name)
        ps, _ = M.proposals(topo, br, calibrations_available=True)
        smp = M.Sampler(lik, pf, ps, B, seed=3)
        x0 = M.init_with(topo, fx["mean_lengths"])
        x0.time_height = ht
        smp.set_initial_state(x0)
        smp.burn_in(fast=[10, 10, 20, 40], slow=[100, 100])
        _cache[key] = smp.state()
    return _cache[key]


def synthetic_problem(n_leaves, B, sparse):
    """A random tree, a banded precision matrix around the distances of one of its states (kept sparse on the device, or densified), valid
    states near that one: (topo, likelihood, prior, states)."""
    key = ("syn", n_leaves, sparse)
    if key not in _cache:
        topo = S.random_topology(n_leaves, seed=5)
        n = topo.n_nodes - 2
        P, assoc = S.banded_precision(n, seed=5)
        st0 = S.random_states(topo, 1, seed=7)
        mu = O.distances(topo.parent, st0.heights[0], st0.rates[0], st0.time_height[0], st0.rate_mean[0])
        if sparse:
            lik = M.SparseLikelihood(M.Sparse(mu, assoc, 0.0)).bind_tree(topo)
        else:
            lik = M.MvnLikelihood(M.Full(mu, P.toarray(), 0.0)).bind_tree(topo)
        pf = M.PriorFunction(1.0, "UncorrelatedGamma", [], [], [], topo)
        _cache[key] = (topo, lik, pf)
    topo, lik, pf = _cache[key]
    st = S.random_states(topo, B, seed=7, jitter=0.002)
    rng = np.random.default_rng(12)
    full = M.StateBatch(st.heights, st.rates, st.time_height, st.rate_mean, np.exp(0.1 * rng.standard_normal(B)), np.exp(0.1 * rng.standard_normal(B)),
                        0.5 + 0.2 * rng.random(B))
    return topo, lik, pf, full


def crude_inv_mass(q0):
    return np.maximum((0.1 * np.abs(q0)).mean(axis=0) ** 2, 1e-12)            # tests/test_gpu_nuts.py:146


def metric_for(q0):
    """C = S R S, S = diag(0.1 mean |q0|) with the floor of tests/test_gpu_nuts.py:146, R_ij = 0.5^|i - j|."""
    s = np.sqrt(crude_inv_mass(q0))
    k = np.arange(len(s))
    return s[:, None] * 0.5 ** np.abs(k[:, None] - k[None, :]) * s[None, :]


def diagonal_run(lf, st, inv_mass, eps):
    """A diagonal-metric transition and two leapfrog steps from st: everything the handle hands back."""
    lf.set_state(st)
    a, d = lf.nuts(eps, inv_mass, max_depth=4, seed=41, transition=3)
    q, v, g = lf.position()
    p = lf.leapfrog(np.random.default_rng(6).normal(size=q.shape) / np.sqrt(inv_mass), 0.5 * eps, inv_mass, 2)
    return (a, d, q, v, g, p) + lf.position()


def same_bits(x, y):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


def test_refusals_leave_the_handle_as_it_was(gpu, golden):
    fx, topo, pf, lik, *_ = golden_problem(golden, "12-leaves-variable-rate")
    B = 4
    st = posterior_states(golden, "12-leaves-variable-rate", 6).slice(0, B)
    fresh = M.Leapfrog(lik, pf, True, B)
    fresh.set_state(st)
    q0 = fresh.position()[0]
    inv_mass, eps = crude_inv_mass(q0), np.array([0.05, 0.1, 0.2, 0.15])
    want = diagonal_run(fresh, st, inv_mass, eps)
    C = metric_for(q0)
    dim = fresh.dim
    assert dim == 37

    lf = M.Leapfrog(lik, pf, True, B)
    lf.set_state(st)

    def refused(Cbad, code, *words):
        with pytest.raises(M.McdError) as ei:
            lf.set_metric(Cbad)
        assert ei.value.code == code and all(w in str(ei.value) for w in words), str(ei.value)
        assert lf.metric() is None
        assert same_bits(diagonal_run(lf, st, inv_mass, eps), want)

    bad = C.copy()
    bad[2, 9] += 1e-9 * math.sqrt(C[2, 2] * C[9, 9])                        # ten times the symmetry bound
    refused(bad, _capi.MCD_ERR_INVALID_ARG, "not symmetric", "C[2][9]", "C[9][2]")
    bad = C.copy()
    bad[5, 6] = bad[6, 5] = 1.5 * math.sqrt(C[5, 5] * C[6, 6])              # a correlation of 1.5: the 2 x 2 minor is indefinite
    refused(bad, _capi.MCD_ERR_INVALID_ARG, "not positive definite", "pivot 6")
    bad = C.copy()
    bad[7, 3] = np.nan
    refused(bad, _capi.MCD_ERR_INVALID_ARG, "C[7][3]", "not finite")
    bad = C.copy()
    bad[4, 4] = -bad[4, 4]
    refused(bad, _capi.MCD_ERR_INVALID_ARG, "not positive definite", "C[4][4]")
    with pytest.raises(ValueError):
        lf.set_metric(C[:-1, :-1])
    # with no dense metric a missing vector stays an error
    for call in (lambda: lf.nuts(eps, None), lambda: lf.nuts_run(2, eps, None), lambda: lf.leapfrog(np.zeros((B, dim)), eps, None, 1),
                 lambda: lf.step_from(q0, np.zeros((B, dim)), np.zeros((B, dim)), eps, None)):
        with pytest.raises(M.McdError) as ei:
            call()
        assert ei.value.code == _capi.MCD_ERR_INVALID_ARG
    assert same_bits(diagonal_run(lf, st, inv_mass, eps), want)
    # a vector passed while a dense metric is set: refused by every entry point, the metric stays
    lf.set_metric(C)
    stored = lf.metric()
    assert np.array_equal(stored, stored.T) and np.array_equal(stored, 0.5 * (C + C.T))
    lf.set_state(st)
    for call in (lambda: lf.nuts(eps, inv_mass), lambda: lf.nuts_run(2, eps, inv_mass), lambda: lf.leapfrog(np.zeros((B, dim)), eps, inv_mass, 1),
                 lambda: lf.step_from(q0, np.zeros((B, dim)), np.zeros((B, dim)), eps, inv_mass),
                 lambda: lf.nuts_warmup(eps, inv_mass, windows=1, window=2)):
        with pytest.raises(M.McdError) as ei:
            call()
        assert ei.value.code == _capi.MCD_ERR_INVALID_ARG and "a dense metric is set on this handle" in str(ei.value)
        assert np.array_equal(lf.metric(), stored)
    assert same_bits(lf.position(), fresh_position(lik, pf, st))            # nothing ran
    lf.clear_metric()
    assert lf.metric() is None
    assert same_bits(diagonal_run(lf, st, inv_mass, eps), want)
    # 401 nodes: more coordinates than a dense metric serves
    topo_b, lik_b, pf_b, st_b = synthetic_problem(201, 2, sparse=True)
    assert topo_b.n_nodes == 401
    big = M.Leapfrog(lik_b, pf_b, False, 2)
    big.set_state(st_b)
    assert big.dim > _capi.MCD_HMC_DENSE_MAX_DIM
    for call in (lambda: big.set_metric(np.eye(big.dim)), lambda: big.nuts_warmup_dense(0.01, np.ones(big.dim), windows=1, window=1)):
        with pytest.raises(M.McdError) as ei:
            call()
        assert ei.value.code == _capi.MCD_ERR_UNSUPPORTED and str(big.dim) in str(ei.value) and "512" in str(ei.value)
        assert big.metric() is None


def fresh_position(lik, pf, st):
    lf = M.Leapfrog(lik, pf, True, st.heights.shape[0])
    lf.set_state(st)
    return lf.position()


def test_set_then_clear_is_the_handle_that_never_had_a_dense_metric(gpu, golden):
    fx, topo, pf, lik, *_ = golden_problem(golden, "12-leaves-variable-rate")
    B = 6
    st = posterior_states(golden, "12-leaves-variable-rate", B)
    eps = np.array([0.05, 0.1, 0.2, 0.3, 0.15, 0.25])
    never = M.Leapfrog(lik, pf, True, B)
    never.set_state(st)
    q0 = never.position()[0]
    inv_mass = crude_inv_mass(q0)
    want = diagonal_run(never, st, inv_mass, eps)
    lf = M.Leapfrog(lik, pf, True, B)
    lf.set_state(st)
    lf.set_metric(metric_for(q0))
    a, d = lf.nuts(eps, None, max_depth=4, seed=41, transition=3)           # the dense metric has run, its buffers exist
    assert np.all(np.isfinite(a)) and not np.array_equal(lf.position()[0], want[2])
    lf.clear_metric()
    assert lf.metric() is None
    assert same_bits(diagonal_run(lf, st, inv_mass, eps), want)


def leapfrog_fixture(golden, which):
    """(likelihood, prior, calibrations available, states) of the four problems of the one-step tests."""
    if which in ("12-leaves-variable-rate", "24-leaves-braces"):
        B = 6 if which.startswith("12") else 5
        _, _, pf, lik, *_ = golden_problem(golden, which)
        return lik, pf, True, posterior_states(golden, which, B)
    if which == "synthetic-129":                                             # 257 nodes, dim 388: two coordinates per thread, no multiple of 64
        topo, lik, pf, st = synthetic_problem(129, 3, sparse=False)
        return lik, pf, True, st
    topo, lik, pf, st = synthetic_problem(33, 4, sparse=True)       # the 65-node sparse handle
    return lik, pf, False, st


FIXTURES = [("12-leaves-variable-rate", 37), ("24-leaves-braces", 73), ("synthetic-129", 388), ("sparse-33", 99)]


@pytest.mark.parametrize("which,dim", FIXTURES)
def test_one_leapfrog_step_against_numpy(gpu, golden, which, dim):
    lik, pf, cal, st = leapfrog_fixture(golden, which)
    B = st.heights.shape[0]
    lf = M.Leapfrog(lik, pf, cal, B)
    lf.set_state(st)
    assert lf.dim == dim
    q0, v0, g0 = lf.position()
    C = metric_for(q0)
    C = 0.5 * (C + C.T)
    U, W = M.metric_factors(C)
    # steps that stay inside the support: from the gradient in the metric's own scales (tests/test_gpu_sparse_hmc.py:415), different per chain
    eps = (1.0 + 0.5 * np.arange(B)) * 1e-2 / np.maximum(1.0, (np.abs(g0) * np.sqrt(np.diag(C))).max(axis=1))
    direction = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    p0 = np.random.default_rng(17).normal(size=(B, dim)) @ W.T
    lf.set_metric(C)
    q1, p2, g1, v1 = lf.step_from(q0, p0, g0, eps, None, direction=direction, have_grad=True)
    assert np.all(np.isfinite(q1)) and np.all(np.isfinite(p2)) and np.all(np.isfinite(v1))
    e = (eps * direction)[:, None]
    p1 = p0 + 0.5 * e * g0
    q_ref = q0 + e * (p1 @ C)
    # the rounding bound of a dim-term fp64 sum, per coordinate
    tol_q = 4 * dim * U53 * (np.abs(q0) + np.abs(e) * (np.abs(p1) @ np.abs(C)))
    err_q = np.abs(q1 - q_ref)
    print(f"{which}: q' error / bound {np.max(err_q / tol_q):.3f}")
    assert np.all(err_q <= tol_q), np.max(err_q / tol_q)
    assert np.all(np.abs(q1 - q0).max(axis=1) > 0)
    # the handle's state is the new point; the second half kick against the other gradient route (tests/test_gpu_nuts.py:167)
    mask = M.get_mask(cal, lf.topo)
    val, grad = M.target_grad(mask, lik, pf, lf.state())
    gmax = np.max(np.abs(grad))
    assert np.array_equal(lf.position()[0], q1)
    assert np.max(np.abs(grad - g1)) <= 1e-8 * gmax
    assert np.max(np.abs(val - v1) / np.maximum(1.0, np.abs(val))) <= 1e-10
    p_ref = p1 + 0.5 * e * grad
    tol_p = 0.5 * np.abs(e) * 1e-8 * gmax + 4 * U53 * np.abs(p_ref)
    assert np.all(np.abs(p2 - p_ref) <= tol_p), np.max(np.abs(p2 - p_ref) / tol_p)
    # mcd_hmc_leapfrog takes the same step through the fused kick + drift: the same bits for the position
    lf.set_state(st)
    p_l = lf.leapfrog(p0, eps, None, 1, direction=direction)
    assert np.array_equal(lf.position()[0], q1)
    assert np.all(np.abs(p_l - p_ref) <= tol_p)


def test_a_diagonal_matrix_as_dense_metric_against_the_diagonal_path(gpu, golden):
    name = "12-leaves-variable-rate"
    _, topo, pf, lik, *_ = golden_problem(golden, name)
    B = 6
    st = posterior_states(golden, name, B)
    eps = np.array([0.05, 0.1, 0.2, 0.3, 0.15, 0.25])
    direction = np.array([1.0, -1.0, 1.0, 1.0, -1.0, -1.0])
    diag = M.Leapfrog(lik, pf, True, B)
    dense = M.Leapfrog(lik, pf, True, B)
    diag.set_state(st)
    dense.set_state(st)
    q0, _, g0 = diag.position()
    v = crude_inv_mass(q0)
    dense.set_metric(np.diag(v))
    p0 = np.random.default_rng(2).normal(size=q0.shape) / np.sqrt(v)
    small = 0.2 * eps                                                       # one step that stays inside the support for every chain
    qa = diag.step_from(q0, p0, g0, small, v, direction=direction)[0]
    qb = dense.step_from(q0, p0, g0, small, None, direction=direction)[0]
    assert np.all(np.isfinite(qa)) and np.all(np.isfinite(qb))
    e = (small * direction)[:, None]
    p1 = p0 + 0.5 * e * g0
    # the zero terms add exactly; only the association of e v p differs
    assert np.all(np.abs(qa - qb) <= 8 * U53 * (np.abs(q0) + np.abs(e * v * p1)))
    # three transitions: the same trees
    diag.set_state(st)
    dense.set_state(st)
    for transition in range(3):
        a1, d1 = diag.nuts(eps, v, max_depth=5, seed=20261004, transition=transition)
        a2, d2 = dense.nuts(eps, None, max_depth=5, seed=20261004, transition=transition)
        q1, lp1, _ = diag.position()
        q2, lp2, _ = dense.position()
        assert np.array_equal(d1, d2), (transition, d1, d2)
        assert np.max(np.abs(a1 - a2)) <= 1e-6                               # tests/test_gpu_nuts.py:160-163
        assert np.max(np.abs(q1 - q2) / np.maximum(1e-3, np.abs(q1))) <= 1e-6
        assert np.all(np.abs(lp1 - lp2) <= 1e-6 * np.maximum(1.0, np.abs(lp1)))
    assert not np.array_equal(q1, q0)


def twin_transition_dense(tw, q0, g0, lp0, eps, C, max_depth, seed, chain, transition):
    """The state machine of tests/test_gpu_nuts.py:58-123 with a dense metric C = M^-1: momenta from numpy's own Cholesky factor."""
    dim = len(q0)

    def uni(d):
        return O.uniform_pair(seed, chain, transition, d)

    z = np.empty(dim)
    for k in range(dim):
        ua, ub = uni(0x4000 + (k >> 1))
        rad, ang = math.sqrt(-2.0 * math.log(ua)), 6.28318530717958647692 * ub
        z[k] = rad * math.sin(ang) if (k & 1) else rad * math.cos(ang)
    U = np.linalg.cholesky(C)
    p0 = np.linalg.solve(U.T, z)

    def kinetic(p):
        return 0.5 * float(p @ (C @ p))

    joint0 = lp0 - kinetic(p0)
    log_u = joint0 + math.log(uni(1)[0])
    minus = [q0.copy(), p0.copy(), g0.copy()]
    plus = [q0.copy(), p0.copy(), g0.copy()]
    prop = (q0.copy(), lp0)
    n, j, leaf, alpha, n_alpha = 1, 0, 0, 0.0, 0

    def no_u_turn(qm, rm, qp, rp):
        w = C @ (qp - qm)
        return float(w @ rm) >= 0.0 and float(w @ rp) >= 0.0

    while True:
        v = -1 if uni(0x10 + 2 * j)[0] < 0.5 else 1
        edge = minus if v < 0 else plus
        n1, s1, cand, stack = 0, True, None, {}
        for i in range(1 << j):
            q, p, g = edge
            e = eps * v
            p = p + 0.5 * e * g
            q = q + e * (C @ p)
            lp = tw.value(q)
            g = tw.grad(q) if math.isfinite(lp) else np.full(dim, np.nan)
            p = p + 0.5 * e * g
            edge[0], edge[1], edge[2] = q, p, g
            joint = lp - kinetic(p)
            if not math.isfinite(joint):
                joint = -math.inf
            nl, sl = log_u <= joint, log_u < TN.DELTA_MAX + joint
            if nl:
                n1 += 1
                if uni(0x100000 + leaf)[0] * n1 < 1.0:
                    cand = (q.copy(), lp)
            s1 = s1 and sl
            alpha += min(1.0, math.exp(min(0.0, joint - joint0)))
            n_alpha += 1
            for k in range(1, j + 1):
                size = 1 << k
                if i % size == 0:
                    stack[k] = (q.copy(), p.copy())
                elif (i + 1) % size == 0 and s1:
                    lq, lr = stack[k]
                    s1 = s1 and (no_u_turn(lq, lr, q, p) if v > 0 else no_u_turn(q, p, lq, lr))
            leaf += 1
            if not s1:
                break
        if not s1:
            return prop[0], prop[1], alpha / n_alpha, j + 1, n
        if n1 > 0 and uni(0x11 + 2 * j)[0] * n < n1:
            prop = cand
        n += n1
        s = no_u_turn(minus[0], minus[1], plus[0], plus[1])
        j += 1
        if not s or j >= max_depth:
            return prop[0], prop[1], alpha / n_alpha, j, n


@pytest.mark.parametrize("eps_scale", [1.0, 0.25])
def test_dense_nuts_follows_the_cpu_twin(gpu, golden, eps_scale):
    """12-leaves, B = 6, three transitions, max_depth 5, with the step sizes of tests/test_gpu_nuts.py:147 -- under this metric most of
    their trees end at the first leaf (it leaves the support) -- and with a quarter of them, where trees of every depth up to 5 are built
    and the U-turn tests of their sub trees run."""
    name = "12-leaves-variable-rate"
    fx, topo, pf, lik, spec, *_ = golden_problem(golden, name)
    B = 6
    st = posterior_states(golden, name, B)
    lf = M.Leapfrog(lik, pf, True, B)
    lf.set_state(st)
    mask = M.get_mask(True, topo)
    q0 = lf.position()[0]
    C = metric_for(q0)
    C = 0.5 * (C + C.T)
    lf.set_metric(C)
    eps = eps_scale * np.array([0.05, 0.1, 0.2, 0.3, 0.15, 0.25])
    seed, max_depth = 20261004, 5
    sub = M.Leapfrog(lik, pf, True, 3)                                      # chains 3 .. 5 alone
    sub.set_state(st.slice(3, 6))
    sub.set_metric(C)
    depths = []
    for transition in range(3):
        q_before, lp_before, g_before = lf.position()
        alpha, depth = lf.nuts(eps, None, max_depth=max_depth, seed=seed, transition=transition)
        q_after, lp_after, g_after = lf.position()
        for b in range(B):
            x_t = M.State(st.time_birth_rate[b], st.time_death_rate[b], st.time_height[b], st.heights[b], st.rate_mean[b], st.rate_variance[b],
                          st.rates[b])
            tw = TN.Twin(fx, spec, mask, x_t)
            assert abs(tw.value(q_before[b]) - lp_before[b]) <= 1e-9 * max(1.0, abs(lp_before[b]))
            qn, lpn, a, d, n = twin_transition_dense(tw, q_before[b], g_before[b], lp_before[b], eps[b], C, max_depth, seed, b, transition)
            assert d == depth[b], (transition, b, d, depth[b])
            assert abs(a - alpha[b]) <= 1e-6, (transition, b, a, alpha[b])
            assert np.max(np.abs(qn - q_after[b]) / np.maximum(1e-3, np.abs(qn))) <= 1e-6, (transition, b)
            assert abs(lpn - lp_after[b]) <= 1e-6 * max(1.0, abs(lpn))
        val, grad = M.target_grad(mask, lik, pf, lf.state())
        assert np.max(np.abs(val - lp_after) / np.maximum(1.0, np.abs(val))) <= 1e-10
        assert np.max(np.abs(grad - g_after)) <= 1e-8 * np.max(np.abs(grad))
        # a chain's draws and sums do not depend on the batch it runs in
        a_s, d_s = sub.nuts(eps[3:6], None, max_depth=max_depth, seed=seed, transition=transition, chain_offset=3)
        assert np.array_equal(d_s, depth[3:6]) and np.array_equal(a_s, alpha[3:6])
        assert same_bits(sub.position(), (q_after[3:6], lp_after[3:6], g_after[3:6]))
        depths += depth.tolist()
    print(f"dense twin, eps x {eps_scale}: depths {depths}")
    assert min(depths) >= 1 and max(depths) <= max_depth
    if eps_scale < 1.0:     # trees of several doublings were built, not every tree ended the same way, every chain has moved
        assert max(depths) >= 4 and len(set(depths)) >= 3 and np.all(np.any(q_after != q0, axis=1))


def test_warmup_takes_the_shrunk_covariance_of_the_window(gpu, golden):
    name = "12-leaves-variable-rate"
    _, topo, pf, lik, *_ = golden_problem(golden, name)
    B, windows, window = 64, 2, 20
    st = posterior_states(golden, name, B)
    mask = M.get_mask(True, topo)
    lf = M.Leapfrog(lik, pf, True, B)
    lf.set_state(st)
    q0 = lf.position()[0]
    im0 = crude_inv_mass(q0)
    kw = dict(windows=windows, window=window, delta=0.65, max_depth=6, seed=11)
    lf.record_begin(period=1, capacity=(windows + 1) * window)
    eps, C, alpha = lf.nuts_warmup_dense(0.02, im0, **kw)
    it, sc, H, R, post, nuts = lf.record_fetch()
    lf.record_end()
    assert it.tolist() == list(range(1, (windows + 1) * window + 1))
    # the metric of the closing window comes from the positions of the LAST adapting window: transitions 20 .. 39
    Q = np.array([M.to_vector(mask, M.State(sc[k, b, 0], sc[k, b, 1], sc[k, b, 2], H[k, b], sc[k, b, 3], sc[k, b, 4], R[k, b]))
                  for k in range(window, 2 * window) for b in range(B)])
    assert Q.shape == (B * window, lf.dim) and np.all(np.isfinite(Q))
    ref = M.shrunk_covariance(Q)
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    # the sum's rounding bound n 2^-53 = 1.4e-13 at n = 1280, two orders of margin for numpy's other order of summation
    err = np.max(np.abs(C - ref) / scale)
    print(f"warm-up covariance: max |C - ref| / sqrt(C_ii C_jj) = {err:.2e}")
    assert err <= 1e-11
    assert np.array_equal(C, C.T) and np.array_equal(lf.metric(), C)
    assert np.all((eps > 1e-3) & (eps < 1.0)) and np.all(np.isfinite(alpha))
    # the step sizes the closing window used are those tuned against C: the recorded ones of the last transition are finite and positive
    assert np.all(nuts[-1, :, 4] > 0)
    end = lf.position()
    # again from the same state: the same bits (a dense metric on the handle is cleared first); without the recorder: the same bits
    for recorded in (True, False):
        lf.set_state(st)
        if recorded:
            lf.record_begin(period=1, capacity=(windows + 1) * window)
        eps2, C2, alpha2 = lf.nuts_warmup_dense(0.02, im0, **kw)
        if recorded:
            lf.record_end()
        assert np.array_equal(eps2, eps) and np.array_equal(C2, C) and np.array_equal(alpha2, alpha), recorded
        assert same_bits(lf.position(), end)
    # a call whose samples would not fit the ring is refused up front
    lf.set_state(st)
    lf.record_begin(period=1, capacity=(windows + 1) * window - 1)
    with pytest.raises(M.McdError) as ei:
        lf.nuts_warmup_dense(0.02, im0, **kw)
    assert ei.value.code == _capi.MCD_ERR_INVALID_ARG and lf.record_count() == 0
    lf.record_end()
    assert same_bits(lf.position(), fresh_position(lik, pf, st))


def test_dense_warmup_then_sampling_agrees_with_metropolis_hastings_chains(gpu, golden):
    """tests/test_gpu_nuts.py:182-229 at 12 leaves x 64 chains with the metric tuned by mcd_hmc_nuts_warmup_dense from the crude start
    (0.1 q)^2: inner node-age means within 3 %, mean acceptance statistic in (0.45, 0.9)."""
    from mcmc_date_amd import monitor as MO

    name, B = "12-leaves-variable-rate", 64
    fx, topo, pf, lik, _, br, ht = golden_problem(golden, name)
    ps, _ = M.proposals(topo, br, calibrations_available=True, exact_jacobians=True)
    ps = [dataclasses.replace(p, jac_root=1) for p in ps]
    smp = M.Sampler(lik, pf, ps, B, seed=78)
    x0 = M.init_with(topo, fx["mean_lengths"])
    x0.time_height = ht
    smp.set_initial_state(x0)
    smp.burn_in(fast=[10, 10, 20, 40, 80], slow=[100, 200, 300, 400])
    MO.collect(smp, 3000, period=50, accumulate=True)
    ages_mh = smp.node_age_summary()[0]
    lf = M.Leapfrog(lik, pf, True, B)
    lf.set_state(smp.state())
    q0 = lf.position()[0]
    eps, C, alpha_c = lf.nuts_warmup_dense(0.02, crude_inv_mass(q0), windows=3, window=60, delta=0.65, max_depth=6, seed=11)
    assert np.all((eps > 1e-3) & (eps < 1.0)) and np.array_equal(lf.metric(), C)
    n_tr = 300
    ages = np.zeros(topo.n_nodes)
    alphas = []
    for t in range(n_tr):
        a, d = lf.nuts(eps, None, max_depth=6, seed=5, transition=1000 + t)
        alphas.append(a.mean())
        s = lf.state()
        ages += (s.time_height[:, None] * s.heights).mean(axis=0)
    ages /= n_tr
    inner = ~topo.leaves
    rel = np.abs(ages[inner] - ages_mh[inner]) / ages_mh[inner]
    print(f"dense metric: mean alpha {np.mean(alphas):.3f}, max relative age difference {rel.max():.4f}, eps {eps.mean():.3f}")
    assert 0.45 < np.mean(alphas) < 0.9, np.mean(alphas)
    assert rel.max() <= 0.03, (rel, np.mean(alphas))
