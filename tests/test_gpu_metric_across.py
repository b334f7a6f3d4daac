"""The dense metric's across-chains form (mcd_hmc_set_metric_form, MCD_HMC_METRIC_ACROSS_CHAINS; csrc/k_metric_gemm.hip,
k_nuts_across.hip): the products with C and U^-1 of all lock-step chains as rows of one matrix product, so a dense metric serves positions
of more than 512 coordinates.

The definitions are the per-chain form's (tests/test_gpu_dense_metric.py, whose problems, metric and CPU twin are used here): references
are numpy on the handle's own gradient for one leapfrog step, the per-chain form and the diagonal path for whole transitions, the CPU twin
at 12 leaves, numpy's momenta for the start of a transition at dim 513, hmc.shrunk_covariance for the warm-up.  A position has
3 L + (1 if calibrations) coordinates for a bifurcating tree of L leaves: 171 leaves give dim 513 / 514, 172 leaves 516."""
import ctypes
import math

import numpy as np
import pytest

import mcmc_date_amd as M
import oracle as O
import test_gpu_nuts as TN
from mcmc_date_amd import _capi
from test_gpu_dense_metric import (FIXTURES, crude_inv_mass, diagonal_run, golden_problem, leapfrog_fixture, metric_for, posterior_states, same_bits,
                                   synthetic_problem, twin_transition_dense)

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
NAME12 = "12-leaves-variable-rate"


def across(lik, pf, cal, B):
    lf = M.Leapfrog(lik, pf, cal, B)
    lf.set_metric_form("across_chains")
    return lf


def safe_eps(g0, C, B):
    """Steps that stay inside the support, different per chain (tests/test_gpu_dense_metric.py:231)."""
    return (1.0 + 0.5 * np.arange(B)) * 1e-2 / np.maximum(1.0, (np.abs(g0) * np.sqrt(np.diag(C))).max(axis=1))


def test_a_dense_metric_at_dim_513_needs_the_across_chains_form(gpu):
    for cal, dim in ((False, 513), (True, 514)):
        topo, lik, pf, st = synthetic_problem(171, 3, sparse=True)
        assert topo.n_nodes == 341
        never = M.Leapfrog(lik, pf, cal, 3)
        never.set_state(st)
        assert never.dim == dim > _capi.MCD_HMC_DENSE_MAX_DIM
        q0, _, g0 = never.position()
        C = metric_for(q0)
        inv_mass = crude_inv_mass(q0)
        eps = safe_eps(g0, np.diag(inv_mass), 3)
        want = diagonal_run(never, st, inv_mass, eps)
        lf = M.Leapfrog(lik, pf, cal, 3)
        lf.set_state(st)
        assert lf.metric_form == "per_chain"
        with pytest.raises(M.McdError) as ei:                                   # the default form: refused as before
            lf.set_metric(C)
        assert ei.value.code == _capi.MCD_ERR_UNSUPPORTED and str(dim) in str(ei.value) and "512" in str(ei.value)
        assert lf.metric() is None
        lf.set_metric_form("across_chains")
        assert lf.metric_form == "across_chains"
        lf.set_metric(C)
        stored = lf.metric()
        assert np.array_equal(stored, 0.5 * (C + C.T)) and np.array_equal(stored, stored.T)
        # the form is fixed while a metric is set; a value that is no form is refused as well
        for call in (lambda: lf.set_metric_form("per_chain"), lambda: _capi.check(_capi.lib().mcd_hmc_set_metric_form(lf._h, 7))):
            with pytest.raises(M.McdError) as ei:
                call()
            assert ei.value.code == _capi.MCD_ERR_INVALID_ARG
            assert lf.metric_form == "across_chains" and np.array_equal(lf.metric(), stored)
        with pytest.raises(ValueError):
            lf.set_metric_form("both")
        a, d = lf.nuts(eps, None, max_depth=3, seed=41, transition=3)           # the dense metric has run, its buffers exist
        assert np.all(np.isfinite(a)) and not np.array_equal(lf.position()[0], want[2])
        lf.clear_metric()
        assert lf.metric() is None and lf.metric_form == "across_chains"
        assert same_bits(diagonal_run(lf, st, inv_mass, eps), want)


def one_step(lf, lik, pf, cal, st, C, eps, direction, p0):
    """tests/test_gpu_dense_metric.py:234-260 on a handle whose metric is set: the step against numpy, the handle's state, the second half
    kick, mcd_hmc_leapfrog's bits.  Returns (q', bound of q')."""
    dim = lf.dim
    lf.set_state(st)
    q0, v0, g0 = lf.position()
    q1, p2, g1, v1 = lf.step_from(q0, p0, g0, eps, None, direction=direction, have_grad=True)
    assert np.all(np.isfinite(q1)) and np.all(np.isfinite(p2)) and np.all(np.isfinite(v1))
    e = (eps * direction)[:, None]
    p1 = p0 + 0.5 * e * g0
    q_ref = q0 + e * (p1 @ C)
    tol_q = 4 * dim * U53 * (np.abs(q0) + np.abs(e) * (np.abs(p1) @ np.abs(C)))      # the rounding bound of a dim-term fp64 sum, in any order
    err_q = np.abs(q1 - q_ref)
    print(f"dim {dim}, B {lf.batch}: q' error / bound {np.max(err_q / tol_q):.3f}")
    assert np.all(err_q <= tol_q), np.max(err_q / tol_q)
    assert np.all(np.abs(q1 - q0).max(axis=1) > 0)
    mask = M.get_mask(cal, lf.topo)
    val, grad = M.target_grad(mask, lik, pf, lf.state())
    gmax = np.max(np.abs(grad))
    assert np.array_equal(lf.position()[0], q1)
    assert np.max(np.abs(grad - g1)) <= 1e-8 * gmax
    assert np.max(np.abs(val - v1) / np.maximum(1.0, np.abs(val))) <= 1e-10
    p_ref = p1 + 0.5 * e * grad
    tol_p = 0.5 * np.abs(e) * 1e-8 * gmax + 4 * U53 * np.abs(p_ref)
    assert np.all(np.abs(p2 - p_ref) <= tol_p), np.max(np.abs(p2 - p_ref) / tol_p)
    lf.set_state(st)
    p_l = lf.leapfrog(p0, eps, None, 1, direction=direction)
    assert np.array_equal(lf.position()[0], q1)                                  # the same position bits through mcd_hmc_leapfrog
    assert np.all(np.abs(p_l - p_ref) <= tol_p)
    return q1, tol_q


def step_inputs(lik, pf, cal, st):
    """(C, eps, direction, p0) of the one-step tests, from a handle without a metric."""
    B = st.heights.shape[0]
    lf = M.Leapfrog(lik, pf, cal, B)
    lf.set_state(st)
    q0, _, g0 = lf.position()
    C = metric_for(q0)
    C = 0.5 * (C + C.T)
    _, W = M.metric_factors(C)
    eps = safe_eps(g0, C, B)
    direction = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    p0 = np.random.default_rng(17).normal(size=(B, lf.dim)) @ W.T
    return C, eps, direction, p0


BIG = [(171, False, 513), (171, True, 514), (172, False, 516)]                  # dim = 1, 2, 0 mod 4 and 1, 2, 4 mod 16


@pytest.mark.parametrize("which,dim", FIXTURES + [(f"synthetic-{L}-{int(cal)}", dim) for L, cal, dim in BIG])
def test_one_leapfrog_step_against_numpy(gpu, golden, which, dim):
    if dim > 512:
        L, cal = next((L, cal) for L, cal, d in BIG if d == dim)
        _, lik, pf, st = synthetic_problem(L, 3, sparse=True)
    else:
        lik, pf, cal, st = leapfrog_fixture(golden, which)
    C, eps, direction, p0 = step_inputs(lik, pf, cal, st)
    lf = across(lik, pf, cal, st.heights.shape[0])
    assert lf.dim == dim
    lf.set_metric(C)
    one_step(lf, lik, pf, cal, st, C, eps, direction, p0)


@pytest.mark.parametrize("B", [15, 16, 17, 33, 49, 64, 65, 130])
def test_row_tiles_and_the_chain_alone(gpu, B):
    """65 nodes (dim 99): batches around one 16-row operand tile and over two, into the fourth wave's rows (48 ..), up to a full 64-row
    tile, one row and two tiles and two rows beyond it; every chain against itself run alone (from 49 chains on: the chains at the
    edges of the waves' rows and of the tiles)."""
    _, lik, pf, st = synthetic_problem(33, B, sparse=True)
    C, eps, direction, p0 = step_inputs(lik, pf, False, st)
    lf = across(lik, pf, False, B)
    assert lf.dim == 99
    lf.set_metric(C)
    q1, _ = one_step(lf, lik, pf, False, st, C, eps, direction, p0)
    lf.set_state(st)
    q0, _, g0 = lf.position()
    q1, p1, g1, v1 = lf.step_from(q0, p0, g0, eps, None, direction=direction, have_grad=True)
    alone = across(lik, pf, False, 1)
    alone.set_metric(C)
    for b in (range(B) if B <= 33 else sorted({b for b in (0, 15, 16, 47, 48, 63, 64, B - 1) if b < B})):
        alone.set_state(st.slice(b, b + 1))
        got = alone.step_from(q0[b:b + 1], p0[b:b + 1], g0[b:b + 1], eps[b:b + 1], None, direction=direction[b:b + 1], have_grad=True)
        assert same_bits(got, (q1[b:b + 1], p1[b:b + 1], g1[b:b + 1], v1[b:b + 1])), b


def test_across_chains_against_per_chain(gpu, golden):
    _, topo, pf, lik, *_ = golden_problem(golden, NAME12)
    B = 6
    st = posterior_states(golden, NAME12, B)
    C, eps1, direction, p0 = step_inputs(lik, pf, True, st)
    per = M.Leapfrog(lik, pf, True, B)
    acr = across(lik, pf, True, B)
    assert per.metric_form == "per_chain" and acr.metric_form == "across_chains"
    for lf in (per, acr):
        lf.set_state(st)
        lf.set_metric(C)
    q0, _, g0 = per.position()
    qa = per.step_from(q0, p0, g0, eps1, None, direction=direction)[0]
    qb = acr.step_from(q0, p0, g0, eps1, None, direction=direction)[0]
    e = (eps1 * direction)[:, None]
    p1 = p0 + 0.5 * e * g0
    tol_q = 4 * per.dim * U53 * (np.abs(q0) + np.abs(e) * (np.abs(p1) @ np.abs(C)))
    assert np.all(np.isfinite(qa)) and np.all(np.abs(qa - qb) <= 2 * tol_q)
    eps = 0.25 * np.array([0.05, 0.1, 0.2, 0.3, 0.15, 0.25])
    per.set_state(st)
    acr.set_state(st)
    depths = []
    for transition in range(3):
        a1, d1 = per.nuts(eps, None, max_depth=5, seed=20261004, transition=transition)
        a2, d2 = acr.nuts(eps, None, max_depth=5, seed=20261004, transition=transition)
        q1, lp1, _ = per.position()
        q2, lp2, _ = acr.position()
        assert np.array_equal(d1, d2), (transition, d1, d2)
        assert np.max(np.abs(a1 - a2)) <= 1e-6
        assert np.max(np.abs(q1 - q2) / np.maximum(1e-3, np.abs(q1))) <= 1e-6
        assert np.all(np.abs(lp1 - lp2) <= 1e-6 * np.maximum(1.0, np.abs(lp1)))
        depths += d2.tolist()
    print(f"across against per chain: depths {depths}")
    assert max(depths) >= 4 and not np.array_equal(q2, q0)


def rhs_count(r):
    """nuts_rhs_plan(j, i).count of round r = 2^j + i - 1 (csrc/nuts_rhs_plan.hpp; pinned by tests/test_nuts_rhs_plan_host.py)."""
    j = (r + 1).bit_length() - 1
    i = r + 1 - (1 << j)
    closes = next(k for k in range(j + 1) if k == j or (i + 1) % (2 << k))
    return 1 + closes + int(i + 1 == 1 << j)


def spread_eps(lik, pf, st, scale, ratio):
    """Step sizes from `scale` to `scale x ratio` times each chain's safe unit (safe_eps without its ramp), the exponents dealt over the
    chains by a fixed permutation so that every row tile holds short and long steps."""
    B = st.heights.shape[0]
    lf = M.Leapfrog(lik, pf, False, B)
    lf.set_state(st)
    q0, _, g0 = lf.position()
    C = metric_for(q0)
    unit = 1.0 / np.maximum(1.0, (np.abs(g0) * np.sqrt(np.diag(C))).max(axis=1))
    u = np.random.default_rng(130).permutation(B) / (B - 1.0)
    return scale * unit * ratio ** u


EPS_130 = dict(scale=1.0, ratio=30.0)


def test_across_chains_nuts_at_130_chains(gpu):
    """The across-chains NUTS at a production row count: 130 chains (two full 64-row tiles and two rows), dim 99, trees of up to 15
    leaves that end at different leaves, so the rounds' products run over lists of every length.  The per-chain form on the same chains
    is the reference; the same bits from the same state again and for chains 60 .. 69 (across the 64-row edge) run alone.

    Measured on the MI355X: chains still building per round 130, 120, 118, 101, 101, 97, 95, 70, 69, 67, 66, 65, 65, 63, 60 in the first
    transition and 130, 120, 116, 103, 101, 99, 96, 82, 82, 81, 78, 76, 74, 72, 71 in the second; depths 1 .. 4 of 10, 19, 31, 70 chains."""
    B, max_depth, seed, transitions = 130, 4, 20261021, 2
    _, lik, pf, st = synthetic_problem(33, B, sparse=True)
    C = step_inputs(lik, pf, False, st)[0]
    eps = spread_eps(lik, pf, st, **EPS_130)
    assert eps.max() >= 30 * eps.min()
    per = M.Leapfrog(lik, pf, False, B)
    acr = across(lik, pf, False, B)
    sub = across(lik, pf, False, 10)
    assert per.dim == 99 and per.metric_form == "per_chain" and acr.metric_form == "across_chains"
    for lf, s in ((per, st), (acr, st), (sub, st.slice(60, 70))):
        lf.set_state(s)
        lf.set_metric(C)
    q0 = acr.position()[0]
    per.record_begin(period=1, capacity=transitions)
    acr.record_begin(period=1, capacity=transitions)
    runs = []
    for transition in range(transitions):
        a1, d1 = per.nuts(eps, None, max_depth=max_depth, seed=seed, transition=transition)
        a2, d2 = acr.nuts(eps, None, max_depth=max_depth, seed=seed, transition=transition)
        q1, lp1, _ = per.position()
        q2, lp2, g2 = acr.position()
        assert np.array_equal(d1, d2), (transition, np.flatnonzero(d1 != d2))
        assert np.max(np.abs(a1 - a2)) <= 1e-6
        assert np.max(np.abs(q1 - q2) / np.maximum(1e-3, np.abs(q1))) <= 1e-6
        assert np.all(np.abs(lp1 - lp2) <= 1e-6 * np.maximum(1.0, np.abs(lp1)))
        a_s, d_s = sub.nuts(eps[60:70], None, max_depth=max_depth, seed=seed, transition=transition, chain_offset=60)
        assert np.array_equal(d_s, d2[60:70]) and np.array_equal(a_s, a2[60:70])
        assert same_bits(sub.position(), (q2[60:70], lp2[60:70], g2[60:70]))
        runs.append((a2, d2, q2, lp2, g2))
    steps = per.record_fetch()[5][:, :, 1]
    nuts_a = acr.record_fetch()[5]
    per.record_end()
    acr.record_end()
    assert steps.shape == (transitions, B) and np.array_equal(nuts_a[:, :, 1], steps)      # equal leapfrog counts, chain by chain
    assert np.array_equal(nuts_a[:, :, 0], np.array([r[1] for r in runs]))
    # the same calls again from the same state, on the handle whose workspace and list the first run has used
    acr.set_state(st)
    for transition in range(transitions):
        a2, d2 = acr.nuts(eps, None, max_depth=max_depth, seed=seed, transition=transition)
        assert same_bits((a2, d2) + acr.position(), runs[transition]), transition
    assert np.mean(np.any(runs[-1][2] != q0, axis=1)) > 0.5                                # most chains have moved
    # what the rounds' products have covered, from the reference's counts: n_r chains are still building in round r
    n_r = [[int(np.sum(steps[t] > r)) for r in range(1 << max_depth)] for t in range(transitions)]
    print(f"across-chains NUTS at {B} chains: chains per round {n_r}, depths {np.bincount(runs[0][1], minlength=max_depth + 1).tolist()}")
    rounds = [(r, n) for per_t in n_r for r, n in enumerate(per_t)]
    assert any(r >= 1 and n > 64 and n % 64 != 0 for r, n in rounds)                        # a ragged second row tile through the list
    assert any(0 < n < 64 and n % 16 != 0 for r, n in rounds)                               # a ragged wave of a single tile
    assert any(rhs_count(r) >= 2 and rhs_count(r) * n > 64 for r, n in rounds)              # several slots, more than one tile of rows
    assert any(r >= 1 and rhs_count(r) >= 2 and n < B and rhs_count(r) * n > 64 for r, n in rounds)   # ... of a list shorter than the batch


@pytest.mark.parametrize("eps_scale", [1.0, 0.25])
def test_across_chains_nuts_follows_the_cpu_twin(gpu, golden, eps_scale):
    """tests/test_gpu_dense_metric.py:376-422 with the across-chains form, its sub-batch check included."""
    fx, topo, pf, lik, spec, *_ = golden_problem(golden, NAME12)
    B = 6
    st = posterior_states(golden, NAME12, B)
    lf = across(lik, pf, True, B)
    lf.set_state(st)
    mask = M.get_mask(True, topo)
    q0 = lf.position()[0]
    C = metric_for(q0)
    C = 0.5 * (C + C.T)
    lf.set_metric(C)
    eps = eps_scale * np.array([0.05, 0.1, 0.2, 0.3, 0.15, 0.25])
    seed, max_depth = 20261004, 5
    sub = across(lik, pf, True, 3)                                          # chains 3 .. 5 alone
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
        a_s, d_s = sub.nuts(eps[3:6], None, max_depth=max_depth, seed=seed, transition=transition, chain_offset=3)
        assert np.array_equal(d_s, depth[3:6]) and np.array_equal(a_s, alpha[3:6])
        assert same_bits(sub.position(), (q_after[3:6], lp_after[3:6], g_after[3:6]))
        depths += depth.tolist()
    print(f"across-chains twin, eps x {eps_scale}: depths {depths}")
    assert min(depths) >= 1 and max(depths) <= max_depth
    if eps_scale < 1.0:
        assert max(depths) >= 4 and len(set(depths)) >= 3 and np.all(np.any(q_after != q0, axis=1))


def problem_513(B):
    topo, lik, pf, st = synthetic_problem(171, B, sparse=True)
    lf = M.Leapfrog(lik, pf, False, B)
    lf.set_state(st)
    q0, lp0, g0 = lf.position()
    assert lf.dim == 513
    return topo, lik, pf, st, q0, lp0, g0


def test_nuts_at_dim_513_with_a_diagonal_matrix_against_the_diagonal_path(gpu):
    """tests/test_gpu_dense_metric.py:263-298 at a dim the per-chain form cannot reach: steps so small that no tree turns, so every tree
    has max_depth = 3 doublings and every round with several right-hand sides runs (leaves 1, 3, 5, 6 of the transition)."""
    B = 3
    topo, lik, pf, st, q0, _, g0 = problem_513(B)
    v = crude_inv_mass(q0)
    eps = safe_eps(g0, np.diag(v), B)
    diag = M.Leapfrog(lik, pf, False, B)
    dense = across(lik, pf, False, B)
    diag.set_state(st)
    dense.set_state(st)
    dense.set_metric(np.diag(v))
    for transition in range(2):
        a1, d1 = diag.nuts(eps, v, max_depth=3, seed=20261004, transition=transition)
        a2, d2 = dense.nuts(eps, None, max_depth=3, seed=20261004, transition=transition)
        q1, lp1, _ = diag.position()
        q2, lp2, _ = dense.position()
        print(f"dim 513, diagonal matrix, transition {transition}: depths {d1.tolist()} {d2.tolist()}")
        assert np.array_equal(d1, d2), (transition, d1, d2)
        assert np.max(np.abs(a1 - a2)) <= 1e-6
        assert np.max(np.abs(q1 - q2) / np.maximum(1e-3, np.abs(q1))) <= 1e-6
        assert np.all(np.abs(lp1 - lp2) <= 1e-6 * np.maximum(1.0, np.abs(lp1)))
        assert d2.max() == 3
    assert not np.array_equal(q2, q0)


def normal_draws(seed, chain, transition, dim):
    z = np.empty(dim)
    for k in range(dim):
        ua, ub = O.uniform_pair(seed, chain, transition, 0x4000 + (k >> 1))
        rad, ang = math.sqrt(-2.0 * math.log(ua)), 6.28318530717958647692 * ub
        z[k] = rad * math.sin(ang) if (k & 1) else rad * math.cos(ang)
    return z


def test_nuts_at_dim_513_momenta_state_and_sub_batch(gpu):
    B, seed = 3, 77
    topo, lik, pf, st, q0, _, g0 = problem_513(B)
    C = metric_for(q0)
    C = 0.5 * (C + C.T)
    U = np.linalg.cholesky(C)
    kappa = np.linalg.cond(C)
    eps = safe_eps(g0, C, B)
    lf = across(lik, pf, False, B)
    lf.set_state(st)
    lf.set_metric(C)
    sub = across(lik, pf, False, 2)                                          # chains 1 .. 2 alone
    sub.set_state(st.slice(1, 3))
    sub.set_metric(C)
    mask = M.get_mask(False, topo)
    lf.record_begin(period=1, capacity=4)
    for transition in range(2):
        value = lf.position()[1]
        alpha, depth = lf.nuts(eps, None, max_depth=3, seed=seed, transition=transition)
        q_after, lp_after, g_after = lf.position()
        joint0 = lf.record_fetch()[5][-1, :, 5]                                # -H at the start of the transition
        for b in range(B):
            p = np.linalg.solve(U.T, normal_draws(seed, b, transition, 513))
            kin = 0.5 * float(p @ (C @ p))
            tol = 64 * 513 * U53 * kappa * (abs(value[b]) + kin)              # SURVEY.md 8c; a wrong triangular product is off by O(kin)
            print(f"dim 513, transition {transition}, chain {b}: |joint0 - ref| {abs(joint0[b] - (value[b] - kin)):.2e}, bound {tol:.2e}, kin {kin:.1f}")
            assert abs(joint0[b] - (value[b] - kin)) <= tol
            assert tol < 1e-3 * kin
        val, grad = M.target_grad(mask, lik, pf, lf.state())
        assert np.max(np.abs(val - lp_after) / np.maximum(1.0, np.abs(val))) <= 1e-10
        assert np.max(np.abs(grad - g_after)) <= 1e-8 * np.max(np.abs(grad))
        a_s, d_s = sub.nuts(eps[1:3], None, max_depth=3, seed=seed, transition=transition, chain_offset=1)
        assert np.array_equal(d_s, depth[1:3]) and np.array_equal(a_s, alpha[1:3])
        assert same_bits(sub.position(), (q_after[1:3], lp_after[1:3], g_after[1:3]))
    lf.record_end()
    assert np.all(np.any(q_after != q0, axis=1))


def test_a_chain_that_leaves_the_support_touches_no_other(gpu):
    B, seed = 3, 5
    topo, lik, pf, st, q0, lp0, g0 = problem_513(B)
    C = metric_for(q0)
    eps = safe_eps(g0, C, B)
    lf = across(lik, pf, False, B)
    lf.set_metric(C)
    runs = []
    for eps1 in (1e-9 * eps[1], 1e4):                                          # tiny; enormous: the first leaf leaves the support
        lf.set_state(st)
        lf.record_begin(period=1, capacity=1)
        a, d = lf.nuts(np.array([eps[0], eps1, eps[2]]), None, max_depth=3, seed=seed, transition=0)
        nuts = lf.record_fetch()[5][0]
        lf.record_end()
        runs.append((a, d, nuts) + lf.position())
    tiny, huge = runs
    for b in (0, 2):
        assert same_bits([x[b] for x in tiny], [x[b] for x in huge]), b
        assert not np.array_equal(huge[3][b], q0[b])
    assert tiny[2][1, 3] == 0 and huge[2][1, 3] == 1                           # the diverged flag of chain 1
    assert huge[1][1] == 1 and np.array_equal(huge[3][1], q0[1]) and huge[4][1] == lp0[1] and np.array_equal(huge[5][1], g0[1])


def test_warmup_at_dim_513_takes_the_shrunk_covariance_of_the_window(gpu):
    B, windows, window = 4, 1, 4
    topo, lik, pf, st = synthetic_problem(171, B, sparse=True)
    mask = M.get_mask(False, topo)
    lf = across(lik, pf, False, B)
    lf.set_state(st)
    q0, _, g0 = lf.position()
    assert lf.dim == 513
    im0 = crude_inv_mass(q0)
    eps0 = safe_eps(g0, np.diag(im0), B)
    lf.record_begin(period=1, capacity=(windows + 1) * window)
    eps, C, alpha = lf.nuts_warmup_dense(eps0, im0, windows=windows, window=window, delta=0.65, max_depth=2, seed=11)
    it, sc, H, R, post, nuts = lf.record_fetch()
    lf.record_end()
    assert it.tolist() == list(range(1, (windows + 1) * window + 1))
    Q = np.array([M.to_vector(mask, M.State(sc[k, b, 0], sc[k, b, 1], sc[k, b, 2], H[k, b], sc[k, b, 3], sc[k, b, 4], R[k, b]))
                  for k in range(window) for b in range(B)])
    assert Q.shape == (B * window, 513) and np.all(np.isfinite(Q))
    ref = M.shrunk_covariance(Q)
    # 16 positions in 513 dimensions: the covariance is singular, the shrinkage term alone makes the metric positive definite
    assert np.linalg.matrix_rank(ref - np.diag(np.full(513, 1e-3 * 5.0 / (16 + 5.0)))) < 16
    assert np.linalg.eigvalsh(ref).min() > 0
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    err = np.max(np.abs(C - ref) / scale)
    print(f"warm-up covariance at dim 513: max |C - ref| / sqrt(C_ii C_jj) = {err:.2e}")
    assert err <= 1e-11
    assert np.array_equal(C, C.T) and np.array_equal(lf.metric(), C) and lf.metric_form == "across_chains"
    assert np.all(np.isfinite(eps)) and np.all(eps > 0) and np.all(np.isfinite(alpha))
    assert not np.array_equal(Q[-B:], Q[:B])                                   # the chains moved inside the window
