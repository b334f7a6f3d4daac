"""The Hamiltonian side over the sparse likelihood: mcd_sparse_tree_grad_batch (csrc/k_sparse_grad.hip: tree state -> ln likelihood and
its state gradient over the sparse precision matrix, one launch), the prior gradient up to 2048 nodes, and the leapfrog / NUTS driver
over a sparse handle (mcd_hmc_create_sparse).

References: oracle.tree_grad_full / oracle.tree_loglik_full_batch on the densified matrix for the gradient kernel; hamiltonian.target_grad,
a dense Leapfrog over the same matrix densified, the CPU twin of tests/test_gpu_nuts.py and sparse Metropolis-Hastings chains for the
driver.  Tolerances are the project's for the same comparisons elsewhere (the lines are named where they are used)."""
import dataclasses

import numpy as np
import pytest

import mcmc_date_amd as M
import oracle as O
import test_gpu_nuts as TN
from mcmc_date_amd import _capi
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

def assoc_of(P):
    ii, jj = np.nonzero(P)
    return [((int(i), int(j)), float(P[i, j])) for i, j in zip(ii, jj)]


def thinned(P):
    """Off-diagonal entries below 5 % of sqrt(P_ii P_jj) dropped, their magnitudes added to the diagonal of their row: P plus a
    symmetric, diagonally dominant correction, hence still positive definite."""
    P = np.asarray(P, float)
    d = np.sqrt(np.diag(P))
    drop = (np.abs(P) < 0.05 * np.outer(d, d)) & ~np.eye(len(P), dtype=bool)
    Pt = np.where(drop, 0.0, P)
    Pt[np.diag_indices_from(Pt)] += np.abs(P * drop).sum(axis=1)
    assert drop.any() and np.linalg.eigvalsh(0.5 * (Pt + Pt.T)).min() > 0      # (the golden matrix is symmetric to rounding only)
    return Pt


def check_against_oracle(topo, st, mu, P_value, logdet, out, P_grad=None):
    """ll of every chain against oracle.tree_loglik_full_batch on P_value, the gradient against oracle.tree_grad_full on P_grad
    (P_value unless given): ll to 1e-11 relative (tests/test_gpu_sparse.py:94), each gradient array to 1e-11 x its largest entry."""
    P_grad = P_value if P_grad is None else P_grad
    ll, gH, gR, gt, gm = (np.asarray(a) for a in out)
    B = st.heights.shape[0]
    ref_ll, _ = O.tree_loglik_full_batch(topo.parent, st.heights, st.rates, st.time_height, st.rate_mean, mu, P_value, logdet)
    ref = [O.tree_grad_full(topo.parent, st.heights[b], st.rates[b], st.time_height[b], st.rate_mean[b], mu, P_grad) for b in range(B)]
    rH, rR = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
    rt, rm = np.array([r[2] for r in ref]), np.array([r[3] for r in ref])
    e_ll = np.max(np.abs(ll - ref_ll) / np.abs(ref_ll))
    errs = {k: np.max(np.abs(a - r)) / np.max(np.abs(r)) for k, a, r in (("gH", gH, rH), ("gR", gR, rR), ("gtH", gt, rt), ("grMu", gm, rm))}
    print(f"n_nodes {topo.n_nodes}: ll {e_ll:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert e_ll <= 1e-11, e_ll
    for k, v in errs.items():
        assert v <= 1e-11, (k, v)
    assert np.all(gR[:, 0] == 0.0)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("n_leaves", [4, 33, 130, 1007, 1024])
def test_sparse_tree_gradient_against_the_oracle(gpu, knobs, n_leaves):
    """7, 65 (a row range that is no multiple of a wave), 259, 2013 and 2047 nodes (the last size that fits), B = 5 (a two-chain
    workgroup has a ragged tail)."""
    import torch

    topo = S.random_topology(n_leaves, seed=11)
    n = topo.n_nodes - 2
    P, assoc = S.banded_precision(n, seed=n_leaves)
    Pd = P.toarray()
    rng = np.random.default_rng(n_leaves)
    mu = rng.uniform(0.01, 0.2, n)
    logdet = -float(np.linalg.slogdet(Pd)[1])
    tl = M.SparseLikelihood(M.Sparse(mu, assoc, logdet)).bind_tree(topo)
    B = 5
    st = S.random_states(topo, B, seed=3)
    out = tl.grad(st)
    check_against_oracle(topo, st, mu, Pd, logdet, out)
    # the value call takes the one-launch quadratic form: another order of summation (as tests/test_gpu_sparse.py:42)
    assert np.allclose(out[0], tl.loglik(st)[0], rtol=1e-13, atol=0)
    # a chain's outputs are the same bits in the batch, alone, through device tensors, and with one or two chains per workgroup
    for b in range(B):
        assert same_bits([np.asarray(a)[b:b + 1] for a in out], tl.grad(st.slice(b, b + 1))), b
    dev = tl.grad(st.to(gpu))
    torch.cuda.synchronize()
    assert same_bits(out, [a.cpu().numpy() for a in dev])
    for chains in (1, 2):
        knobs.setenv("MCD_SPARSE_GRAD_CHAINS", chains)
        assert same_bits(out, tl.grad(st)), chains
        assert same_bits([np.asarray(a)[4:5] for a in out], tl.grad(st.slice(4, 5))), chains
    knobs.delenv("MCD_SPARSE_GRAD_CHAINS")
    # NaN in one chain stays in that chain -- in both geometries (chain 3 shares its workgroup with chain 2 in the two-chain one)
    Rn = st.rates.copy()
    Rn[3, topo.n_nodes // 2] = np.nan
    stn = M.StateBatch(st.heights, Rn, st.time_height, st.rate_mean)
    for chains in (1, 2):
        knobs.setenv("MCD_SPARSE_GRAD_CHAINS", chains)
        bad = [np.asarray(a) for a in tl.grad(stn)]
        for a, good in zip(bad, out):
            assert np.all(np.isnan(a[3])), chains
            assert np.array_equal(np.delete(a, 3, axis=0), np.delete(np.asarray(good), 3, axis=0)), chains


def test_sparse_tree_gradient_matrices_off_the_easy_path(gpu, knobs):
    """65 nodes (63 distances): a row of 40 entries (beyond the 16-wide record), an empty row, a non-symmetric matrix (the gradient is
    that of (P + P^T) / 2) and duplicate positions in the association list."""
    topo = S.random_topology(33, seed=11)
    n = topo.n_nodes - 2
    st = S.random_states(topo, 5, seed=4)
    rng = np.random.default_rng(8)
    mu = rng.uniform(0.01, 0.2, n)
    base = S.banded_precision(n, seed=2)[0].toarray()

    def run(P_value, assoc, P_grad=None, logdet=3.25):
        tl = M.SparseLikelihood(M.Sparse(mu, assoc, logdet)).bind_tree(topo)
        outs = []
        for chains in (1, 2):
            knobs.setenv("MCD_SPARSE_GRAD_CHAINS", chains)
            outs.append(tl.grad(st))
            check_against_oracle(topo, st, mu, P_value, logdet, outs[-1], P_grad)
            assert np.allclose(outs[-1][0], tl.loglik(st)[0], rtol=1e-13, atol=0)
        assert same_bits(outs[0], outs[1])

    # row 20 (and column 20) with 40 entries, kept diagonally dominant
    Pl = base.copy()
    Pl[20, :] = 0.0
    Pl[:, 20] = 0.0
    cols = np.setdiff1d(np.arange(n), [20])[::(n - 1) // 39][:39]
    v = rng.uniform(-300.0, 300.0, len(cols))
    Pl[20, cols] = v
    Pl[cols, 20] = v
    Pl[np.diag_indices(n)] = np.abs(Pl - np.diag(np.diag(Pl))).sum(axis=1) + 700.0
    assert np.count_nonzero(Pl[20]) == 40 and np.array_equal(Pl, Pl.T)
    run(Pl, assoc_of(Pl))
    # an empty row (and column): distance 31 does not enter
    Pe = base.copy()
    Pe[31, :] = 0.0
    Pe[:, 31] = 0.0
    run(Pe, assoc_of(Pe))
    # a non-symmetric matrix: the value uses P as given, the gradient its symmetric part
    Pn = base.copy()
    Pn[np.triu_indices(n, 1)] *= 0.5
    Pn[5, 50] += 123.0
    assert not np.array_equal(Pn, Pn.T)
    run(Pn, assoc_of(Pn), P_grad=0.5 * (Pn + Pn.T))
    # duplicate positions add up
    dup = assoc_of(base)
    half = [((i, j), 0.25 * v) for (i, j), v in dup[::3]]
    rest = [((i, j), 0.75 * v) for (i, j), v in dup[::3]]
    lst = half + [e for k, e in enumerate(dup) if k % 3 != 0] + rest
    Pdup = np.zeros((n, n))
    for (i, j), v in lst:
        Pdup[i, j] += v
    run(Pdup, lst)


def test_prior_gradient_beyond_64_kib_of_lds(gpu):
    """2047 nodes (7 n_nodes + 2 doubles = 112 KiB of LDS; the launcher used to refuse above 64 KiB, 1169 nodes), B = 3: the value is the
    value kernel's to 1e-11 (tests/test_gpu_prior.py: close), same bits alone and in the batch, central differences of the value kernel
    (step and tolerance of test_prior_gradient_large_tree_same_bits_whatever_the_batch); 2049 nodes are refused."""
    topo = S.random_topology(1024, seed=9)
    nn = topo.n_nodes
    assert nn == 2047
    B = 3
    st = S.random_states(topo, B, seed=9)
    rng = np.random.default_rng(9)
    birth, death, rvar = np.exp(0.3 * rng.standard_normal(B)), np.exp(0.3 * rng.standard_normal(B)), 0.2 + rng.random(B)
    cal = [M.Calibration("root", 0, 0.9, 0.025, 1.1, 0.025), M.Calibration("n", 5, 0.2, 0.025, None, 0.0)]
    con = [M.Constraint("k", 7, 3, 0.025)]
    full = M.StateBatch(st.heights, st.rates, st.time_height, st.rate_mean, birth, death, rvar)
    inner = np.flatnonzero(~topo.leaves)
    for model in ("UncorrelatedGamma", "AutocorrelatedLogNormal"):
        pf = M.PriorFunction(1.0, model, cal, con, [], topo)
        lp, g = pf.grad(full)
        ref = pf.logprior(full)
        assert np.all(np.isfinite(lp)) and np.all(np.abs(lp - ref) <= 1e-11 * np.maximum(1.0, np.abs(ref)))
        for b in range(B):
            lp_s, g_s = pf.grad(full.slice(b, b + 1))
            assert np.array_equal(lp_s, lp[b:b + 1])
            for k in g_s:
                assert np.array_equal(np.asarray(g_s[k]), np.asarray(g[k])[b:b + 1]), (model, b, k)
        b, eps = 1, 1e-6
        fields = dict(heights=st.heights, rates=st.rates, time_height=st.time_height, rate_mean=st.rate_mean, time_birth_rate=birth,
                      time_death_rate=death, rate_variance=rvar)

        def value(name, v, delta):
            a = {k: np.array(x[b:b + 1], dtype=float) for k, x in fields.items()}
            if v is None:
                a[name][0] += delta
            else:
                a[name][0, v] += delta
            return pf.logprior(M.StateBatch(a["heights"], a["rates"], a["time_height"], a["rate_mean"], a["time_birth_rate"],
                                            a["time_death_rate"], a["rate_variance"]))[0]

        # heights whose neighbours are far enough for the step: the root and the first inner nodes with a gap of 1e-2 on either side
        Hb, ch = st.heights[b], [np.flatnonzero(topo.parent == v) for v in range(nn)]
        roomy = [int(v) for v in inner if v > 0 and Hb[topo.parent[v]] - Hb[v] > 1e-2 and Hb[v] - Hb[ch[v]].max() > 1e-2]
        assert len(roomy) >= 4
        coords = [("heights", v) for v in [0] + roomy[:3] + roomy[-1:]]
        coords += [("rates", v) for v in (1, 17, 1300, nn - 1)]
        coords += [(k, None) for k in ("time_birth_rate", "time_death_rate", "time_height", "rate_mean", "rate_variance")]
        for name, v in coords:
            fd = (value(name, v, eps) - value(name, v, -eps)) / (2 * eps)
            gv = np.asarray(g[name])[b] if v is None else np.asarray(g[name])[b, v]
            assert abs(fd - gv) <= 1e-4 * max(1.0, abs(gv)), (model, name, v, fd, gv)
    big = S.random_topology(1025, seed=9)
    assert big.n_nodes == 2049
    stb = S.random_states(big, 1, seed=9)
    pfb = M.PriorFunction(1.0, "UncorrelatedGamma", [], [], [], big)
    with pytest.raises(M.McdError) as ei:
        pfb.grad(M.StateBatch(stb.heights, stb.rates, stb.time_height, stb.rate_mean, np.ones(1), np.ones(1), np.ones(1)))
    assert ei.value.code == _capi.MCD_ERR_UNSUPPORTED and "2049" in str(ei.value)
    # ... and the handles that work go on working
    pf = M.PriorFunction(1.0, "UncorrelatedGamma", cal, con, [], topo)
    assert np.all(np.isfinite(pf.grad(full)[0]))


def thinned_fixture(fx):
    Pt = thinned(fx["sigma_inv"])
    lhd = M.Sparse(fx["mu"], assoc_of(Pt), float(fx["logdet"]))
    assert len(lhd.sigma_inv_assoc) < Pt.size
    return Pt, lhd


def test_leapfrog_over_the_sparse_handle(gpu, golden):
    fx = golden["12-leaves-variable-rate"]
    topo = M.Topology(fx["parent"])
    cal, con, br = TN.tables(fx)
    ht = float(fx["prior_ht"])
    pf = M.PriorFunction(ht, "UncorrelatedGamma", cal, con, br, topo)
    Pt, lhd = thinned_fixture(fx)
    slik = M.SparseLikelihood(lhd).bind_tree(topo)
    dlik = M.MvnLikelihood(M.Full(fx["mu"], Pt, float(fx["logdet"]))).bind_tree(topo)
    B = 8
    ps, _ = M.proposals(topo, br, calibrations_available=True)
    smp = M.Sampler(slik, pf, ps, B, seed=2)
    x0 = M.init_with(topo, fx["mean_lengths"])
    x0.time_height = ht
    smp.set_initial_state(x0)
    for period in (50, 50, 100, 100):
        smp.run(period)
        smp.autotune()
    s = smp.state()
    lf = M.Leapfrog(slik, pf, True, B)
    lf.set_state(s)
    q0, v0, g0 = lf.position()
    mask = M.get_mask(True, topo)
    val, grad = M.target_grad(mask, slik, pf, s)
    assert lf.dim == mask.sum()
    assert np.allclose(v0, val, rtol=1e-13) and np.allclose(g0, grad, rtol=1e-11, atol=1e-9)      # tests/test_gpu_prior.py:283
    # against the dense driver over the same matrix densified
    ld = M.Leapfrog(dlik, pf, True, B)
    ld.set_state(s)
    qd, vd, gd = ld.position()
    assert np.array_equal(qd, q0)
    assert np.max(np.abs(vd - v0) / np.maximum(1.0, np.abs(vd))) <= 1e-10                          # tests/test_gpu_sparse.py:40
    assert np.max(np.abs(gd - g0)) <= 1e-8 * np.max(np.abs(gd))                                    # tests/test_gpu_nuts.py:167
    # reversibility
    rng = np.random.default_rng(3)
    inv_mass = np.full(lf.dim, 1.0)
    scale = 1.0 / np.maximum(1.0, np.abs(g0).max(axis=1))
    p0 = rng.normal(size=(B, lf.dim))
    eps = 2e-2 * scale
    p1 = lf.leapfrog(p0, eps, inv_mass, 12)
    q1, v1, _ = lf.position()
    assert np.all(np.isfinite(v1)) and np.all(np.abs(q1 - q0).max(axis=1) > 1e-6)
    p2 = lf.leapfrog(-p1, eps, inv_mass, 12)
    q2, v2, _ = lf.position()
    assert np.allclose(q2, q0, rtol=1e-10, atol=1e-12) and np.allclose(-p2, p0, rtol=1e-8, atol=1e-10) and np.allclose(v2, v0, rtol=1e-11)   # :298
    # the same trajectory on the dense driver ends at the same place to rounding
    pd1 = ld.leapfrog(p0, eps, inv_mass, 12)
    assert np.allclose(pd1, p1, rtol=1e-7, atol=1e-9) and np.allclose(ld.position()[0], q1, rtol=1e-8, atol=1e-10)


def test_leapfrog_position_on_a_large_tree(gpu):
    """2013 nodes, B = 4: beyond the dense kernels and beyond the prior gradient's old limit."""
    topo, slik, pf, st = large_problem(4)
    lf = M.Leapfrog(slik, pf, False, 4)
    lf.set_state(st)
    q0, v0, g0 = lf.position()
    mask = M.get_mask(False, topo)
    val, grad = M.target_grad(mask, slik, pf, st)
    assert np.all(np.isfinite(v0)) and np.all(np.isfinite(g0))
    assert np.allclose(v0, val, rtol=1e-13) and np.allclose(g0, grad, rtol=1e-11, atol=1e-9)


_large = {}


def large_problem(B):
    """1007 leaves (2013 nodes), a banded precision matrix around the states' own distances, valid states."""
    if "p" not in _large:
        topo = S.random_topology(1007, seed=5)
        n = topo.n_nodes - 2
        _, assoc = S.banded_precision(n, seed=5)
        st0 = S.random_states(topo, 1, seed=7)
        mu = O.distances(topo.parent, st0.heights[0], st0.rates[0], st0.time_height[0], st0.rate_mean[0])
        slik = M.SparseLikelihood(M.Sparse(mu, assoc, 0.0)).bind_tree(topo)
        pf = M.PriorFunction(1.0, "UncorrelatedGamma", [], [], [], topo)
        _large["p"] = (topo, slik, pf)
    topo, slik, pf = _large["p"]
    st = S.random_states(topo, B, seed=7, jitter=0.002)
    rng = np.random.default_rng(12)
    full = M.StateBatch(st.heights, st.rates, st.time_height, st.rate_mean, np.exp(0.1 * rng.standard_normal(B)), np.exp(0.1 * rng.standard_normal(B)),
                        0.5 + 0.2 * rng.random(B))
    return topo, slik, pf, full


def test_device_nuts_over_the_sparse_handle_follows_the_cpu_twin(gpu, golden):
    """The checks of test_gpu_nuts.test_device_nuts_follows_the_cpu_twin, the twin on the thinned matrix."""
    fx = dict(golden["12-leaves-variable-rate"])
    Pt, lhd = thinned_fixture(fx)
    fx["sigma_inv"] = Pt
    topo = M.Topology(fx["parent"])
    cal, con, br = TN.tables(fx)
    ht = float(fx["prior_ht"])
    pf = M.PriorFunction(ht, "UncorrelatedGamma", cal, con, br, topo)
    lik = M.SparseLikelihood(lhd).bind_tree(topo)
    spec = O.PriorSpec(fx["parent"], ht, "UncorrelatedGamma", [(c.node, c.lower, c.lower_p, c.upper, c.upper_p) for c in cal],
                       [(k.young, k.old, k.p) for k in con], [(b.nodes, b.sd) for b in br])
    B = 6
    ps, _ = M.proposals(topo, br, calibrations_available=True)
    smp = M.Sampler(lik, pf, ps, B, seed=3)
    x0 = M.init_with(topo, fx["mean_lengths"])
    x0.time_height = ht
    smp.set_initial_state(x0)
    smp.burn_in(fast=[10, 10, 20, 40], slow=[100, 100])
    lf = M.Leapfrog(lik, pf, True, B)
    lf.set_state(smp.state())
    mask = M.get_mask(True, topo)
    q0, lp0, g0 = lf.position()
    inv_mass = np.maximum((0.1 * np.abs(q0)).mean(axis=0) ** 2, 1e-12)
    eps = np.array([0.05, 0.1, 0.2, 0.3, 0.15, 0.25])
    st = lf.state()
    seed, max_depth = 20261004, 5
    for transition in range(3):
        q_before, lp_before, g_before = lf.position()
        alpha, depth = lf.nuts(eps, inv_mass, max_depth=max_depth, seed=seed, transition=transition)
        q_after, lp_after, g_after = lf.position()
        for b in range(B):
            x_t = M.State(st.time_birth_rate[b], st.time_death_rate[b], st.time_height[b], st.heights[b], st.rate_mean[b], st.rate_variance[b],
                          st.rates[b])
            tw = TN.Twin(fx, spec, mask, x_t)
            assert abs(tw.value(q_before[b]) - lp_before[b]) <= 1e-9 * max(1.0, abs(lp_before[b]))
            qn, lpn, a, d, n = TN.twin_transition(tw, q_before[b], g_before[b], lp_before[b], eps[b], inv_mass, max_depth, seed, b, transition)
            assert d == depth[b], (transition, b, d, depth[b])
            assert abs(a - alpha[b]) <= 1e-6, (transition, b, a, alpha[b])
            assert np.max(np.abs(qn - q_after[b]) / np.maximum(1e-3, np.abs(qn))) <= 1e-6, (transition, b)
            assert abs(lpn - lp_after[b]) <= 1e-6 * max(1.0, abs(lpn))
        val, grad = M.target_grad(mask, lik, pf, lf.state())
        assert np.max(np.abs(val - lp_after) / np.maximum(1.0, np.abs(val))) <= 1e-10
        assert np.max(np.abs(grad - g_after)) <= 1e-8 * np.max(np.abs(grad))
    assert depth.max() <= max_depth and depth.min() >= 1


def test_sparse_nuts_chains_agree_with_sparse_metropolis_hastings_chains(gpu, golden):
    """test_gpu_nuts.test_device_nuts_chains_agree_with_metropolis_hastings_chains at 12 leaves x 64 chains, both samplers over the same
    SparseTreeLikelihood (the thinned target): inner node-age means within 3 %, mean acceptance statistic in (0.45, 0.9)."""
    from mcmc_date_amd import monitor as MO

    fx = golden["12-leaves-variable-rate"]
    B = 64
    topo = M.Topology(fx["parent"])
    cal, con, br = TN.tables(fx)
    ht = float(fx["prior_ht"])
    pf = M.PriorFunction(ht, "UncorrelatedGamma", cal, con, br, topo)
    lik = M.SparseLikelihood(thinned_fixture(fx)[1]).bind_tree(topo)
    ps, _ = M.proposals(topo, br, calibrations_available=True, exact_jacobians=True)
    ps = [dataclasses.replace(p, jac_root=1) for p in ps]
    smp = M.Sampler(lik, pf, ps, B, seed=78)
    x0 = M.init_with(topo, fx["mean_lengths"])
    x0.time_height = ht
    smp.set_initial_state(x0)
    smp.burn_in(fast=[10, 10, 20, 40, 80], slow=[100, 200, 300, 400])
    tr = MO.collect(smp, 3000, period=50, accumulate=True)
    ages_mh = smp.node_age_summary()[0]
    mask = M.get_mask(True, topo)
    qs = np.array([M.to_vector(mask, M.State(tr.time_birth_rate[k, b], tr.time_death_rate[k, b], tr.time_height[k, b], tr.heights[k, b],
                                             tr.rate_mean[k, b], tr.rate_variance[k, b], tr.rates[k, b]))
                   for k in range(tr.heights.shape[0]) for b in range(0, B, 2)])
    inv_mass = qs.var(axis=0)
    lf = M.Leapfrog(lik, pf, True, B)
    lf.set_state(smp.state())
    eps, _, _, _ = lf.nuts_run(150, 0.03, inv_mass, adapt=True, delta=0.65, max_depth=6, seed=5)
    assert np.all((eps > 0.005) & (eps < 0.6)), eps
    n_tr = 300
    ages = np.zeros(topo.n_nodes)
    alphas = []
    for t in range(n_tr):
        a, d = lf.nuts(eps, inv_mass, max_depth=6, seed=5, transition=1000 + t)
        alphas.append(a.mean())
        s = lf.state()
        ages += (s.time_height[:, None] * s.heights).mean(axis=0)
    ages /= n_tr
    inner = ~topo.leaves
    rel = np.abs(ages[inner] - ages_mh[inner]) / ages_mh[inner]
    assert 0.45 < np.mean(alphas) < 0.9, np.mean(alphas)
    assert rel.max() <= 0.03, (rel, np.mean(alphas))


def test_sparse_nuts_on_a_large_tree(gpu):
    """2013 nodes, 8 chains, three transitions at max_depth 3: finite, 1 <= depth <= 3, the handle consistent with target_grad
    (tests/test_gpu_nuts.py:165-167), chain 5 alone with chain_offset = 5 ends at the same bits."""
    B = 8
    topo, slik, pf, st = large_problem(B)
    mask = M.get_mask(False, topo)
    lf = M.Leapfrog(slik, pf, False, B)
    lf.set_state(st)
    one = M.Leapfrog(slik, pf, False, 1)
    one.set_state(st.slice(5, 6))
    q0, _, g0 = lf.position()
    # masses from the positions' own scales (deep nodes have heights of 1e-10 and gaps to match: a unit mass would step out of the support
    # at once and every transition would be a rejection), step sizes from the gradient in those scales
    inv_mass = np.maximum((0.1 * np.abs(q0)).mean(axis=0) ** 2, 1e-60)
    eps = 1e-2 / np.maximum(1.0, (np.abs(g0) * np.sqrt(inv_mass)).max(axis=1))
    for transition in range(3):
        alpha, depth = lf.nuts(eps, inv_mass, max_depth=3, seed=77, transition=transition)
        a1, d1 = one.nuts(eps[5:6], inv_mass, max_depth=3, seed=77, transition=transition, chain_offset=5)
        q, v, g = lf.position()
        assert np.all(np.isfinite(alpha)) and np.all(np.isfinite(q)) and np.all(np.isfinite(v)) and np.all(np.isfinite(g))
        assert depth.min() >= 1 and depth.max() <= 3
        print(f"transition {transition}: depth {depth.tolist()} alpha {np.round(alpha, 3).tolist()}")
        val, grad = M.target_grad(mask, slik, pf, lf.state())
        assert np.max(np.abs(val - v) / np.maximum(1.0, np.abs(val))) <= 1e-10
        assert np.max(np.abs(grad - g)) <= 1e-8 * np.max(np.abs(grad))
        q1, v1, g1 = one.position()
        assert d1[0] == depth[5] and a1[0] == alpha[5]
        assert np.array_equal(q1[0], q[5]) and v1[0] == v[5] and np.array_equal(g1[0], g[5])
    assert np.all(np.any(q != q0, axis=1))                  # every chain has moved


def test_refusals(gpu):
    import ctypes as C

    L = _capi.lib()
    big = S.random_topology(1025, seed=9)
    n = big.n_nodes - 2
    assert big.n_nodes == 2049
    mu = np.full(n, 0.1)
    tl_big = M.SparseLikelihood(M.Sparse(mu, [((i, i), 100.0) for i in range(n)], 0.0)).bind_tree(big)
    st_big = S.random_states(big, 2, seed=1)
    with pytest.raises(M.McdError) as ei:
        tl_big.grad(st_big)
    assert ei.value.code == _capi.MCD_ERR_UNSUPPORTED and "2049" in str(ei.value)
    pf_big = M.PriorFunction(1.0, "UncorrelatedGamma", [], [], [], big)
    with pytest.raises(M.McdError) as ei:
        M.Leapfrog(tl_big, pf_big, False, 2)
    assert ei.value.code == _capi.MCD_ERR_UNSUPPORTED and "2049" in str(ei.value)
    assert np.all(np.isfinite(tl_big.loglik(st_big)[0]))             # the value still works at that size
    # a prior with another node count; NULL handles
    topo = S.random_topology(33, seed=11)
    n = topo.n_nodes - 2
    P, assoc = S.banded_precision(n, seed=33)
    tl = M.SparseLikelihood(M.Sparse(np.full(n, 0.1), assoc, 1.0)).bind_tree(topo)
    pf = M.PriorFunction(1.0, "UncorrelatedGamma", [], [], [], topo)
    other = M.PriorFunction(1.0, "UncorrelatedGamma", [], [], [], S.random_topology(34, seed=11))
    lf = M.Leapfrog(tl, pf, False, 3)
    st = S.random_states(topo, 3, seed=2)
    full = M.StateBatch(st.heights, st.rates, st.time_height, st.rate_mean, np.ones(3), np.ones(3), np.full(3, 0.5))
    lf.set_state(full)
    before = lf.position()
    with pytest.raises(M.McdError) as ei:
        M.Leapfrog(tl, other, False, 3)
    assert ei.value.code == _capi.MCD_ERR_INVALID_ARG
    h = C.c_void_p()
    assert L.mcd_hmc_create_sparse(C.byref(h), None, pf._p, 0, 3) == _capi.MCD_ERR_INVALID_ARG and not h.value
    assert L.mcd_hmc_create_sparse(C.byref(h), tl._t, None, 0, 3) == _capi.MCD_ERR_INVALID_ARG and not h.value
    assert L.mcd_hmc_create_sparse(None, tl._t, pf._p, 0, 3) == _capi.MCD_ERR_INVALID_ARG
    assert L.mcd_hmc_create_sparse(C.byref(h), tl._t, pf._p, 0, 0) == _capi.MCD_ERR_INVALID_ARG and not h.value
    x = np.zeros(8)
    p = x.ctypes.data_as(C.c_void_p)
    assert L.mcd_sparse_tree_grad_batch(None, p, p, 8, p, p, 1, 0, None, p, p, p, p, p) == _capi.MCD_ERR_INVALID_ARG
    assert L.mcd_sparse_tree_grad_batch(tl._t, None, p, topo.n_nodes, p, p, 1, 0, None, p, p, p, p, p) == _capi.MCD_ERR_INVALID_ARG
    assert L.mcd_sparse_tree_grad_batch(tl._t, p, p, 8, p, p, 1, 0, None, p, p, p, p, p) == _capi.MCD_ERR_INVALID_ARG     # ld_state < n_nodes
    # after the refusals the existing handles still work, to the bit
    after = lf.position()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    lf.set_state(full)
    assert all(np.array_equal(a, b) for a, b in zip(before, lf.position()))
    assert same_bits(tl.grad(st), tl.grad(st))
