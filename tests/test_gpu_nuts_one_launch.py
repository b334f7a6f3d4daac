"""The one-launch form of the NUTS driver (mcd_hmc_set_transition_form, MCD_HMC_TRANSITION_ONE_LAUNCH; csrc/k_nuts_chain.hip): a whole
transition of every chain, and the steps of mcd_hmc_leapfrog, as ONE kernel launch.  Its definition is "the same bits as the rounds form
with the substitution sweep as its likelihood gradient" (what every batch of this file takes), so every comparison builds two handles over
the same problem, one per form, sets the same state and compares with np.array_equal -- with equal_nan where a chain may leave the support,
which also requires the same NaN positions.

Sizes: the golden fixtures of 11, 23 and 47 nodes (the last with braces, calibrations and a constraint); a synthetic bifurcating tree of 33
leaves (65 nodes, N = 63: two 64-node slices of the prior, the last column block nearly full); a 66-node tree (N = 64, the bound), and 67
nodes for the refusal.  An even number of nodes needs a node that does not bifurcate, and the prior refuses multifurcations (birthDeathWith:
"Tree is multifurcating"), so the 66-node tree has one ONE-CHILD node instead: the same N = 64, the same 66 nodes."""
import functools
import os

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("time_birth_rate", "time_death_rate", "time_height", "rate_mean", "rate_variance", "heights", "rates")
SIZES = {"11-nodes": ("06-leaves-constant-rate", 3), "23-nodes": ("12-leaves-variable-rate", 5), "47-nodes": ("24-leaves-braces", 8),
         "65-nodes": (33, 4), "66-nodes": ("33+1", 2)}


class Problem:
    """Likelihood, prior and `chains` distinct start states of one size; what the handles of every test are built over."""

    def __init__(self, what, chains, model="UncorrelatedGamma", sparse=False):
        from mcmc_date_amd import synthetic as S

        self.chains = chains
        if isinstance(what, str) and not what.endswith("+1"):
            fx = dict(np.load(os.path.join(GOLDEN, what + ".npz")))
            topo = M.Topology(fx["parent"])
            cal = [M.Calibration(f"c{i}", int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for i, r in enumerate(fx["cal"])]
            con = [M.Constraint(f"k{i}", int(r[0]), int(r[1]), r[2]) for i, r in enumerate(fx["con"])]
            br = [M.Brace(f"b{i}", [int(n) for n in fx["brace_nodes"][fx["brace_ptr"][i]:fx["brace_ptr"][i + 1]]], float(s))
                  for i, s in enumerate(fx["brace_sd"])]
            ht = float(fx["prior_ht"])
            if sparse:
                P = np.asarray(fx["sigma_inv"])
                assoc = [((int(i), int(j)), float(P[i, j])) for i in range(P.shape[0]) for j in range(P.shape[1])]
                self.lik = M.SparseLikelihood(M.Sparse(fx["mu"], assoc, float(fx["logdet"]))).bind_tree(topo)
            else:
                self.lik = M.MvnLikelihood(M.Full(fx["mu"], fx["sigma_inv"], float(fx["logdet"]))).bind_tree(topo)
            self.pf = M.PriorFunction(ht, model, cal, con, br, topo)
            self.cal = len(cal) > 0
            self.ps, _ = M.proposals(topo, br, calibrations_available=self.cal)
            x0 = M.init_with(topo, fx["mean_lengths"])
            if self.cal:
                x0.time_height = ht
            smp = M.Sampler(self.lik, self.pf, self.ps, chains, seed=77)             # a short burn-in: the chains differ afterwards
            smp.set_initial_state(x0)
            for _ in range(2):
                smp.run(6)
                smp.autotune()
            self.s0 = smp.state()
        else:
            topo = S.random_topology(33 if what == "33+1" else what, seed=31)
            if what == "33+1":                                                          # a leaf (not the root's child) gets one child
                par = [int(p) for p in topo.parent]
                v = max(u for u in range(1, len(par)) if u not in par and par[u] != 0)
                topo = M.Topology(np.asarray([p + 1 if p > v else p for p in par[:v + 1]] + [v] + [p + 1 if p > v else p for p in par[v + 1:]], np.int32))
            n = topo.n_nodes - 2
            mu, sigma = S.random_spd_problem(n, seed=n)
            self.lik = M.MvnLikelihood.from_covariance(mu, sigma).bind_tree(topo)
            inner = [v for v in range(1, topo.n_nodes) if (np.asarray(topo.parent) == v).any()]
            cal = [M.Calibration("root", 0, 0.9, 0.025, 1.3, 0.025), M.Calibration("c", int(inner[len(inner) // 2]), 1e-3, 0.025, 5.0, 0.025)]
            self.pf = M.PriorFunction(1.0, "UncorrelatedLogNormal", cal, [], [], topo)
            self.cal = True
            s0 = S.random_states(topo, chains, seed=5)
            s0.time_birth_rate = np.linspace(1.0, 1.2, chains)
            s0.time_death_rate = np.linspace(0.8, 0.7, chains)
            s0.rate_variance = np.linspace(0.3, 0.4, chains)
            self.s0 = s0
        self.topo = topo

    def handle(self, form, rows=None):
        lo, hi = rows or (0, self.chains)
        lf = M.Leapfrog(self.lik, self.pf, self.cal, hi - lo)
        if form != "rounds":
            lf.set_transition_form(form)
        lf.set_state(M.StateBatch(**{f: np.ascontiguousarray(getattr(self.s0, f)[lo:hi]) for f in FIELDS}))
        return lf

    def pair(self, rows=None):
        return self.handle("rounds", rows), self.handle("one_launch", rows)

    def inputs(self, lf):
        """(eps [B], inv_mass [dim]): masses from the positions' own scales, step sizes from the gradient in those scales, spread over
        the chains so that their trees differ."""
        q, _, g = lf.position()
        inv_mass = np.maximum((0.1 * np.abs(q)).mean(axis=0) ** 2, 1e-12)
        eps = 0.05 / np.maximum(1.0, (np.abs(g) * np.sqrt(inv_mass)).max(axis=1)) * np.geomspace(0.5, 6.0, lf.batch)
        return eps, inv_mass

    def dense_metric(self, inv_mass):
        """A full inverse mass matrix around the diagonal one: S (I + 0.3 A A^T / 3) S, exactly symmetric."""
        dim = inv_mass.size
        A = np.random.default_rng(dim).standard_normal((dim, 3))
        s = np.sqrt(inv_mass)
        C = s[:, None] * (np.eye(dim) + 0.1 * A @ A.T) * s[None, :]
        return 0.5 * (C + C.T)


@functools.lru_cache(maxsize=None)
def problem(size, model="UncorrelatedGamma"):
    what, chains = SIZES[size]
    return Problem(what, chains, model)


def same_handles(a, b, what=""):
    """state, position, ln target and gradient of two handles: the same bits, the same NaNs"""
    for x, y, name in zip(a.position(), b.position(), ("q", "value", "grad")):
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {name}"
    sa, sb = a.state(), b.state()
    for f in FIELDS:
        assert np.array_equal(getattr(sa, f), getattr(sb, f), equal_nan=True), f"{what}: {f}"


def refused(call, code, *words):
    with pytest.raises(_capi.McdError) as ei:
        call()
    assert ei.value.code == code, ei.value
    for w in words:
        assert w in str(ei.value), (w, str(ei.value))


# ---- 1. form and refusals ------------------------------------------------------------------------------------------------------------
def test_form_round_trip_refusals_and_persistence(gpu):
    pr = problem("23-nodes")
    lf = pr.handle("rounds")
    assert lf.transition_form == "rounds"
    lf.set_transition_form("one_launch")
    assert lf.transition_form == "one_launch"
    lf.set_transition_form("rounds")
    assert lf.transition_form == "rounds"
    lf.set_transition_form("one_launch")
    # any other value
    refused(lambda: _capi.check(_capi.lib().mcd_hmc_set_transition_form(lf._h, 2)), _capi.MCD_ERR_INVALID_ARG, "form = 2")
    with pytest.raises(ValueError):
        lf.set_transition_form("both")
    assert lf.transition_form == "one_launch"
    # the across-chains form of a dense metric, in both orders
    refused(lambda: lf.set_metric_form("across_chains"), _capi.MCD_ERR_UNSUPPORTED, "MCD_HMC_METRIC_ACROSS_CHAINS", "MCD_HMC_TRANSITION_ONE_LAUNCH")
    assert lf.metric_form == "per_chain" and lf.transition_form == "one_launch"
    acr = pr.handle("rounds")
    acr.set_metric_form("across_chains")
    refused(lambda: acr.set_transition_form("one_launch"), _capi.MCD_ERR_UNSUPPORTED, "MCD_HMC_METRIC_ACROSS_CHAINS")
    assert acr.transition_form == "rounds" and acr.metric_form == "across_chains"
    # the form survives set_state and set_metric(None); the refused handle's next transition is a rounds handle's
    eps, inv_mass = pr.inputs(lf)
    lf.set_metric(pr.dense_metric(inv_mass))
    lf.clear_metric()
    lf.set_state(pr.s0)
    assert lf.transition_form == "one_launch"
    ref = pr.handle("rounds")
    out = [h.nuts(eps, inv_mass, max_depth=4, seed=9, transition=3) for h in (ref, lf, acr)]
    for o in out[1:]:
        assert np.array_equal(out[0][0], o[0]) and np.array_equal(out[0][1], o[1])
    same_handles(ref, lf, "one launch")
    same_handles(ref, acr, "refused")


def test_a_tree_of_67_nodes_and_a_sparse_handle_are_refused(gpu):
    big = Problem(34, 2)
    sp = Problem("12-leaves-variable-rate", 2, sparse=True)
    for pr, words in ((big, ("65 distances", "67 nodes", "64 distances", "66 nodes")), (sp, ("sparse", "21 distances", "64 distances"))):
        lf, ref = pr.handle("rounds"), pr.handle("rounds")
        refused(lambda: lf.set_transition_form("one_launch"), _capi.MCD_ERR_UNSUPPORTED, *words)
        assert lf.transition_form == "rounds"
        eps, inv_mass = pr.inputs(ref)
        a, b = lf.nuts(eps, inv_mass, max_depth=3, seed=2), ref.nuts(eps, inv_mass, max_depth=3, seed=2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        same_handles(lf, ref, "after the refusal")


# ---- 2. leapfrog ---------------------------------------------------------------------------------------------------------------------
def leapfrog_case(pr, n_steps, dense=False, blow_up=False):
    a, b = pr.pair()
    eps, inv_mass = pr.inputs(a)
    if blow_up:
        eps = eps.copy()
        eps[1] *= 1e4                                                   # this chain's first drift takes it out of the support
    if dense:
        C = pr.dense_metric(inv_mass)
        a.set_metric(C)
        b.set_metric(C)
        inv_mass = None
    rng = np.random.default_rng(n_steps + 17)
    p0 = rng.standard_normal((a.batch, a.dim)) / np.sqrt(pr.inputs(a)[1])
    direction = np.where(np.arange(a.batch) % 2 == 0, 1.0, -1.0)
    pa = a.leapfrog(p0, eps, inv_mass, n_steps, direction=direction)
    pb = b.leapfrog(p0, eps, inv_mass, n_steps, direction=direction)
    assert np.array_equal(pa, pb, equal_nan=True), "p"
    same_handles(a, b, f"{n_steps} steps")
    return a, pa


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("n_steps", [0, 1, 2, 7])
def test_leapfrog_steps(gpu, size, n_steps):
    a, p = leapfrog_case(problem(size), n_steps)
    assert np.isfinite(p).any() and np.isfinite(a.position()[1]).any()   # (a comparison of NaNs alone would show nothing)


@pytest.mark.parametrize("model", ["UncorrelatedGamma", "UncorrelatedLogNormal", "UncorrelatedWhiteNoise", "AutocorrelatedLogNormal"])
def test_leapfrog_every_clock_model(gpu, model):
    leapfrog_case(problem("23-nodes", model), 3)


def test_leapfrog_out_of_the_support(gpu):
    a, p = leapfrog_case(problem("23-nodes"), 2, blow_up=True)
    assert np.isnan(a.position()[2][1]).any() and np.isfinite(a.position()[2][0]).all()      # the NaN gradient the header describes


@pytest.mark.parametrize("size", ["23-nodes", "66-nodes"])
def test_leapfrog_dense_metric(gpu, size):
    leapfrog_case(problem(size), 3, dense=True)


# ---- 3. transitions ------------------------------------------------------------------------------------------------------------------
VARIANTS = {"depth-6": (6, 1.0, False), "depth-1": (1, 1.0, False), "eps-x20": (6, 20.0, False), "eps-by-50": (5, 1 / 50.0, False),
            "dense": (6, 1.0, True)}


@functools.lru_cache(maxsize=None)
def transitions(size, variant):
    """Six consecutive transitions on both forms, compared after each; then one ROUNDS-form leapfrog from both handles: the raw outputs of
    the gradient kernels belong to the accepted point on either.  Returns the depths met [6, B]."""
    max_depth, scale, dense = VARIANTS[variant]
    pr = problem(size)
    a, b = pr.pair()
    eps, inv_mass = pr.inputs(a)
    eps = eps * scale
    if dense:
        C = pr.dense_metric(inv_mass)
        a.set_metric(C)
        b.set_metric(C)
        inv_mass = None
    depths = []
    for t in range(6):
        ra = a.nuts(eps, inv_mass, max_depth=max_depth, seed=11, transition=t)
        rb = b.nuts(eps, inv_mass, max_depth=max_depth, seed=11, transition=t)
        assert np.array_equal(ra[0], rb[0], equal_nan=True), f"alpha of transition {t}"
        assert np.array_equal(ra[1], rb[1]), f"depth of transition {t}: {ra[1]} {rb[1]}"
        same_handles(a, b, f"transition {t}")
        depths.append(ra[1])
    b.set_transition_form("rounds")
    p0 = np.random.default_rng(3).standard_normal((a.batch, a.dim)) / np.sqrt(pr.inputs(a)[1])
    pa, pb = a.leapfrog(p0, eps, inv_mass, 1), b.leapfrog(p0, eps, inv_mass, 1)
    assert np.array_equal(pa, pb, equal_nan=True), "the leapfrog step after the transitions"
    same_handles(a, b, "after the leapfrog step")
    return np.asarray(depths)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_transitions(gpu, size, variant):
    depths = transitions(size, variant)
    max_depth = VARIANTS[variant][0]
    assert depths.min() >= 1 and depths.max() <= max_depth
    if variant in ("depth-1", "eps-by-50"):
        assert (depths == max_depth).all(), depths                      # every chain reaches the depth stop: the full counted loop


def test_chains_finish_in_different_rounds(gpu):
    assert any(len(np.unique(transitions(size, "depth-6")[t])) > 1 for size in SIZES for t in range(6)), \
        {size: transitions(size, "depth-6").tolist() for size in SIZES}


# ---- 4. batch independence -----------------------------------------------------------------------------------------------------------
def test_chains_do_not_depend_on_the_batch(gpu):
    pr = Problem("12-leaves-variable-rate", 24)
    whole, part = pr.handle("one_launch"), pr.handle("one_launch", rows=(8, 16))
    eps, inv_mass = pr.inputs(whole)
    for t in range(3):
        rw = whole.nuts(eps, inv_mass, max_depth=5, seed=21, transition=t)
        rp = part.nuts(eps[8:16], inv_mass, max_depth=5, seed=21, transition=t, chain_offset=8)
        assert np.array_equal(rw[0][8:16], rp[0]) and np.array_equal(rw[1][8:16], rp[1])
    for x, y in zip(whole.position(), part.position()):
        assert np.array_equal(x[8:16], y, equal_nan=True)
    sw, sp = whole.state(), part.state()
    for f in FIELDS:
        assert np.array_equal(getattr(sw, f)[8:16], getattr(sp, f), equal_nan=True), f


# ---- 5. tuning -----------------------------------------------------------------------------------------------------------------------
def test_tuning(gpu):
    pr = problem("47-nodes")
    a, b = pr.pair()
    eps, inv_mass = pr.inputs(a)
    for x, y in zip(a.nuts_run(8, eps, inv_mass, adapt=True, max_depth=5, seed=4), b.nuts_run(8, eps, inv_mass, adapt=True, max_depth=5, seed=4)):
        assert np.array_equal(x, y)                                     # eps, mean_alpha, q_mean, q_var
    same_handles(a, b, "nuts_run")
    for x, y in zip(a.nuts_warmup(eps, inv_mass, windows=2, window=6, max_depth=5, seed=5, first_transition=8),
                    b.nuts_warmup(eps, inv_mass, windows=2, window=6, max_depth=5, seed=5, first_transition=8)):
        assert np.array_equal(x, y)                                     # eps, masses, mean_alpha
    same_handles(a, b, "nuts_warmup")


def test_dense_warmup(gpu):
    pr = Problem("12-leaves-variable-rate", 16)
    a, b = pr.pair()
    eps, inv_mass = pr.inputs(a)
    for x, y in zip(a.nuts_warmup_dense(eps, inv_mass, windows=2, window=6, max_depth=5, seed=6),
                    b.nuts_warmup_dense(eps, inv_mass, windows=2, window=6, max_depth=5, seed=6)):
        assert np.array_equal(x, y)                                     # eps, the metric, mean_alpha
    assert a.metric() is not None and np.array_equal(a.metric(), b.metric())
    assert b.transition_form == "one_launch"
    same_handles(a, b, "nuts_warmup_dense")


# ---- 6. recorder ---------------------------------------------------------------------------------------------------------------------
def test_recorder(gpu):
    pr = problem("23-nodes")
    a, b = pr.pair()
    plain = pr.handle("one_launch")
    eps, inv_mass = pr.inputs(a)
    for h in (a, b):
        h.record_begin(period=2, capacity=8)
        h.nuts_run(6, eps, inv_mass, max_depth=5, seed=8)
    plain.nuts_run(6, eps, inv_mass, max_depth=5, seed=8)
    sa, sb = a.record_summary(max_lag=0, per_chain=True), b.record_summary(max_lag=0, per_chain=True)
    assert sa.n_samples == sb.n_samples == 3
    for f in ("pooled", "per_chain", "nuts_stats"):
        assert np.array_equal(getattr(sa, f), getattr(sb, f), equal_nan=True), f
    fa, fb = a.record_fetch(), b.record_fetch()
    assert len(fa) == len(fb) == 6 and fa[0].tolist() == [2, 4, 6]
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y, equal_nan=True)
    for h in (a, b):
        h.record_end()
    assert b.transition_form == "one_launch"                           # (the form survives recorder begin / end)
    same_handles(a, b, "recorded")
    same_handles(b, plain, "recorded against unrecorded")
    st = plain.state()
    assert np.array_equal(fb[2][-1], st.heights) and np.array_equal(fb[3][-1], st.rates)


# ---- 7. the attached cycle -----------------------------------------------------------------------------------------------------------
def test_attached_cycle(gpu):
    pr = Problem("12-leaves-variable-rate", 4)
    runs = []
    for form in ("rounds", "one_launch"):
        smp = M.Sampler(pr.lik, pr.pf, pr.ps, 4, seed=77)
        smp.set_state(pr.s0)
        lf = pr.handle(form)
        eps, inv_mass = pr.inputs(lf)
        smp.attach_hamiltonian(lf, eps, inv_mass, max_depth=5)
        smp.run(4)
        runs.append((smp.state(), smp.posterior(), smp.hamiltonian_stats(), lf.transition_form))
        smp.detach_hamiltonian()
    (s0, p0, h0, f0), (s1, p1, h1, f1) = runs
    assert (f0, f1) == ("rounds", "one_launch")
    for f in FIELDS:
        assert np.array_equal(getattr(s0, f), getattr(s1, f)), f
    assert np.array_equal(p0, p1)
    assert h0["transitions"] == h1["transitions"] == 4
    for k in ("alpha_sum", "depth_sum", "leapfrog_steps", "divergent"):
        assert np.array_equal(h0[k], h1[k]), k
