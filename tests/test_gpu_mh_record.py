"""The sample recorder of the Metropolis-Hastings driver on the device (mcd_mh_record_*): thinned samples of every chain, stored by
the kernels of every launch structure while mcd_mh_run runs.  Everything is compared with what the entry points that existed before
the recorder return (state, posterior, age sums, traces) on a twin sampler without a recorder -- never with the recorder itself.

Every case names the launch structure it is meant for and asserts that the run took it (mcd_mh_last_path), so that a change of the
planner cannot silently drop a path from this file.  Schedules are explicit ([n_iter, S] with a short S, dense proposals -- the ones
that leave a segment -- also on the steps that close an iteration), so both sides of a comparison see the same one.

Cutting a run: a call of mcd_mh_run starts its incremental likelihood from a full product and counts its periodic refresh from the call's
first step.  A PREFIX of a run therefore passes through the same bits as the long run on every path (measured without a recorder:
the prefix's ln acceptance ratios equal the head of the long run's bit for bit; test_prefix_runs_pass_through_the_same_bits asserts it),
so mid-launch samples are compared exactly with prefix runs.  A run cut into CHUNKS restarts z = L^-1 (d - mu) (or q) from a full product
at every call, so on the paths that evaluate incrementally (2, 6, 8, 9) its ln likelihoods agree with the uncut run's only to rounding:
there the decisions must be equal and the values agree within the tolerance that tests/test_gpu_mh.py uses between two launch structures
of the same chain (tol = 1e-8 + 1e-12 max |ln posterior term|, rtol 1e-12 on the ln likelihood: test_gpu_mh.py:277 / :297 and :348 /
:363); everything else (states, ln priors, ln Jacobians) and all of it on the other paths is compared exactly."""
import ctypes as C

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi, monitor
from mcmc_date_amd import sampler as SM

pytestmark = pytest.mark.gpu

FIELDS = ("time_birth_rate", "time_death_rate", "time_height", "rate_mean", "rate_variance", "heights", "rates")
SCALARS = ("time_birth_rate", "time_death_rate", "time_height", "rate_mean", "rate_variance")      # the order of scalars[..., 5]
# name -> (likelihood, leaves or fixture, chains, knobs, MCD_MH_PATH_*)
CASES = {
    "1-chain-lds": ("golden", "12-leaves-variable-rate", 16, {}, 1),
    "2-chain-streamed": ("dense", 129, 32, {}, 2),
    "8-segments": ("dense", 150, 24, {}, 8),
    "9-all-in-segments": ("sparse", 100, 17, {}, 9),
    "9-dense-leave-the-segment": ("sparse", 300, 17, {}, 9),
    "3-prior-beside": ("golden", "12-leaves-variable-rate", 16, {"MCD_MH_PER_PHASE": 1}, 3),
    "4-two-launch": ("golden", "12-leaves-variable-rate", 16, {"MCD_MH_PER_PHASE": 1, "MCD_MH_PRIOR": 0}, 4),
    "5-step-wg-x": ("dense", 200, 12, {"MCD_MH_INCREMENTAL": 0}, 5),
    "6-step-wg-incremental": ("dense", 200, 12, {"MCD_MH_SEGMENTS": 0}, 6),
    "7-step-wg-sparse": ("sparse", 300, 17, {"MCD_MH_SEGMENTS": 0}, 7),
}
INCREMENTAL_PATHS = (2, 6, 8, 9)         # a new call restarts their kept z / q from a full product (module docstring)
S_STEPS = 12                             # steps per iteration of the schedules here


class Case:
    """Tree, likelihood, prior, proposal table and initial states of one case, and samplers on them."""

    def __init__(self, name, knobs):
        from mcmc_date_amd import synthetic as S

        kind, what, self.B, self.knobs, self.path = CASES[name]
        for k, v in self.knobs.items():                      # (MCD_MH_PER_PHASE is read by mcd_mh_create: set before any sampler exists;
            knobs.setenv(k, v)                               # the knobs fixture puts every knob back when the test ends)
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
        """[n_iter, S]: proposals drawn from the whole table, one in eight from the ones that move every distance (scalings of the time
        height and the rate mean, the whole-tree proposals: what leaves a segment), and a dense one forced onto the first and onto
        the last step of some iterations -- the steps whose decision another launch takes."""
        tab = M.table_arrays(self.ps)
        dense = [i for i in range(len(self.ps)) if (tab["kind"][i] == SM.SCALE_SCALAR and tab["node"][i] in (SM.TIME_HEIGHT, SM.RATE_MEAN))
                 or tab["kind"][i] in (SM.SCALE_NORM_TREE, SM.SCALE_RATES_TREE_CONTRA, SM.SLIDE_ROOT_CONTRA, SM.SCALE_CONTRARILY)]
        assert len(dense) >= 3
        rng = np.random.default_rng(seed)
        sched = rng.integers(0, len(self.ps), size=(n_iter, S)).astype(np.int32)
        pick = rng.random((n_iter, S)) < 0.125
        sched[pick] = rng.choice(dense, size=int(pick.sum()))
        for it in range(n_iter):
            if it % 3 == 1:
                sched[it, S - 1] = dense[it % len(dense)]
            if it % 4 == 2:
                sched[it, 0] = dense[(it + 1) % len(dense)]
        return sched

    def check_path(self, smp):
        got = int(_capi.lib().mcd_mh_last_path(smp._h))
        assert got == self.path, f"meant for launch structure {self.path}, the run took {got}: {smp.last_path()}"

    def tol(self, post):
        return 1e-8 + 1e-12 * np.abs(post[..., :2]).max()            # tests/test_gpu_mh.py:277, :348


def same_state(s, sample_fields):
    for f in FIELDS:
        assert np.array_equal(getattr(s, f), sample_fields[f]), f


def sample_fields(fetched, k):
    it, sc, H, R, post, beta = fetched
    d = {name: sc[k, :, i] for i, name in enumerate(SCALARS)}
    d["heights"], d["rates"] = H[k], R[k]
    return d


def post_equal(case, got, want, exact):
    """[B, 3] ln prior, ln likelihood, ln jacobianRootBranch: bit for bit, or -- the ln likelihood of a run that was cut differently on an
    incremental path -- as tests/test_gpu_mh.py:297 / :363 compare two launch structures."""
    if exact:
        assert np.array_equal(got, want), np.max(np.abs(got - want))
    else:
        assert np.array_equal(got[:, [0, 2]], want[:, [0, 2]])
        assert np.allclose(got[:, 1], want[:, 1], rtol=1e-12, atol=case.tol(want)), np.max(np.abs(got[:, 1] - want[:, 1]))


@pytest.fixture(params=list(CASES))
def case(request, gpu, knobs):
    return Case(request.param, knobs)


def test_recorder_does_not_disturb_the_chains(case):
    sched = case.schedule(24)
    out = []
    for recorded in (True, False):
        smp = case.sampler()
        if recorded:
            smp.record_begin(2, 12)
        ta, tk = smp.run_schedule(sched, accumulate=True, trace=True)
        case.check_path(smp)
        out.append((ta, tk, smp.state(), smp.posterior(), smp.tuning(), smp.age_sums()))
        if recorded:
            assert smp.record_count() == 12
            smp.record_end()
    (a1, k1, s1, p1, t1, g1), (a2, k2, s2, p2, t2, g2) = out
    assert np.array_equal(a1, a2, equal_nan=True) and np.array_equal(k1, k2) and 0.02 < k1.mean() < 0.98
    for f in FIELDS:
        assert np.array_equal(getattr(s1, f), getattr(s2, f)), f
    assert np.array_equal(p1, p2)
    assert all(np.array_equal(x, y) for x, y in zip(t1, t2))
    assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1]) and g1[2] == g2[2] == 24


def test_end_of_call_samples_are_exact(case):
    period, n_calls = 2, 9
    sched = case.schedule(period * n_calls)
    rec, plain = case.sampler(), case.sampler()
    rec.record_begin(period, 4)
    for c in range(n_calls):
        part = sched[c * period:(c + 1) * period]
        rec.run_schedule(part)
        plain.run_schedule(part)
        assert rec.record_count() == 1
        f = rec.record_fetch()
        assert rec.record_count() == 0
        assert np.array_equal(f[0], [period * (c + 1)]) and f[0].dtype == np.int64
        same_state(plain.state(), sample_fields(f, 0))
        assert np.array_equal(f[4][0], plain.posterior())
        assert np.array_equal(f[5][0], np.ones(case.B))
    case.check_path(rec)
    rec.record_end()


def test_mid_launch_samples_add_up_to_the_age_sums(case):
    K = 30
    sched = case.schedule(K)
    smp = case.sampler()
    smp.record_begin(1, K)
    _, tk = smp.run_schedule(sched, accumulate=True, trace=True)
    case.check_path(smp)
    it, sc, H, R, post, beta = smp.record_fetch()
    age_sum, _, n = smp.age_sums()
    assert n == K and len(it) == K and np.array_equal(it, np.arange(1, K + 1))
    total = np.zeros_like(age_sum)
    for k in range(K):                                       # the device's order: one iteration after the other, fp64
        total = total + sc[k, :, 2][:, None] * H[k]
    assert np.array_equal(total, age_sum), np.max(np.abs(total - age_sum))
    same_state(smp.state(), sample_fields((it, sc, H, R, post, beta), K - 1))
    assert np.array_equal(post[K - 1], smp.posterior())
    # the samples are not all the same state: chains moved between them
    assert tk.any() and not np.array_equal(H[0], H[K - 1])
    smp.record_end()


def test_prefix_runs_pass_through_the_same_bits(case):
    """No recorder involved: the ln acceptance ratios and decisions of a run cut after k iterations are the head of the long run's."""
    sched = case.schedule(24)
    smp = case.sampler()
    ta, tk = smp.run_schedule(sched, trace=True)
    case.check_path(smp)
    for k in (3, 12):
        pre = case.sampler()
        pa, pk = pre.run_schedule(sched[:k], trace=True)
        assert np.array_equal(pk, tk[:k * S_STEPS]) and np.array_equal(pa, ta[:k * S_STEPS], equal_nan=True), k


def test_mid_launch_samples_equal_prefix_runs(case):
    period, n_iter = 3, 24
    sched = case.schedule(n_iter)
    smp = case.sampler()
    smp.record_begin(period, n_iter // period)
    smp.run_schedule(sched)
    case.check_path(smp)
    f = smp.record_fetch()
    n = n_iter // period
    assert np.array_equal(f[0], period * np.arange(1, n + 1))
    for k in (1, n // 2, n):                                 # first, middle and last sample
        pre = case.sampler()
        pre.run_schedule(sched[:k * period])
        same_state(pre.state(), sample_fields(f, k - 1))
        assert np.array_equal(f[4][k - 1], pre.posterior()), k
    smp.record_end()


def test_chunked_runs_record_the_same_samples(case):
    period = 3
    sched = case.schedule(23)
    exact = case.path not in INCREMENTAL_PATHS
    one, cut = case.sampler(), case.sampler()
    one.record_begin(period, 8)
    _, k_one = one.run_schedule(sched, trace=True)
    case.check_path(one)
    f1 = one.record_fetch()
    cut.record_begin(period, 4)
    parts, k_cut, lo = [], [], 0
    for n in (5, 7, 11):
        _, tk = cut.run_schedule(sched[lo:lo + n], trace=True)
        k_cut.append(tk)
        lo += n
        assert cut.record_count() == lo // period - (lo - n) // period
        parts.append(cut.record_fetch())
    f2 = [np.concatenate([p[i] for p in parts]) for i in range(6)]
    assert np.array_equal(f1[0], [3, 6, 9, 12, 15, 18, 21]) and np.array_equal(f2[0], f1[0])
    assert np.array_equal(np.concatenate(k_cut), k_one)
    for i in (1, 2, 3, 5):
        assert np.array_equal(f1[i], f2[i]), i
    for k in range(len(f1[0])):
        post_equal(case, f2[4][k], f1[4][k], exact)
    one.record_end()
    cut.record_end()


def test_capacity_and_misuse(case):
    L = _capi.lib()
    sched = case.schedule(8)
    smp = case.sampler()
    for call in (lambda: smp.record_fetch(), lambda: smp.record_end(), lambda: smp.record_count()):
        with pytest.raises(_capi.McdError, match="no recorder is active"):
            call()
    with pytest.raises(_capi.McdError, match="period must be >= 1"):
        smp.record_begin(0, 4)
    with pytest.raises(_capi.McdError, match="capacity must be >= 1"):
        smp.record_begin(2, 0)
    smp.record_begin(2, 3)
    with pytest.raises(_capi.McdError, match="active already"):
        smp.record_begin(2, 3)
    smp.run_schedule(sched[:5])                              # iterations 2, 4
    assert smp.record_count() == 2
    before = (smp.state(), smp.posterior(), smp.tuning(), smp.iterations_done)
    with pytest.raises(_capi.McdError, match=r"would record 2 samples.* 1 free") as e:
        smp.run_schedule(sched[5:8])                         # iterations 6, 8: one slot short
    code = e.value.code
    del e                                                    # (its traceback holds this frame: a cycle that would keep the handles alive)
    assert code == _capi.MCD_ERR_INVALID_ARG
    assert smp.record_count() == 2 and smp.iterations_done == before[3]
    for f in FIELDS:
        assert np.array_equal(getattr(smp.state(), f), getattr(before[0], f)), f
    assert np.array_equal(smp.posterior(), before[1]) and all(np.array_equal(x, y) for x, y in zip(smp.tuning(), before[2]))
    first = smp.record_fetch(1)                              # the oldest one only
    assert np.array_equal(first[0], [2]) and smp.record_count() == 1
    smp.run_schedule(sched[5:8])                             # the same run fits now; its samples wrap around the ring
    case.check_path(smp)
    rest = smp.record_fetch()
    assert np.array_equal(rest[0], [4, 6, 8]) and smp.record_count() == 0
    # ... and are what a plain sampler holds after the same calls
    plain = case.sampler()
    plain.run_schedule(sched[:5])
    plain.run_schedule(sched[5:8])
    same_state(plain.state(), sample_fields(rest, 2))
    assert np.array_equal(rest[4][2], plain.posterior())
    smp.set_state(case.s0)                                   # allowed while recording; the count goes on
    smp.run_schedule(sched[:2])
    assert np.array_equal(smp.record_fetch()[0], [10])
    smp.record_end()
    smp.close()                                              # (and a handle destroyed with an active recorder frees it)
    smp2 = case.sampler()
    smp2.record_begin(1, 2)
    smp2.close()


def test_mc3_temperatures_are_recorded(gpu, knobs):
    case = Case("1-chain-lds", knobs)
    case.B = 8
    case.s0 = case.s0.slice(0, 8)
    smp = case.sampler(seed=5)
    mc3 = M.MC3(smp, n_chains=4, swap_period=2, n_swaps=3, betas=[1.0, 0.9, 0.8, 0.7], seed=11)
    n_periods = 6
    smp.record_begin(2, n_periods)
    betas, colds = [], []
    for _ in range(n_periods):                               # MC3.run period by period: the temperatures each period ran with
        b = np.empty(8)
        _capi.check(_capi.lib().mcd_mh_mc3_get(smp._h, None, None, None, b.ctypes.data_as(C.POINTER(C.c_double))))
        betas.append(b)
        colds.append(mc3.cold())
        mc3.run(2)
    case.check_path(smp)
    it, sc, H, R, post, beta = smp.record_fetch()
    assert np.array_equal(it, 2 * np.arange(1, n_periods + 1))
    assert np.array_equal(beta, np.array(betas))
    assert len({tuple(b) for b in betas}) > 1, "no swap was accepted: the test shows nothing"
    for k in range(n_periods):
        assert np.array_equal(np.nonzero(beta[k] == 1.0)[0], colds[k])
    smp.record_end()


def test_monitor_record_equals_collect_and_prior_components(gpu, knobs, tmp_path):
    case = Case("1-chain-lds", knobs)
    a, b = case.sampler(seed=9), case.sampler(seed=9)
    n_iter, period = 12, 2
    tr_c = monitor.collect(a, n_iter, period=period, accumulate=True)
    tr_r = monitor.record(b, n_iter, period=period, accumulate=True, chunk=period)
    case.check_path(b)
    assert np.array_equal(tr_c.iteration, tr_r.iteration) and len(tr_r.iteration) == n_iter // period
    for f in FIELDS:
        assert np.array_equal(getattr(tr_c, f), getattr(tr_r, f)), f
    assert tr_c.post is None and tr_r.post.shape == (6, case.B, 3) and np.array_equal(tr_r.post[-1], b.posterior())
    assert all(np.array_equal(x, y) for x, y in zip(a.age_sums(), b.age_sums()))
    # a longer chunk on a third twin: path 1 evaluates every step in full, so cutting the run differently changes nothing
    c = case.sampler(seed=9)
    tr_l = monitor.record(c, n_iter, period=period, accumulate=True, chunk=5)
    for f in FIELDS + ("iteration", "post"):
        assert np.array_equal(getattr(tr_l, f), getattr(tr_r, f)), f
    comp = monitor.prior_components(case.pf, tr_r)
    assert comp.shape == (6, case.B, 3)
    for k in range(6):
        for ch in range(case.B):
            _, one = case.pf.logprior(tr_r.states(k).slice(ch, ch + 1), want_components=True)
            assert np.array_equal(comp[k, ch], one[0]), (k, ch)
    assert np.allclose(comp.sum(axis=2), tr_r.post[:, :, 0], rtol=1e-10, atol=1e-8)      # (the chain kernel keeps the blocks it did not move)
    f1 = monitor.write_monitor_files(str(tmp_path / "a"), tr_r, 3, case.topo, prior=case.pf)
    f2 = monitor.write_monitor_files(str(tmp_path / "b"), tr_r, 3, case.topo, components=comp)
    assert len(f1) == len(f2) == 4
    for x, y in zip(f1, f2):
        assert open(x).read() == open(y).read(), (x, y)
