"""The sample recorder of the NUTS driver (mcd_hmc_record_*, csrc/k_hmc_record.hip): thinned samples and the transitions' diagnostics kept on
the device while mcd_hmc_nuts / _nuts_run / _nuts_warmup run, and their summaries computed where they lie.

Shapes: the committed 06-leaves (11 nodes), 12-leaves (23 nodes, over the thinned sparse matrix of tests/test_gpu_sparse_hmc.py) and
24-leaves-braces (47 nodes) inputs; 3 chains (odd) and 70 (past a wave's width); one case moves its states through the C ABI with
ld_state = n_nodes + 3; max_depth 4 - 5, 12 - 24 transitions.  References: the same handle without a recorder (same bits), a loop of
mcd_hmc_nuts with a state read-back per transition (same bits), mcd_trace_summary on the fetched samples (same bits) and
diagnostics.summary under the tolerances of tests/test_gpu_mh_summary.py, numpy reductions of the fetched diagnostics, and for the
diverged flag a CPU twin on the oracles that follows the device's random streams (tests/test_gpu_nuts.py) and stops a sub tree on the
Delta_max test of hmc._nuts_chain (`log_u < DELTA_MAX + joint`).  ln prior + ln likelihood + ln jacobianRootBranch of a sample against
mcd_hmc_get_position's value: 1e-12 max(1, |value|), the project's fp64 bound for one re-evaluated sum."""
import ctypes as C
import math

import numpy as np
import pytest

import mcmc_date_amd as M
import oracle as O
import test_gpu_mh_summary as TS
import test_gpu_nuts as TN
import test_gpu_sparse_hmc as TSH
from mcmc_date_amd import _capi, hmc, monitor

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
FIELDS = ("time_birth_rate", "time_death_rate", "time_height", "heights", "rate_mean", "rate_variance", "rates")
# name -> (likelihood, fixture, chains, ld_state - n_nodes, max_depth)
CASES = {
    "dense-11-nodes-3-chains": ("dense", "06-leaves-constant-rate", 3, 0, 5),
    "sparse-23-nodes-70-chains": ("sparse", "12-leaves-variable-rate", 70, 3, 4),
    "dense-47-nodes-70-chains": ("dense", "24-leaves-braces", 70, 0, 4),
}
SEED, T0, N_TRANS = 20261018, 100, 24
_cache = {}


def _p(a):
    return a.ctypes.data_as(_dp)


class Case:
    """Likelihood, prior, step sizes, masses and separated start states of one case (made once), and fresh drivers on them."""

    def __init__(self, golden, name):
        kind, fxname, self.B, self.pad, self.max_depth = CASES[name]
        fx = golden[fxname]
        self.topo = topo = M.Topology(fx["parent"])
        cal, con, br = TN.tables(fx)
        ht = float(fx["prior_ht"])
        self.cal = len(cal) > 0
        self.pf = M.PriorFunction(ht, "UncorrelatedGamma", cal, con, br, topo)
        if kind == "sparse":
            self.lik = M.SparseLikelihood(TSH.thinned_fixture(fx)[1]).bind_tree(topo)
        else:
            self.lik = M.MvnLikelihood(M.Full(fx["mu"], fx["sigma_inv"], float(fx["logdet"]))).bind_tree(topo)
        x0 = M.init_with(topo, fx["mean_lengths"])
        if self.cal:
            x0.time_height = ht
        # typical posterior states, different per chain (as tests/test_gpu_nuts.py), then a short adaptation of the step sizes
        ps, _ = M.proposals(topo, br, calibrations_available=self.cal)
        smp = M.Sampler(self.lik, self.pf, ps, self.B, seed=3)
        smp.set_initial_state(x0)
        smp.burn_in(fast=[10, 10, 20, 40], slow=[100, 100])
        lf = M.Leapfrog(self.lik, self.pf, self.cal, self.B)
        lf.set_state(smp.state())
        q0 = lf.position()[0]
        self.inv_mass = np.maximum((0.1 * np.abs(q0)).mean(axis=0) ** 2, 1e-12)
        self.eps, _, _, _ = lf.nuts_run(20, 0.05, self.inv_mass, adapt=True, max_depth=5, seed=1)
        assert np.all(np.isfinite(self.eps)) and np.all(self.eps > 0)
        self.start = lf.state()
        assert np.unique(self.start.rate_mean).size == self.B
        lf.close()

    def fresh(self):
        lf = M.Leapfrog(self.lik, self.pf, self.cal, self.B)
        set_state(self, lf, self.start)
        return lf


def case_of(golden, name):
    if name not in _cache:
        _cache[name] = Case(golden, name)
    return _cache[name]


def set_state(case, lf, s):
    """Through the C ABI with ld_state = n_nodes + pad (the padding poisoned: nothing may read it)."""
    nn, B, ld = case.topo.n_nodes, case.B, case.topo.n_nodes + case.pad
    H, R = np.full((B, ld), np.nan), np.full((B, ld), np.nan)
    H[:, :nn], R[:, :nn] = s.heights, s.rates
    f = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    a = [f(s.time_birth_rate), f(s.time_death_rate), f(s.time_height), H, f(s.rate_mean), f(s.rate_variance), R]
    _capi.check(_capi.lib().mcd_hmc_set_state(lf._h, *[_p(x) for x in a], ld))


def get_state(case, lf):
    nn, B, ld = case.topo.n_nodes, case.B, case.topo.n_nodes + case.pad
    birth, death, tH, rMu, rVar = (np.empty(B) for _ in range(5))
    H, R = np.full((B, ld), -7.0), np.full((B, ld), -7.0)
    _capi.check(_capi.lib().mcd_hmc_get_state(lf._h, *[_p(a) for a in (birth, death, tH, H, rMu, rVar, R)], ld))
    assert np.all(H[:, nn:] == -7.0) and np.all(R[:, nn:] == -7.0)
    return M.StateBatch(np.ascontiguousarray(H[:, :nn]), np.ascontiguousarray(R[:, :nn]), tH, rMu, birth, death, rVar)


def same_state(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def reference(golden, name):
    """The period-1 record of N_TRANS transitions in one call (transitions T0 ..), and the end state: made once per case."""
    key = ("ref", name)
    if key not in _cache:
        case = case_of(golden, name)
        lf = case.fresh()
        lf.record_begin(1, N_TRANS)
        out = lf.nuts_run(N_TRANS, case.eps, case.inv_mass, adapt=False, max_depth=case.max_depth, seed=SEED, first_transition=T0)
        assert lf.record_count() == N_TRANS
        f = lf.record_fetch()
        assert lf.record_count() == 0 and np.array_equal(f[0], np.arange(1, N_TRANS + 1))
        end = get_state(case, lf)
        lf.record_end()
        lf.close()
        for a in f:
            a.setflags(write=False)
        _cache[key] = (f, end, out)
    return _cache[key]


@pytest.mark.parametrize("mode", ["run", "run-adapt", "warmup"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_chains_do_not_change(gpu, golden, name, mode):
    case = case_of(golden, name)

    def go(record):
        lf = case.fresh()
        if record:
            lf.record_begin(2, 16)
        if mode == "warmup":
            out = lf.nuts_warmup(case.eps, case.inv_mass, windows=2, window=4, delta=0.65, max_depth=case.max_depth, seed=SEED, first_transition=T0)
        else:
            out = lf.nuts_run(12, case.eps, case.inv_mass, adapt=(mode == "run-adapt"), delta=0.65, max_depth=case.max_depth, seed=SEED,
                              first_transition=T0)
        n = lf.record_count() if record else None
        st = get_state(case, lf)
        pos = lf.position()
        lf.close()                                             # (mcd_hmc_destroy frees an active ring)
        return out, st, pos, n

    plain, st_p, pos_p, _ = go(False)
    rec, st_r, pos_r, n = go(True)
    assert n == 6
    assert same_state(st_p, st_r)
    for a, b in zip(plain, rec):                               # eps, mean_alpha, q_mean, q_var / eps, inv_mass, mean_alpha
        assert np.array_equal(a, b, equal_nan=True)
    for a, b in zip(pos_p, pos_r):
        assert np.array_equal(a, b, equal_nan=True)
    assert all(np.all(np.isfinite(a)) for a in plain)


@pytest.mark.parametrize("name", list(CASES))
def test_recorded_equals_the_cut_run(gpu, golden, name):
    case = case_of(golden, name)
    (it, sc, H, R, post, nuts), end, (eps_out, mean_alpha, q_mean, q_var) = reference(golden, name)
    n = 12
    cut = case.fresh()
    s1, s2, asum = np.zeros(cut.dim), np.zeros(cut.dim), np.zeros(case.B)
    for t in range(N_TRANS):
        alpha, depth = cut.nuts(case.eps, case.inv_mass, max_depth=case.max_depth, seed=SEED, transition=T0 + t)
        q, value, _ = cut.position()
        for b in range(case.B):                                # the order of summation mcd_hmc_nuts_run documents: b, then k, transitions in order
            s1 += q[b]
            s2 += q[b] * q[b]
        asum += alpha
        if t >= n:
            continue
        st = get_state(case, cut)
        assert np.array_equal(sc[t], np.stack([st.time_birth_rate, st.time_death_rate, st.time_height, st.rate_mean, st.rate_variance], axis=1)), t
        assert np.array_equal(H[t], st.heights) and np.array_equal(R[t], st.rates), t
        assert np.array_equal(nuts[t, :, 2], alpha) and np.array_equal(nuts[t, :, 0], depth.astype(np.float64)), t
        assert np.array_equal(nuts[t, :, 4], case.eps), t
        total = (post[t, :, 0] + post[t, :, 1]) + post[t, :, 2]
        err = np.abs(total - value) / np.maximum(1.0, np.abs(value))
        print(f"{name} transition {t}: ln posterior of the sample against the handle's value, largest error {err.max():.2e}")
        assert np.all(err <= 1e-12), (t, err.max())
        assert np.all(nuts[t, :, 1] >= 1) and np.all(nuts[t, :, 1] <= 2 ** case.max_depth - 1) and np.all((nuts[t, :, 3] == 0) | (nuts[t, :, 3] == 1))
        assert np.all(np.isfinite(nuts[t, :, 5]))
    assert same_state(get_state(case, cut), end)
    # the position moments of the run in one call, now summed on the device: the bits of the host loop above
    cnt = float(case.B) * N_TRANS
    mean = s1 / cnt
    assert np.array_equal(q_mean, mean) and np.array_equal(q_var, s2 / cnt - mean * mean)
    assert np.array_equal(mean_alpha, asum / N_TRANS) and np.array_equal(eps_out, case.eps)
    cut.close()


@pytest.mark.parametrize("name", list(CASES))
def test_thinning_wrap_and_refusal(gpu, golden, name):
    case = case_of(golden, name)
    ref, _, _ = reference(golden, name)
    L = _capi.lib()
    kw = dict(adapt=False, max_depth=case.max_depth, seed=SEED)
    lf = case.fresh()
    lf.record_begin(3, 4)
    with pytest.raises(_capi.McdError, match="active already"):
        lf.record_begin(1, 4)
    lf.nuts_run(5, case.eps, case.inv_mass, first_transition=T0, **kw)
    assert lf.record_count() == 1
    lf.nuts_run(7, case.eps, case.inv_mass, first_transition=T0 + 5, **kw)
    assert lf.record_count() == 4                               # transitions 3, 6, 9, 12: the ring is full
    before = get_state(case, lf)
    for call, adds in ((lambda: lf.nuts_run(9, case.eps, case.inv_mass, first_transition=T0 + 12, **kw), 3),
                       (lambda: lf.nuts_warmup(case.eps, case.inv_mass, windows=1, window=3, max_depth=case.max_depth, seed=SEED,
                                               first_transition=T0 + 12), 2)):
        with pytest.raises(_capi.McdError) as e:
            call()
        code, msg = e.value.code, str(e.value)
        del e
        assert code == _capi.MCD_ERR_INVALID_ARG and f"record {adds} samples" in msg and "has 0 free slots" in msg, msg
        assert f"record {adds} samples" in L.mcd_last_error().decode()
        assert lf.record_count() == 4 and same_state(get_state(case, lf), before)
    set_state(case, lf, before)                                 # mcd_hmc_set_state leaves the recorder and its count alone
    assert lf.record_count() == 4
    first = lf.record_fetch(2)
    assert np.array_equal(first[0], [3, 6]) and lf.record_count() == 2
    lf.nuts_run(6, case.eps, case.inv_mass, first_transition=T0 + 12, **kw)       # samples 5 and 6 go to slots 0 and 1: the ring wraps
    rest = lf.record_fetch()
    assert np.array_equal(rest[0], [9, 12, 15, 18]) and lf.record_count() == 0
    for k, a in enumerate(ref):
        got = np.concatenate([first[k], rest[k]])
        assert np.array_equal(got, a[2:18:3]), k
    lf.record_end()
    with pytest.raises(_capi.McdError, match="no recorder is active"):
        lf.record_count()
    # mcd_hmc_nuts alone: refused when its sample has no slot, allowed again after a fetch
    lf.record_begin(1, 2)
    for t in range(2):
        lf.nuts(case.eps, case.inv_mass, max_depth=case.max_depth, seed=SEED, transition=T0 + 18 + t)
    before = get_state(case, lf)
    with pytest.raises(_capi.McdError) as e:
        lf.nuts(case.eps, case.inv_mass, max_depth=case.max_depth, seed=SEED, transition=T0 + 20)
    code, msg = e.value.code, str(e.value)
    del e
    assert code == _capi.MCD_ERR_INVALID_ARG and "record 1 samples" in msg and "has 0 free slots" in msg, msg
    assert lf.record_count() == 2 and same_state(get_state(case, lf), before)
    got = lf.record_fetch(1)
    assert np.array_equal(got[0], [1])
    for k in range(1, 6):
        assert np.array_equal(got[k][0], ref[k][18]), k
    lf.nuts(case.eps, case.inv_mass, max_depth=case.max_depth, seed=SEED, transition=T0 + 20)
    got = lf.record_fetch()
    assert np.array_equal(got[0], [2, 3])
    for k in range(1, 6):
        assert np.array_equal(got[k], ref[k][19:21]), k
    lf.record_end()
    lf.close()


def raw_summary(lf, skip, n, max_lag):
    Q = 2 * lf.topo.n_nodes + 9
    pooled, pc, stats = np.empty((Q, 9)), np.empty((lf.batch, Q, 4)), np.empty((lf.batch, 4))
    used = C.c_int64(-1)
    rc = _capi.lib().mcd_hmc_record_summary(lf._h, skip, n, max_lag, C.byref(used), _p(pooled), _p(pc), _p(stats))
    return rc, used.value, pooled, pc, stats


@pytest.mark.parametrize("name", list(CASES))
def test_summary_where_the_samples_lie(gpu, golden, name):
    case = case_of(golden, name)
    kw = dict(adapt=False, max_depth=case.max_depth, seed=SEED)
    lf = case.fresh()
    with pytest.raises(_capi.McdError, match="no recorder is active"):
        lf.record_summary()
    lf.record_begin(1, 16)
    lf.nuts_run(10, case.eps, case.inv_mass, first_transition=T0, **kw)
    assert len(lf.record_fetch(6)[0]) == 6
    lf.nuts_run(12, case.eps, case.inv_mass, first_transition=T0 + 10, **kw)
    assert lf.record_count() == 16                              # samples 7 .. 22 in slots 6 .. 15, 0 .. 5
    Q = C.c_int64(0)
    _capi.check(_capi.lib().mcd_hmc_record_quantities(lf._h, C.byref(Q)))
    assert Q.value == 2 * case.topo.n_nodes + 9
    before = get_state(case, lf)
    whole = lf.record_summary(max_lag=5, per_chain=True)
    part = lf.record_summary(skip=3, n=10, max_lag=3, per_chain=True)      # slots 9 .. 15, 0 .. 2
    again = lf.record_summary(skip=3, n=10, max_lag=3, per_chain=True)
    assert whole.n_samples == 16 and whole.max_lag == 5 and part.n_samples == 10 and part.max_lag == 3
    for a, b in ((part.pooled, again.pooled), (part.per_chain, again.per_chain), (part.nuts_stats, again.nuts_stats)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # refusals before any launch: a bad window, a bad max_lag
    for args, word in (((16, -1, 1), "16 samples are waiting"), ((10, 7, 1), "ends past the 16 waiting"), ((0, -1, 4), "odd")):
        rc, used, _, _, _ = raw_summary(lf, *args)
        assert rc == _capi.MCD_ERR_INVALID_ARG and used == 0 and word in _capi.lib().mcd_last_error().decode(), args
    assert lf.record_count() == 16 and same_state(get_state(case, lf), before)
    f = lf.record_fetch()
    assert np.array_equal(f[0], np.arange(7, 23))               # a summary frees no slot
    ref, _, _ = reference(golden, name)
    for k in range(1, 6):
        assert np.array_equal(f[k], ref[k][6:22]), k
    x = TS.quantities(f)
    for got, xs, lag, label in ((whole, x, 5, "whole"), (part, x[3:13], 3, "across the wrap")):
        dev = M.trace_summary(np.ascontiguousarray(xs), max_lag=lag)
        assert np.array_equal(got.pooled.view(np.uint64), dev.pooled.view(np.uint64)), label
        assert np.array_equal(got.per_chain.view(np.uint64), dev.per_chain.view(np.uint64)), label
        TS.compare(got, xs, lag, f"{name}, {label}")
        nuts = f[5][3:13] if xs is not x else f[5]
        want = np.stack([nuts[:, :, 3].sum(axis=0), nuts[:, :, 0].mean(axis=0), nuts[:, :, 0].max(axis=0), nuts[:, :, 1].sum(axis=0)], axis=1)
        assert np.array_equal(got.nuts_stats, want), label
    # the monitor's summary takes the driver as it takes a Sampler
    lf.nuts_run(8, case.eps, case.inv_mass, first_transition=T0 + 22, **kw)
    ages = monitor.summarize_recorded(lf, burn_in=0.25, max_lag=1)
    got = lf.record_summary(skip=2, max_lag=1)
    assert np.array_equal(ages.mean, got.ages[:, 0]) and np.array_equal(ages.rhat, got.ages[:, 6], equal_nan=True)
    lf.record_end()
    lf.close()


def test_record_nuts_feeds_the_monitor_files(gpu, golden, tmp_path):
    name = "dense-11-nodes-3-chains"
    case = case_of(golden, name)
    ref, _, _ = reference(golden, name)
    lf = case.fresh()
    tr = monitor.record_nuts(lf, 12, case.eps, case.inv_mass, period=2, chunk=5, max_depth=case.max_depth, seed=SEED, first_transition=T0)
    assert np.array_equal(tr.iteration, T0 + np.arange(2, 13, 2))
    assert np.array_equal(tr.heights, ref[2][1:12:2]) and np.array_equal(tr.post, ref[4][1:12:2]) and np.array_equal(tr.nuts, ref[5][1:12:2])
    assert tr.beta is None
    files = monitor.write_monitor_files(str(tmp_path / "chain0"), tr, 0, case.topo)
    assert len(files) == 3 and len(open(files[0]).read().splitlines()) == 7
    with pytest.raises(_capi.McdError, match="no recorder is active"):
        lf.record_count()
    lf.close()


# ---- the diverged flag against the CPU twin --------------------------------------------------------------------------------------------
# Chosen on the CPU with the twin alone (choose_divergence_setting below; no device involved), from the 12-leaves start state of
# divergence_problem with the masses (0.1 q)^2.  There the twin's acceptance statistic is 1 at the step size 0.03 and every transition
# fails the Delta_max test from 0.15 on (so at 50 x 0.03 = 1.5 as well: all of 1.5, 2, 2.5, 3 x seeds 1 .. 8 are divergent throughout, which
# shows no non-divergent transition); at 0.1 none fails.  Two chains at either side of that threshold show both kinds.
DIV_SEED, DIV_EPS, DIV_CHAINS, DIV_TRANSITIONS, DIV_DEPTH = 1, np.array([0.1, 0.1, 0.15, 0.15]), 4, 2, 4


def twin_transition_with_flag(tw, q0, g0, lp0, eps, inv_mass, max_depth, seed, chain, transition):
    """tests/test_gpu_nuts.py: twin_transition (the device's state machine and random streams on the CPU oracles) that also says whether a
    leaf failed hmc._nuts_chain's Delta_max test.  Returns (depth, diverged, q_new)."""
    dim = len(q0)
    uni = lambda d: O.uniform_pair(seed, chain, transition, d)
    p0 = np.empty(dim)
    for k in range(dim):
        ua, ub = uni(0x4000 + (k >> 1))
        rad, ang = math.sqrt(-2.0 * math.log(ua)), 6.28318530717958647692 * ub
        p0[k] = (rad * math.sin(ang) if (k & 1) else rad * math.cos(ang)) / math.sqrt(inv_mass[k])
    joint0 = lp0 - 0.5 * float(np.sum(p0 * p0 * inv_mass))
    log_u = joint0 + math.log(uni(1)[0])
    minus, plus = [q0.copy(), p0.copy(), g0.copy()], [q0.copy(), p0.copy(), g0.copy()]
    prop = q0.copy()
    n, j, leaf, diverged = 1, 0, 0, False

    def no_u_turn(qm, rm, qp, rp):
        d = qp - qm
        return float(np.dot(d, rm * inv_mass)) >= 0.0 and float(np.dot(d, rp * inv_mass)) >= 0.0

    while True:
        v = -1 if uni(0x10 + 2 * j)[0] < 0.5 else 1
        edge = minus if v < 0 else plus
        n1, s1, cand, stack = 0, True, None, {}
        for i in range(1 << j):
            q, p, g = edge
            e = eps * v
            p = p + 0.5 * e * g
            q = q + e * inv_mass * p
            with np.errstate(all="ignore"):
                lp = tw.value(q)
                g = tw.grad(q) if math.isfinite(lp) else np.full(dim, np.nan)
            p = p + 0.5 * e * g
            edge[0], edge[1], edge[2] = q, p, g
            joint = lp - 0.5 * float(np.sum(p * p * inv_mass))
            if not math.isfinite(joint):
                joint = -math.inf
            nl, sl = log_u <= joint, log_u < hmc.DELTA_MAX + joint
            diverged = diverged or not sl
            if nl:
                n1 += 1
                if uni(0x100000 + leaf)[0] * n1 < 1.0:
                    cand = q.copy()
            s1 = s1 and sl
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
            return j + 1, diverged, prop
        if n1 > 0 and uni(0x11 + 2 * j)[0] * n < n1:
            prop = cand
        n += n1
        s = no_u_turn(minus[0], minus[1], plus[0], plus[1])
        j += 1
        if not s or j >= max_depth:
            return j, diverged, prop


def divergence_problem(golden):
    fx = golden["12-leaves-variable-rate"]
    topo = M.Topology(fx["parent"])
    cal, con, br = TN.tables(fx)
    ht = float(fx["prior_ht"])
    spec = O.PriorSpec(fx["parent"], ht, "UncorrelatedGamma", [(c.node, c.lower, c.lower_p, c.upper, c.upper_p) for c in cal],
                       [(k.young, k.old, k.p) for k in con], [(b.nodes, b.sd) for b in br])
    x0 = M.init_with(topo, fx["mean_lengths"])
    x0.time_height = ht
    # init_with's unit rates put the distances three orders of magnitude above the data's: one mean rate brings their sum to the data's
    d = O.distances(topo.parent, np.asarray(x0.time_tree), np.asarray(x0.rate_tree), x0.time_height, x0.rate_mean)
    x0.rate_mean = float(np.sum(fx["mu"]) / np.sum(d))
    mask = M.get_mask(True, topo)
    q0 = M.to_vector(mask, x0)
    inv_mass = np.maximum((0.1 * np.abs(q0)) ** 2, 1e-12)
    return fx, topo, (cal, con, br), ht, spec, x0, mask, q0, inv_mass


def choose_divergence_setting(golden, seed, eps):
    """The twin alone, every chain walking on from its own selected point: [transition][chain] diverged flags."""
    fx, topo, _, _, spec, x0, mask, q0, inv_mass = divergence_problem(golden)
    tw = TN.Twin(fx, spec, mask, x0)
    flags = np.zeros((DIV_TRANSITIONS, DIV_CHAINS), bool)
    for b in range(DIV_CHAINS):
        q = q0.copy()
        for t in range(DIV_TRANSITIONS):
            _, flags[t, b], q = twin_transition_with_flag(tw, q, tw.grad(q), tw.value(q), eps[b], inv_mass, DIV_DEPTH, seed, b, t)
    return flags


def test_the_diverged_flag_is_the_twins(gpu, golden):
    fx, topo, (cal, con, br), ht, spec, x0, mask, q0, inv_mass = divergence_problem(golden)
    B = DIV_CHAINS
    pf = M.PriorFunction(ht, "UncorrelatedGamma", cal, con, br, topo)
    lik = M.MvnLikelihood(M.Full(fx["mu"], fx["sigma_inv"], float(fx["logdet"]))).bind_tree(topo)
    lf = M.Leapfrog(lik, pf, True, B)
    lf.set_state(M.StateBatch.from_states([x0] * B))
    tw = TN.Twin(fx, spec, mask, x0)
    lf.record_begin(1, DIV_TRANSITIONS)
    flags, followed = [], []
    for t in range(DIV_TRANSITIONS):
        q_b, lp_b, g_b = lf.position()
        _, depth = lf.nuts(DIV_EPS, inv_mass, max_depth=DIV_DEPTH, seed=DIV_SEED, transition=t)
        res = [twin_transition_with_flag(tw, q_b[b], g_b[b], lp_b[b], DIV_EPS[b], inv_mass, DIV_DEPTH, DIV_SEED, b, t) for b in range(B)]
        flags.append([r[1] for r in res])
        followed.append([r[0] == depth[b] for b, r in enumerate(res)])
    flags, followed = np.array(flags), np.array(followed)
    stats = lf.record_summary(max_lag=0).nuts_stats
    nuts = lf.record_fetch()[5]
    lf.record_end()
    lf.close()
    keep = followed.all(axis=0)                                 # the chains on which the twin follows the device in depth
    print(f"twin follows the device on chains {np.flatnonzero(keep).tolist()}; twin flags {flags.astype(int).tolist()}, device {nuts[:, :, 3].astype(int).tolist()}")
    assert keep.sum() >= B - B // 4 and np.array_equal(nuts[0, :, 4], DIV_EPS)
    assert flags[:, keep].any() and not flags[:, keep].all()    # at least one divergent and one non-divergent transition
    assert np.array_equal(nuts[:, keep, 3], flags[:, keep].astype(np.float64))
    assert np.array_equal(stats[:, 0], nuts[:, :, 3].sum(axis=0)) and np.array_equal(stats[:, 2], nuts[:, :, 0].max(axis=0))
    assert np.array_equal(stats[:, 1], nuts[:, :, 0].mean(axis=0)) and np.array_equal(stats[:, 3], nuts[:, :, 1].sum(axis=0))
