"""Checkpoint and continue of the device sampler (mcd_mh_save / mcd_mh_load; `Settings ... Save`, `continue` and `--init-from-save` of the
reference, app/Main.hs:494-509 and :424-440).  The property under test is an equivalence of bits: "one handle, two calls" against "first
call, save, fresh handle, load, second call", on every launch structure of the driver -- so no test here has a tolerance."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi, checkpoint as K

pytestmark = pytest.mark.gpu

# case -> (fixture name or number of leaves, sparse handle, chains, knobs, what last_path() must say)
CASES = {
    "chain_lds": ("12-leaves-variable-rate", False, 3, {}, "factor resident in LDS"),
    "streamed": (33, False, 3, {}, "two chains per workgroup"),
    "two_launch": (33, False, 3, {"MCD_MH_PER_PHASE": "1"}, "two launches per lock step"),
    "segments": (130, False, 2, {}, "segments: "),
    "step_wg": (161, False, 2, {"MCD_MH_SEGMENTS": "0"}, "workgroup-per-chain step kernel"),
    "sparse_segments": ("24-leaves-braces", True, 3, {}, "segments over a sparse precision matrix"),
}
SEED = 13
STATE_FIELDS = ("heights", "rates", "time_height", "rate_mean", "rate_variance", "time_birth_rate", "time_death_rate")
INVALID = _capi.MCD_ERR_INVALID_ARG


@functools.lru_cache(maxsize=None)
def problem(tree, max_B=8):
    """Everything but the handles: topology, likelihood operands, the prior's arguments, proposal table, initial states for up to max_B chains
    and the schedules -- two tuning periods, call 1 (about 300 lock steps) and call 2 (about 600, so that the recomputation of z every 256
    steps falls inside it); whole iterations on the fixtures, slices of one long cycle on the random trees."""
    from mcmc_date_amd import synthetic as S

    if isinstance(tree, int):
        topo = S.random_topology(tree, seed=7)
        mu, sigma = S.random_spd_problem(topo.n_nodes - 2, seed=7)
        sigma_inv, logdet = np.linalg.inv(sigma), float(np.linalg.slogdet(sigma)[1])
        s0 = S.random_states(topo, max_B, seed=8)
        s0.time_birth_rate = np.full(max_B, 1.0); s0.time_death_rate = np.full(max_B, 0.8); s0.rate_variance = np.full(max_B, 0.3)
        cal = [M.Calibration("root", 0, 0.9, 0.025, 1.1, 0.025), M.Calibration("n", 5, 0.2, 0.025, None, 0.0)]
        con, br, ht = [], [], 1.0
        ps, _ = M.proposals(topo, [], calibrations_available=True)
        flat = M.cycle_schedule(ps, 2, np.random.default_rng(0)).reshape(1, -1)
        assert flat.shape[1] >= 1020
        cuts = [0, 60, 120, 420, 1020]
        tune1, tune2, call1, call2 = (flat[:, a:b] for a, b in zip(cuts[:-1], cuts[1:]))
    else:
        fx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", tree + ".npz")))
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
        s0 = M.StateBatch.from_states([x0] * max_B)
        per_iter = M.cycle_schedule(ps, 1, np.random.default_rng(0)).shape[1]
        k1, k2 = -(-300 // per_iter), -(-600 // per_iter)
        sched = M.cycle_schedule(ps, 2 + k1 + k2, np.random.default_rng(0))
        tune1, tune2, call1, call2 = sched[:1], sched[1:2], sched[2:2 + k1], sched[2 + k1:]
        assert call2.size > 256
    return dict(topo=topo, ps=ps, mu=np.asarray(mu), sigma_inv=sigma_inv, logdet=logdet, prior=(ht, "UncorrelatedGamma", cal, con, br), s0=s0,
                tune=(tune1, tune2), call1=call1, call2=call2)


def fresh(P, B, sparse=False, seed=SEED, ps=None, state=False):
    """A sampler over FRESH likelihood, prior and handle objects of the problem; state: put it into the problem's initial states."""
    topo = P["topo"]
    if sparse:
        Q = P["sigma_inv"]
        assoc = [((int(i), int(j)), float(Q[i, j])) for i in range(Q.shape[0]) for j in range(Q.shape[1])]
        lik = M.SparseLikelihood(M.Sparse(P["mu"], assoc, P["logdet"]), device=0).bind_tree(topo)
    else:
        lik = M.MvnLikelihood(M.Full(P["mu"], P["sigma_inv"], P["logdet"])).bind_tree(topo)
    ht, model, cal, con, br = P["prior"]
    smp = M.Sampler(lik, M.PriorFunction(ht, model, cal, con, br, topo), P["ps"] if ps is None else ps, B, seed=seed)
    if state:
        smp.set_state(rows(P["s0"], B))
    return smp


def rows(s, B):
    return M.StateBatch(**{f: np.ascontiguousarray(getattr(s, f)[:B]) for f in STATE_FIELDS})


def snapshot(smp):
    """Everything the accessors show of a handle between two runs."""
    s = smp.state()
    out = {f: np.array(getattr(s, f)) for f in STATE_FIELDS}
    out["posterior"] = smp.posterior()
    out["tune"], out["accepted"], out["tried"] = smp.tuning()
    out["age_sum"], out["age_sq"], n = smp.age_sums()
    out["n_samples"] = np.array(n)
    return out


def same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k}"


def to_call_1(smp, P):
    """Two short tuned periods (tuning parameters other than 1, counters other than 0 afterwards), then call 1 with the age sums."""
    for t in P["tune"]:
        smp.run_schedule(t)
        smp.autotune()
    smp.run_schedule(P["call1"], accumulate=True)


_scenarios = {}


def scenario(case, knobs):
    """Computed once per case and shared by the tests below: handle A (two tuned periods, call 1, save twice, call 2), handle C (the same
    without a save) and handle B (fresh objects, no set_state, load, save, call 2)."""
    tree, sparse, B, env, want = CASES[case]
    for k, v in env.items():
        knobs.setenv(k, v)
    if case in _scenarios:
        return _scenarios[case]
    P = problem(tree)
    r = dict(P=P, B=B)
    a = fresh(P, B, sparse, state=True)
    to_call_1(a, P)
    r["size"] = a.save_size()
    r["at_save"] = snapshot(a)
    r["blob"], r["blob_again"] = a.save(), a.save()
    r["a_trace"] = a.run_schedule(P["call2"], trace=True)
    r["a_path"] = a.last_path()
    r["a_end"] = snapshot(a)
    c = fresh(P, B, sparse, state=True)
    to_call_1(c, P)
    r["c_trace"] = c.run_schedule(P["call2"], trace=True)
    r["c_end"] = snapshot(c)
    b = fresh(P, B, sparse)
    with pytest.raises(M.McdError, match="set_state first"):
        b.run_schedule(P["call2"])
    b.load(r["blob"])
    r["b_loaded"] = snapshot(b)
    r["b_blob"] = b.save()
    r["b_trace"] = b.run_schedule(P["call2"], trace=True)
    r["b_path"] = b.last_path()
    r["b_end"] = snapshot(b)
    r["b_iterations"] = (a.iterations_done, b.iterations_done)
    _scenarios[case] = r
    return r


@pytest.mark.parametrize("case", list(CASES))
def test_continue_equals_uninterrupted(gpu, case, knobs):
    """Handle B -- fresh objects, never set_state, refused by run before the load -- runs call 2 from A's blob and gives A's call 2: ln
    acceptance ratios, decisions, the seven state fields, posterior terms, tuning parameters and counters, age sums and their count."""
    r = scenario(case, knobs)
    want = CASES[case][4]
    assert want in r["a_path"] and want in r["b_path"], (r["a_path"], r["b_path"])
    assert r["P"]["call2"].size > 256
    t, acc, tried = r["at_save"]["tune"], r["at_save"]["accepted"], r["at_save"]["tried"]
    assert np.any(t != 1.0) and np.any(tried != 0)                       # (the blob had something to carry)
    same(r["at_save"], r["b_loaded"], "after load")
    assert np.array_equal(r["a_trace"][0], r["b_trace"][0], equal_nan=True) and np.array_equal(r["a_trace"][1], r["b_trace"][1])
    same(r["a_end"], r["b_end"], "after call 2")
    assert r["b_iterations"][0] == r["b_iterations"][1]


@pytest.mark.parametrize("case", list(CASES))
def test_save_is_read_only(gpu, case, knobs):
    """A's call 2, behind two saves, is that of a handle that never saved."""
    r = scenario(case, knobs)
    assert np.array_equal(r["a_trace"][0], r["c_trace"][0], equal_nan=True) and np.array_equal(r["a_trace"][1], r["c_trace"][1])
    same(r["a_end"], r["c_end"], "saved against never saved")


@pytest.mark.parametrize("case", list(CASES))
def test_blob_is_deterministic_and_round_trips(gpu, case, knobs):
    """Two saves give the same bytes, B's save right behind its load gives A's blob, the section checksums that the pack kernel formed are
    the numpy restatement's, the parsed arrays are what the accessors return, and the size is DESIGN section 9's formula."""
    r = scenario(case, knobs)
    blob = r["blob"]
    assert blob == r["blob_again"] and blob == r["b_blob"]
    n = K.c_bytes(blob)
    P, B = r["P"], r["B"]
    assert n == r["size"] == K.save_size(B, P["topo"].n_nodes, len(P["ps"]))
    p = K.parse(blob)                                                    # (raises where a checksum of the device differs from numpy's)
    words = np.frombuffer(blob[:n], "<u8")
    for sid, off, nbytes, csum in p["sections"]:
        assert K.checksum(words[off // 8:(off + nbytes) // 8]) == csum and nbytes % 8 == 0
    info = _capi.ckpt_inspect(blob[:n])
    assert (info.n_nodes, info.n_prop, info.batch, info.seed) == (P["topo"].n_nodes, len(P["ps"]), B, SEED)
    assert info.dense == (0 if CASES[case][1] else 1) and info.topology == K.topology_hash(P["topo"].parent) and info.table == K.table_hash(M.table_arrays(P["ps"]))
    s = r["at_save"]
    for i, f in enumerate(("time_birth_rate", "time_death_rate", "time_height", "rate_mean", "rate_variance")):
        assert np.array_equal(p["sc"][i], s[f]), f
    for f in ("heights", "rates", "tune", "accepted", "tried", "age_sum", "age_sq"):
        assert np.array_equal(p[f], s[f]), f
    assert np.array_equal(p["post"], s["posterior"]) and p["meta"]["n_samples"] == int(s["n_samples"])
    assert p["meta"]["step"] == sum(x.size for x in P["tune"]) + P["call1"].size


def mc3_all(smp, mc):
    beta = np.empty(smp.batch)
    _capi.check(_capi.lib().mcd_mh_mc3_get(smp._h, None, None, None, beta.ctypes.data_as(C.POINTER(C.c_double))))
    return dict(rank=mc.rank, swaps_tried=mc.swaps_tried, swaps_accepted=mc.swaps_accepted, beta=beta, phase=np.array(mc.phase), **snapshot(smp))


def test_mc3_continues(gpu, knobs, tmp_path):
    """Six swap periods against three, a checkpoint file, a fresh handle with a fresh MC3, restore, three more: rank table, swap counters,
    temperatures, states and the phase.  A blob with MC3 needs mcd_mh_mc3_init done alike."""
    P = problem("12-leaves-variable-rate")
    mk = lambda: fresh(P, 8, state=True)
    u = mk()
    mu_ = M.MC3(u, n_chains=4, swap_period=2, n_swaps=3, seed=5)
    mu_.run(12)
    a = mk()
    ma = M.MC3(a, n_chains=4, swap_period=2, n_swaps=3, seed=5)
    ma.run(6)
    path = str(tmp_path / "mc3.ckpt")
    ma.checkpoint(path)
    b = fresh(P, 8)
    mb = M.MC3(b, n_chains=4, swap_period=2, n_swaps=3, seed=5)
    mb.restore(path)
    assert mb.phase == 3
    mb.run(6)
    same(mc3_all(u, mu_), mc3_all(b, mb), "mc3")
    assert mb.phase == 6 and np.any(mu_.swaps_accepted > 0)
    blob = open(path, "rb").read()
    with pytest.raises(M.McdError, match="mcd_mh_mc3_init") as e:
        fresh(P, 8).load(blob)
    assert e.value.code == INVALID
    other = fresh(P, 8, state=True)
    M.MC3(other, n_chains=4, swap_period=2, n_swaps=3, seed=5, betas=[1.0, 0.9, 0.8, 0.7])
    before = snapshot(other)
    with pytest.raises(M.McdError, match="ladder"):
        other.load(blob)
    same(before, snapshot(other), "refused")


def test_power_posterior_continues(gpu, knobs):
    """The power-posterior bit and the exponents travel in the blob: the loading handle never calls set_power."""
    P = problem("12-leaves-variable-rate")
    a = fresh(P, 3, state=True)
    a.set_power(np.array([0.0, 0.5, 1.0]))
    a.run_schedule(P["call1"])
    blob = a.save()
    assert K.parse(blob)["meta"]["lik_only"] == 1
    ta = a.run_schedule(P["call2"], trace=True)
    b = fresh(P, 3)
    b.load(blob)
    tb = b.run_schedule(P["call2"], trace=True)
    assert np.array_equal(ta[0], tb[0], equal_nan=True) and np.array_equal(ta[1], tb[1])
    same(snapshot(a), snapshot(b), "power")


def test_recorder_phase_continues(gpu, knobs):
    """Period 3: four iterations, fetch, save; the loading handle begins a recorder of period 3 and runs five more: the samples of
    iterations 6 and 9, as on the saved handle.  Waiting samples refuse a save; another period refuses the load."""
    P = problem("12-leaves-variable-rate")
    sched = M.cycle_schedule(P["ps"], 9, np.random.default_rng(1))
    a = fresh(P, 3, state=True)
    a.record_begin(3, 8)
    a.run_schedule(sched[:4])
    assert len(a.record_fetch()[0]) == 1
    blob = a.save()
    a.run_schedule(sched[4:])
    got_a = a.record_fetch()
    b = fresh(P, 3)
    b.record_begin(3, 8)
    b.load(blob)
    b.run_schedule(sched[4:])
    got_b = b.record_fetch()
    assert list(got_a[0]) == [6, 9] and len(got_a) == len(got_b)
    for x, y in zip(got_a, got_b):
        assert np.array_equal(x, y)
    a.run_schedule(sched[:3])                                            # iteration 12: a sample waits
    with pytest.raises(M.McdError, match="mcd_mh_record_fetch") as e:
        a.save()
    assert e.value.code == INVALID
    c = fresh(P, 3, state=True)
    c.record_begin(2, 8)
    before = snapshot(c)
    with pytest.raises(M.McdError, match="period"):
        c.load(blob)
    same(before, snapshot(c), "refused")
    d = fresh(P, 3)                                                      # no recorder: the counts are ignored
    d.load(blob)
    d.run_schedule(sched[4:])
    same(snapshot(b), snapshot(d), "without a recorder")


def test_attached_hamiltonian_continues(gpu, knobs):
    """Three attached iterations, save, a fresh sampler with a fresh leapfrog handle attached alike, load, three more: states, posterior
    terms and the transitions' sums.  A blob with an attachment needs one on the loading handle."""
    from hamiltonian_cases import Case

    case = Case("23-nodes-chain-lds", knobs)
    sched = case.schedule(6)
    a = case.sampler(batch=4)
    la = case.leapfrog(batch=4)
    eps, im = case.nuts_inputs(la, a)
    a.attach_hamiltonian(la, eps, im, max_depth=4)
    a.run_schedule(sched[:3])
    blob = a.save()
    a.run_schedule(sched[3:])
    b = M.Sampler(case.lik, case.pf, case.ps, 4, seed=a.seed)
    lb = case.leapfrog(batch=4)
    with pytest.raises(M.McdError, match="mcd_mh_attach_hamiltonian") as e:
        b.load(blob)
    assert e.value.code == INVALID
    b.attach_hamiltonian(lb, eps, im, max_depth=4)
    b.load(blob)
    b.run_schedule(sched[3:])
    same(snapshot(a), snapshot(b), "attached")
    sa, sb = a.hamiltonian_stats(), b.hamiltonian_stats()
    assert sa["transitions"] == sb["transitions"] == 6
    for k in ("alpha_sum", "depth_sum", "leapfrog_steps", "divergent"):
        assert np.array_equal(sa[k], sb[k]), k


def _flip(blob, byte, bit=0):
    x = bytearray(blob)
    x[byte] ^= 1 << bit
    return bytes(x)


def test_refusals_leave_the_handle_untouched(gpu, knobs):
    """Every mismatch of the configuration and every damaged blob is refused with MCD_ERR_INVALID_ARG and its own message; the refused
    handle shows the bits it showed before, and its next call is a control handle's."""
    from mcmc_date_amd import synthetic as S

    r = scenario("chain_lds", knobs)
    P, B = r["P"], r["B"]
    blob = r["blob"][:K.c_bytes(r["blob"])]
    p = K.parse(blob)
    tune_at = [off for sid, off, _, _ in p["sections"] if sid == K.SECTION_IDS["tune"]][0]
    v, w = fresh(P, B, state=True), fresh(P, B, state=True)
    for s in (v, w):
        s.run_schedule(P["tune"][0], accumulate=True)
    before = snapshot(v)

    def refused(smp, data, match):
        was = snapshot(smp)
        with pytest.raises(M.McdError, match=match) as e:
            smp.load(data)
        assert e.value.code == INVALID
        same(was, snapshot(smp), match)

    bumped = bytearray(blob)
    bumped[8:12] = (K.VERSION + 1).to_bytes(4, "little")
    refused(v, blob[:-16], "truncated")
    refused(v, blob[:40], "truncated")
    refused(v, _flip(blob, 0), "bad magic")
    refused(v, bytes(bumped), "unknown version 2")
    refused(v, _flip(blob, tune_at + 11, 5), "checksum does not match its bytes")
    refused(v, _flip(blob, 8 * K.W_SEED + 2, 3), "header's checksum")
    refused(fresh(P, B + 1, state=True), blob, "batch of 3 chains")
    ps2 = list(P["ps"])
    ps2[3] = M.Proposal(**{**ps2[3].__dict__, "p0": ps2[3].p0 * (1 + 2.0 ** -50)})
    refused(fresh(P, B, ps=ps2, state=True), blob, "another proposal table")
    refused(fresh(P, B, seed=SEED + 1, state=True), blob, "seed")
    refused(fresh(P, B, sparse=True, state=True), blob, "dense likelihood")
    # another topology of as many nodes, under a likelihood and prior of its own
    topo2 = S.random_topology(12, seed=3)
    assert topo2.n_nodes == P["topo"].n_nodes and not np.array_equal(topo2.parent, P["topo"].parent)
    mu, sigma = S.random_spd_problem(topo2.n_nodes - 2, seed=3)
    lik2 = M.MvnLikelihood.from_covariance(mu, sigma).bind_tree(topo2)
    pf2 = M.PriorFunction(1.0, "UncorrelatedGamma", [], [], [], topo2)
    t2 = M.Sampler(lik2, pf2, M.proposals(topo2, [])[0], B, seed=SEED)
    s2 = S.random_states(topo2, B, seed=2)
    s2.time_birth_rate = np.full(B, 1.0); s2.time_death_rate = np.full(B, 0.8); s2.rate_variance = np.full(B, 0.3)
    t2.set_state(s2)
    refused(t2, blob, "another topology")
    # a buffer too small for the save: the needed size in the message and in *written
    need, n = v.save_size(), C.c_int64(0)
    buf = C.create_string_buffer(need - 8)
    assert _capi.lib().mcd_mh_save(v._h, buf, need - 8, C.byref(n)) == INVALID
    assert n.value == need and str(need) in _capi.lib().mcd_last_error().decode()
    same(before, snapshot(v), "after all refusals")
    tv, tw = v.run_schedule(P["call1"], trace=True), w.run_schedule(P["call1"], trace=True)
    assert np.array_equal(tv[0], tw[0], equal_nan=True) and np.array_equal(tv[1], tw[1])
    same(snapshot(v), snapshot(w), "next call")


def test_state_and_tuning_mode(gpu, knobs):
    """`--init-from-save`: a handle with another seed takes states, posterior terms and tuning parameters; its counters are zero, its age
    sums and recorder its own, and its next run draws from its own streams."""
    r = scenario("chain_lds", knobs)
    P, B = r["P"], r["B"]
    t = fresh(P, B, seed=SEED + 1, state=True)
    t.record_begin(1, 64)
    t.run_schedule(P["call1"], accumulate=True)
    was, waiting = snapshot(t), t.record_count()
    assert waiting > 0 and was["n_samples"] > 0
    t.load(r["blob"], what="state+tuning")
    now, want = snapshot(t), r["at_save"]
    for f in STATE_FIELDS + ("posterior", "tune"):
        assert np.array_equal(now[f], want[f]), f
    assert not now["accepted"].any() and not now["tried"].any()
    for f in ("age_sum", "age_sq", "n_samples"):
        assert np.array_equal(now[f], was[f]), f
    assert t.record_count() == waiting and t.iterations_done == len(P["call1"])
    t.record_fetch()
    ta, tk = t.run_schedule(P["call2"], trace=True)
    assert not np.array_equal(tk, r["a_trace"][1]) and np.isfinite(ta).any()
    with pytest.raises(ValueError):
        t.load(r["blob"], what="tuning")


def test_monitor_record_resumes_from_its_checkpoint(gpu, knobs, tmp_path):
    """monitor.record with a checkpoint behind every chunk: a run whose objects are dropped after chunk 2 and resumed from the file on fresh
    objects gives the samples of the uninterrupted run from chunk 3 on, at the same iteration numbers."""
    P = problem("12-leaves-variable-rate")
    path = str(tmp_path / "run.ckpt")
    whole = M.monitor.record(fresh(P, 3, state=True), 14, period=3, chunk=4)
    lost = M.monitor.record(fresh(P, 3, state=True), 8, period=3, chunk=4, checkpoint=path, every=1)
    assert os.path.exists(path) and not [f for f in os.listdir(tmp_path) if ".tmp." in f]
    del lost
    rest = M.monitor.record(fresh(P, 3), 6, period=3, chunk=4, resume=path)
    assert list(whole.iteration) == [3, 6, 9, 12] and list(rest.iteration) == [9, 12]
    for f in STATE_FIELDS + ("post", "beta"):
        assert np.array_equal(getattr(whole, f)[2:], getattr(rest, f)), f
