#!/usr/bin/env python
"""Device NUTS (mcd_hmc_nuts*) with and without its sample recorder: transitions per second of the SAME run -- same start states, step
sizes, masses and random streams -- three ways:
  unrecorded   one mcd_hmc_nuts_run of --transitions transitions, nothing kept;
  recorded     the same with the device recorder at --record PERIOD, drained once per chunk of 256 transitions, the drain inside the timed
               region (monitor.record_nuts);
  cut          one mcd_hmc_nuts per transition with a state read-back after each (mcd_hmc_get_state): what a caller who wants every sample
               had to do before the recorder (the read-back does not depend on PERIOD: a caller cannot know the state without it).
  --name NAME            a committed input (dense likelihood), Metropolis-Hastings burn-in for the start states
  --synthetic N_LEAVES   a random tree over a banded sparse precision matrix around the states' own distances (2 N_LEAVES - 1 nodes)
One JSON line per run; *_runs hold every repeat, the headline figures are their medians.

  --metric {diag,dense}  instead of the three ways above: warm-up from the problem's crude masses with that metric -- mcd_hmc_nuts_warmup (pooled
                         variances) or mcd_hmc_nuts_warmup_dense (the full covariance), --windows windows of --window transitions --, then
                         --transitions recorded transitions at the tuned step sizes: microseconds per leapfrog step (a lock step of all chains:
                         the transition's rounds are the longest tree's leaves), leapfrog steps per transition and chain, mean tree depth, the
                         tuned step sizes, and the smallest effective sample size over the inner node ages per leapfrog step
                         (Leapfrog.record_summary).
  --metric-form {per_chain,across_chains}   with --metric dense: how the dense metric's products are taken (Leapfrog.set_metric_form); the
                         line then carries the seconds the warm-up call spent in its four phases (factorisations, window covariance,
                         window buffer, transitions).
  --metric-factor {host,device}   with --metric dense: where the factors of every window's covariance are taken
                         (Leapfrog.set_metric_factor): the host's long double loops, or csrc/k_metric_factor.hip; reported beside the phases.

  --cycle {host,library}  instead: --transitions iterations of the reference's `--hamiltonian` mode (the Metropolis-Hastings cycle plus one
                         NUTS transition per iteration) on --name x --chains, from the same start states, step sizes and masses:
                         host      hmc.run_cycle_with_nuts -- the states cross the host twice per iteration between the two handles;
                         library   Sampler.attach_hamiltonian + Sampler.run -- mcd_mh_run with the attached handle, hand-overs on the device.
                         Milliseconds per iteration (median, every repeat, maximum - minimum of the repeats), mean tree depth and leapfrog
                         steps per transition.  The measurement runs in a child process under --limit seconds.

  --transition-form {rounds,one_launch}   how the leapfrog handle launches a transition (Leapfrog.set_transition_form): rounds of three
                         launches with a host poll each, or the whole transition as one launch (csrc/k_nuts_chain.hip; dense likelihoods
                         of up to 64 distances).  It applies to the plain run, --metric, --record and --cycle library (the attached
                         handle); the plain run's line carries milliseconds per transition (median and maximum - minimum of the
                         repeats), the mean tree depth and microseconds per leapfrog step (transition time / mean leapfrog steps)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mcmc_date_amd as M  # noqa: E402
from mcmc_date_amd import monitor  # noqa: E402


def golden_problem(name, B):
    topo, _, lf, eps, inv_mass = golden_setup(name, B)
    return topo, lf, eps, inv_mass, "dense"


def golden_setup(name, B):
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
    topo = M.Topology(fx["parent"])
    cal = [M.Calibration(f"c{i}", int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for i, r in enumerate(fx["cal"])]
    con = [M.Constraint(f"k{i}", int(r[0]), int(r[1]), r[2]) for i, r in enumerate(fx["con"])]
    br = [M.Brace(f"b{i}", [int(n) for n in fx["brace_nodes"][fx["brace_ptr"][i]:fx["brace_ptr"][i + 1]]], float(s)) for i, s in enumerate(fx["brace_sd"])]
    ht = float(fx["prior_ht"])
    pf = M.PriorFunction(ht, "UncorrelatedGamma", cal, con, br, topo)
    lik = M.MvnLikelihood(M.Full(fx["mu"], fx["sigma_inv"], float(fx["logdet"]))).bind_tree(topo)
    ps, _ = M.proposals(topo, br, calibrations_available=len(cal) > 0)
    smp = M.Sampler(lik, pf, ps, B, seed=3)
    x0 = M.init_with(topo, fx["mean_lengths"])
    if cal:
        x0.time_height = ht
    smp.set_initial_state(x0)
    smp.burn_in(fast=[10, 10, 20, 40], slow=[100, 100])
    lf = M.Leapfrog(lik, pf, len(cal) > 0, B)
    lf.set_state(smp.state())
    q0 = lf.position()[0]
    inv_mass = np.maximum((0.1 * np.abs(q0)).mean(axis=0) ** 2, 1e-12)
    eps, _, _, _ = lf.nuts_run(40, 0.05, inv_mass, adapt=True, max_depth=5, seed=1)
    return topo, smp, lf, eps, inv_mass


def cycle_report(args):
    """--cycle: the same iterations through the host round trip or through the attached handle."""
    B, T = args.chains, args.transitions
    topo, smp, lf, eps, inv_mass = golden_setup(args.name, B)
    start = smp.state()
    library = args.cycle == "library"
    lf.set_transition_form(args.transition_form)
    if library:
        smp.attach_hamiltonian(lf, eps, inv_mass, max_depth=args.max_depth)

    def go(n, first):
        if library:
            smp.run(n)
        else:
            M.run_cycle_with_nuts(smp, lf, None, n, eps, inv_mass, max_depth=args.max_depth, first_transition=first)
        smp.posterior()                                                # (waits for the sampler's stream)

    smp.set_state(start)
    go(2, 0)                                                           # (code objects, allocations)
    if library:
        smp.hamiltonian_stats(reset=True)
    runs = []
    for r in range(max(1, args.repeat)):
        smp.set_state(start)
        t0 = time.perf_counter()
        go(T, 1000 * (r + 1))
        runs.append(1e3 * (time.perf_counter() - t0) / T)
    if library:
        st = smp.hamiltonian_stats()
        n = max(1, st["transitions"])
        depth, leaves, divergent = float(st["depth_sum"].mean()) / n, float(st["leapfrog_steps"].mean()) / n, int(st["divergent"].sum())
    else:                                                              # one more pass, untimed, with the NUTS driver's recorder on
        smp.set_state(start)
        lf.record_begin(period=1, capacity=T)
        go(T, 1000)
        nuts = lf.record_fetch()[-1]
        lf.record_end()
        depth, leaves, divergent = float(nuts[:, :, 0].mean()), float(nuts[:, :, 1].mean()), int(nuts[:, :, 3].sum())
    print(json.dumps({"metric": "Metropolis-Hastings cycle + one NUTS transition per iteration", "cycle": args.cycle, "dataset": args.name,
                      "n_nodes": topo.n_nodes, "chains": B, "iterations": T, "steps_per_iteration": int(sum(p.weight for p in smp.table)),
                      "max_depth": args.max_depth, "transition_form": lf.transition_form, "path": smp.last_path(), "ms_per_iteration": float(np.median(runs)), "ms_per_iteration_runs": runs,
                      "spread_ms": max(runs) - min(runs), "mean_depth": depth, "leapfrog_steps_per_transition": leaves, "divergent": divergent}),
          flush=True)


def synthetic_problem(n_leaves, B):
    import oracle as O
    from mcmc_date_amd import synthetic as S

    topo = S.random_topology(n_leaves, seed=5)
    n = topo.n_nodes - 2
    _, assoc = S.banded_precision(n, seed=5)
    st0 = S.random_states(topo, 1, seed=7)
    mu = O.distances(topo.parent, st0.heights[0], st0.rates[0], st0.time_height[0], st0.rate_mean[0])
    lik = M.SparseLikelihood(M.Sparse(mu, assoc, 0.0)).bind_tree(topo)
    pf = M.PriorFunction(1.0, "UncorrelatedGamma", [], [], [], topo)
    st = S.random_states(topo, B, seed=7, jitter=0.002)
    rng = np.random.default_rng(12)
    full = M.StateBatch(st.heights, st.rates, st.time_height, st.rate_mean, np.exp(0.1 * rng.standard_normal(B)), np.exp(0.1 * rng.standard_normal(B)),
                        0.5 + 0.2 * rng.random(B))
    lf = M.Leapfrog(lik, pf, False, B)
    lf.set_state(full)
    q0, _, g0 = lf.position()
    # masses from the positions' own scales, step sizes from the gradient in those scales (tests/test_gpu_sparse_hmc.py)
    inv_mass = np.maximum((0.1 * np.abs(q0)).mean(axis=0) ** 2, 1e-60)
    eps = 1e-2 / np.maximum(1.0, (np.abs(g0) * np.sqrt(inv_mass)).max(axis=1))
    return topo, lf, eps, inv_mass, "sparse"


def metric_report(args, topo, lf, eps0, inv_mass0, form):
    B, T = lf.batch, args.transitions
    dense = args.metric == "dense"
    kw = dict(max_depth=args.max_depth, seed=args.seed)
    t0 = time.perf_counter()
    if dense:
        lf.set_metric_form(args.metric_form)
        lf.set_metric_factor(args.metric_factor)
        eps, _, alpha_w = lf.nuts_warmup_dense(eps0, inv_mass0, windows=args.windows, window=args.window, **kw)
        inv_mass = None
    else:
        eps, inv_mass, alpha_w = lf.nuts_warmup(eps0, inv_mass0, windows=args.windows, window=args.window, **kw)
    warm_s = time.perf_counter() - t0
    phases = None
    if dense:                                                      # the library's own clock over the call's four phases (hmc_capi.cpp)
        buf = (ctypes.c_double * 4)()
        hook = ctypes.CDLL(M._capi.LIB_PATH).mcd_hmc_warmup_phases_
        hook.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        M._capi.check(hook(lf._h, buf))
        phases = dict(zip(("factorisations_s", "covariance_s", "window_buffer_s", "transitions_s"), buf))
    first = (args.windows + 1) * args.window
    lf.record_begin(period=1, capacity=T)
    lf.position()
    t0 = time.perf_counter()
    _, alpha, _, _ = lf.nuts_run(T, eps, inv_mass, adapt=False, first_transition=first, **kw)
    lf.position()                                                  # (waits for the handle's stream)
    run_s = time.perf_counter() - t0
    summ = lf.record_summary(max_lag=min(255, max(1, T // 2)))
    nuts = lf.record_fetch()[-1]                                   # [T, B, 6] = Leapfrog.NUTS_FIELDS
    lf.record_end()
    steps = nuts[:, :, 1]
    lock_steps = float(steps.max(axis=1).sum())
    inner = np.flatnonzero(~topo.leaves)
    ess = summ.ages[inner, 7]
    print(json.dumps({"metric": "NUTS leapfrog steps (all chains in lock step)", "mass_matrix": args.metric,
                      "metric_form": args.metric_form if dense else None, "warmup_phases": phases,
                      "metric_factor": args.metric_factor if dense else None, "transition_form": lf.transition_form,
                      "dataset": f"synthetic {args.synthetic} leaves" if args.synthetic else args.name, "likelihood": form, "n_nodes": topo.n_nodes,
                      "dim": lf.dim, "chains": B, "windows": args.windows, "window": args.window, "transitions": T, "max_depth": args.max_depth,
                      "warmup_s": warm_s, "warmup_mean_alpha": float(alpha_w.mean()), "eps_mean": float(eps.mean()), "eps_min": float(eps.min()),
                      "eps_max": float(eps.max()), "run_s": run_s, "us_per_leapfrog_step": 1e6 * run_s / max(1.0, lock_steps),
                      "leapfrog_steps_per_transition": float(steps.mean()), "mean_depth": float(nuts[:, :, 0].mean()),
                      "divergent": int(nuts[:, :, 3].sum()), "mean_alpha": float(alpha.mean()), "min_ess_node_ages": float(ess.min()),
                      "min_ess_per_leapfrog_step": float(ess.min()) / max(1.0, float(steps.sum()))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="24-leaves-braces")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--transitions", type=int, default=60)
    ap.add_argument("--max-depth", type=int, default=5)
    ap.add_argument("--record", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--metric", choices=("diag", "dense"), default=None)
    ap.add_argument("--metric-form", choices=("per_chain", "across_chains"), default="per_chain")
    ap.add_argument("--metric-factor", choices=("host", "device"), default="host")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window", type=int, default=60)
    ap.add_argument("--cycle", choices=("host", "library"), default=None)
    ap.add_argument("--transition-form", choices=("rounds", "one_launch"), default="rounds")
    ap.add_argument("--limit", type=int, default=300, help="seconds the child process of --cycle may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cycle and not args.child:                                   # the measurement in a child of its own, under its own time limit
        if args.synthetic:
            ap.error("--cycle runs on a committed input (--name)")
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"cycle": args.cycle, "error": f"time limit of {args.limit} s"}), flush=True)
            return 124
    if args.cycle:
        return cycle_report(args)
    if args.metric_form != "per_chain" and args.metric != "dense":
        ap.error("--metric-form is valid with --metric dense")
    if args.metric_factor != "host" and args.metric != "dense":
        ap.error("--metric-factor is valid with --metric dense")
    B, T = args.chains, args.transitions
    topo, lf, eps, inv_mass, form = synthetic_problem(args.synthetic, B) if args.synthetic else golden_problem(args.name, B)
    lf.set_transition_form(args.transition_form)
    if args.metric:
        return metric_report(args, topo, lf, eps, inv_mass, form)
    start = lf.state()
    kw = dict(max_depth=args.max_depth, seed=args.seed)

    def timed(fn):
        lf.set_state(start)
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def cut():
        for t in range(T):
            lf.nuts(eps, inv_mass, transition=t, **kw)
            lf.state()

    timed(lambda: lf.nuts_run(2, eps, inv_mass, adapt=False, **kw))                     # (code objects, allocations)
    runs = {"unrecorded": [], "recorded": [], "cut": []}
    ends = {}
    for _ in range(max(1, args.repeat)):
        runs["unrecorded"].append(timed(lambda: lf.nuts_run(T, eps, inv_mass, adapt=False, **kw)))
        ends["unrecorded"] = lf.state()
        runs["recorded"].append(timed(lambda: monitor.record_nuts(lf, T, eps, inv_mass, period=args.record, chunk=256, **kw)))
        ends["recorded"] = lf.state()
        runs["cut"].append(timed(cut))
        ends["cut"] = lf.state()
    lf.set_state(start)                                                # one more pass, untimed, for the trees' sizes
    # (monitor.record_nuts above ends its own recording before it returns, so no recorder is active here)
    lf.record_begin(period=1, capacity=T)
    lf.nuts_run(T, eps, inv_mass, adapt=False, **kw)
    nuts = lf.record_fetch()[-1]                                       # [T, B, 6] = Leapfrog.NUTS_FIELDS
    lf.record_end()
    ms = [1e3 * v / T for v in runs["unrecorded"]]
    steps = float(nuts[:, :, 1].mean())
    same = all(np.array_equal(ends["unrecorded"].heights, ends[k].heights) and np.array_equal(ends["unrecorded"].rates, ends[k].rates) for k in ends)
    rate = {k: T / float(np.median(v)) for k, v in runs.items()}
    spread = {k: (max(v) - min(v)) / float(np.median(v)) for k, v in runs.items()}
    print(json.dumps({"metric": "NUTS transitions/s (all chains in lock step)", "dataset": f"synthetic {args.synthetic} leaves" if args.synthetic else args.name,
                      "likelihood": form, "n_nodes": topo.n_nodes, "chains": B, "transitions": T, "max_depth": args.max_depth, "record_period": args.record,
                      "transition_form": lf.transition_form, "ms_per_transition": float(np.median(ms)), "ms_per_transition_runs": ms,
                      "spread_ms": max(ms) - min(ms), "mean_depth": float(nuts[:, :, 0].mean()), "leapfrog_steps_per_transition": steps,
                      "us_per_leapfrog_step": 1e3 * float(np.median(ms)) / max(1.0, steps),
                      "unrecorded_transitions_per_s": rate["unrecorded"], "recorded_transitions_per_s": rate["recorded"],
                      "cut_transitions_per_s": rate["cut"], "recorded_over_cut": rate["recorded"] / rate["cut"],
                      "recorded_over_unrecorded": rate["recorded"] / rate["unrecorded"], "same_end_state": bool(same),
                      "relative_spread": spread, **{k + "_s_runs": v for k, v in runs.items()}}), flush=True)


if __name__ == "__main__":
    sys.exit(main())
