#!/usr/bin/env python3
"""MH proposal-steps per second of the lock-step driver (mcd_mh_*) on a golden dataset, next to the CPU twin
(oracle/mh_oracle.c, OpenMP over chains).  BASELINE.json configs[1]: tests/12-leaves-variable-rate, 64 chains.
One JSON line per chain count.  Usage: python tools/bench_mh.py [--name 12-leaves-variable-rate] [--chains 64,4096]
  --synthetic N_LEAVES[:sparse]   a synthetic tree instead (tools/bench_mh_large.py's problem; no CPU twin), the whole shuffled cycle
  --record PERIOD                 the same timed run three ways: unmonitored, with the device recorder at that period drained per chunk of
                                  256 iterations (the drain inside the timed region; monitor.record), and cut into calls of PERIOD iterations
                                  with a state read-back after each (monitor.collect)
  --summary WINDOW                after the timed runs, WINDOW samples are recorded (period 1, a short random schedule) and the node-age summary
                                  of that window is taken two ways on the same samples, each timed: (b) Sampler.record_summary, on the device
                                  in the ring (all quantities, with rhat and ess, lag cap 255); (a) record_fetch of the window +
                                  monitor.summarize_node_ages on the host (ages only).  (b) runs first: the fetch frees the slots.
  --mc3 C                         with --summary: the same window once more under Metropolis-coupled MCMC, groups of C chains (the default
                                  ladder, a swap phase behind every sample), the COLD sequences summarised three ways, each timed:
                                  Sampler.record_summary_mc3 on the device (gather + summary, lag cap 255); record_fetch of the window +
                                  diagnostics.rung_trace + diagnostics.summary on the host (the only route without it); and
                                  Sampler.record_summary of a run WITHOUT MC3 on chains / C chains and the same window -- the device
                                  summary of as many sequences without the gather
  --checkpoint                    after the timed runs: Sampler.save and Sampler.load (what="full", the blob back into the same handle), each once
                                  to warm up and then five times: checkpoint_bytes, checkpoint_save_ms and checkpoint_load_ms (medians) beside
                                  the line's other figures
  --repeat N                      the timed region N times (every value is printed; gpu_steps_per_s and gpu_us_per_lockstep are then the
                                  median of the N runs -- with the default N = 1 the one timed run, as before)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="12-leaves-variable-rate")
    ap.add_argument("--chains", default="64,4096")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--cpu-iters", type=int, default=20)
    ap.add_argument("--synthetic", default=None)
    ap.add_argument("--record", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--summary", type=int, default=0)
    ap.add_argument("--mc3", type=int, default=0)
    ap.add_argument("--checkpoint", action="store_true")
    args = ap.parse_args()
    import mcmc_date_amd as M

    def timed(f):
        t0 = time.perf_counter()
        f()
        return time.perf_counter() - t0

    def figures(smp, S, B, n_nodes, dataset, make=None):
        """the timed runs of one sampler: unmonitored, and with --record the recorded and the chopped loop beside it"""
        out = {"dataset": dataset, "chains": B, "n_nodes": n_nodes, "steps_per_iteration": S, "iterations": args.iters, "path": smp.last_path()}
        per_step = lambda dt: 1e6 * dt / (S * args.iters)
        out["gpu_us_per_lockstep_runs"] = [per_step(timed(lambda: smp.run(args.iters))) for _ in range(args.repeat)]
        if args.record > 0:
            from mcmc_date_amd import monitor

            rec = [timed(lambda: monitor.record(smp, args.iters, period=args.record, chunk=256)) for _ in range(args.repeat)]
            cut = [timed(lambda: monitor.collect(smp, args.iters, period=args.record)) for _ in range(args.repeat)]
            out.update({"record_period": args.record, "recorded_us_per_lockstep_runs": [per_step(x) for x in rec],
                        "chopped_us_per_lockstep_runs": [per_step(x) for x in cut],
                        "unmonitored_us_per_iteration": float(np.median(out["gpu_us_per_lockstep_runs"])) * S,
                        "recorded_us_per_iteration": 1e6 * float(np.median(rec)) / args.iters,
                        "chopped_us_per_iteration": 1e6 * float(np.median(cut)) / args.iters})
        if args.checkpoint:
            blob = smp.save()                                                        # (first call: code object load, staging allocation)
            smp.load(blob)
            t_save = [timed(smp.save) for _ in range(5)]
            t_load = [timed(lambda: smp.load(blob)) for _ in range(5)]
            out.update({"checkpoint_bytes": len(blob), "checkpoint_save_ms": 1e3 * float(np.median(t_save)), "checkpoint_load_ms": 1e3 * float(np.median(t_load)),
                        "checkpoint_save_ms_runs": [1e3 * x for x in t_save], "checkpoint_load_ms_runs": [1e3 * x for x in t_load]})
        if args.summary > 0:
            from mcmc_date_amd import monitor

            window = args.summary
            sched = np.random.default_rng(5).integers(0, len(smp.table), size=(window, 8)).astype(np.int32)   # 8 steps per sample: the run is not what is timed
            smp.record_begin(1, window)
            smp.run_schedule(sched)
            smp.record_summary(max_lag=1)                                            # (first call: code object load)
            got = []
            t_dev = [timed(lambda: got.append(smp.record_summary(max_lag=255))) for _ in range(max(args.repeat, 1))]
            fetched = []
            t_fetch = timed(lambda: fetched.append(smp.record_fetch()))
            it, sc, H = fetched[0][:3]
            host = []
            t_host = timed(lambda: host.append(monitor.summarize_node_ages((sc[:, :, 2][:, :, None] * H).reshape(-1, n_nodes), burn_in=0.0)))
            smp.record_end()
            same = bool(np.array_equal(got[-1].ages[:, 2:6], np.stack([host[0].minimum, host[0].maximum, host[0].ci_lower, host[0].ci_upper], axis=1)))
            out.update({"summary_window_samples": window, "summary_window_bytes": int(window * B * (2 * n_nodes + 9) * 8),
                        "summary_max_lag": got[-1].max_lag, "device_summary_s_runs": t_dev, "host_fetch_s": t_fetch, "host_summarize_s": t_host,
                        "host_total_s": t_fetch + t_host, "device_summary_s": float(np.median(t_dev)), "order_statistics_equal": same})
            if args.mc3 > 0:
                out.update(mc3_summary(smp, B, n_nodes, window, sched, make))
        return out

    def mc3_summary(smp, B, n_nodes, window, sched, make):
        """--mc3 C: the cold sequences of the same window three ways (module docstring)"""
        from mcmc_date_amd import diagnostics as D

        Cn, G = args.mc3, B // args.mc3
        reps = max(args.repeat, 1)
        plain = make(G)                                                              # no MC3, G chains: the summary without the gather
        plain.record_begin(1, window)
        plain.run_schedule(sched)
        plain.record_summary(max_lag=1)
        t_plain = [timed(lambda: plain.record_summary(max_lag=255)) for _ in range(reps)]
        plain.record_end()
        mc3 = M.MC3(smp, n_chains=Cn, swap_period=1, n_swaps=Cn - 1, seed=7)
        smp.record_begin(1, window)
        for k in range(window):                                                      # a swap phase behind every sample; not what is timed
            smp.run_schedule(sched[k:k + 1])
            mc3.swap()
        mc3.record_summary(max_lag=1)
        got = []
        t_dev = [timed(lambda: got.append(mc3.record_summary(max_lag=255, flow=True))) for _ in range(reps)]
        fetched, tr, host = [], [], []
        t_fetch = timed(lambda: fetched.append(smp.record_fetch()))
        it, sc, H, R, post, beta = fetched[0]

        def gather():
            x = np.concatenate([sc[:, :, 2][:, :, None] * H, R, sc, post, ((post[:, :, 0] + post[:, :, 1]) + post[:, :, 2])[:, :, None]], axis=2)
            tr.append(D.rung_trace(x, beta, 1.0, Cn))

        t_rung = timed(gather)
        t_host = timed(lambda: host.append(D.summary(tr[0][0], got[-1].max_lag, per_chain=False)))
        smp.record_end()
        same = bool(np.array_equal(got[-1].pooled[:, 2:6], host[0].pooled[:, 2:6], equal_nan=True) and np.array_equal(got[-1].holder, tr[0][1]))
        return {"mc3_summary_chains_per_group": Cn, "mc3_summary_groups": G, "mc3_summary_max_lag": got[-1].max_lag,
                "mc3_summary_device_s_runs": t_dev, "mc3_summary_device_s": float(np.median(t_dev)),
                "mc3_summary_host_fetch_s": t_fetch, "mc3_summary_host_rung_trace_s": t_rung, "mc3_summary_host_summarize_s": t_host,
                "mc3_summary_host_total_s": t_fetch + t_rung + t_host,
                "mc3_summary_plain_G_chains_device_s_runs": t_plain, "mc3_summary_plain_G_chains_device_s": float(np.median(t_plain)),
                "mc3_summary_cold_holder_changes": int((np.diff(got[-1].holder, axis=0) != 0).sum()),
                "mc3_summary_round_trips": int(got[-1].round_trips.sum()), "mc3_summary_order_statistics_and_holder_equal": same}

    if args.synthetic:
        from mcmc_date_amd import synthetic as SY

        n_leaves, _, form = args.synthetic.partition(":")
        topo = SY.random_topology(int(n_leaves), seed=3)
        n = topo.n_nodes - 2
        if form == "sparse":
            _, assoc = SY.banded_precision(n, seed=3)
            lik = M.SparseLikelihood(M.Sparse(np.random.default_rng(3).uniform(0.01, 0.2, n), assoc, 0.0)).bind_tree(topo)
        else:
            mu, sigma = SY.random_spd_problem(n, seed=3)
            lik = M.MvnLikelihood.from_covariance(mu, sigma).bind_tree(topo)
        pf = M.PriorFunction(1.0, "UncorrelatedGamma", [], [], [], topo)
        ps, _ = M.proposals(topo, [], calibrations_available=True)
        S = sum(p.weight for p in ps)
        for B in [int(x) for x in args.chains.split(",")]:
            s0 = SY.random_states(topo, B, seed=4)
            s0.time_birth_rate = np.full(B, 1.0); s0.time_death_rate = np.full(B, 0.8); s0.rate_variance = np.full(B, 0.3)
            def make(Bm, s0=s0):
                s = M.Sampler(lik, pf, ps, Bm, seed=13)
                s.set_state(s0.slice(0, Bm))
                return s

            smp = make(B)
            smp.run(2)
            smp.autotune()
            smp.run(1)
            r = figures(smp, S, B, topo.n_nodes, f"synthetic {n_leaves} leaves, {form or 'dense'}", make)
            r["gpu_us_per_lockstep"] = float(np.median(r["gpu_us_per_lockstep_runs"]))
            print(json.dumps({"metric": "MH lock step (us), synthetic tree", **r}), flush=True)
        return
    import oracle as O
    from test_gpu_mh import setup

    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", args.name + ".npz")))
    for B in [int(x) for x in args.chains.split(",")]:
        topo, ps, smp, twin = setup(fx, B=B, seed=1)
        S = sum(p.weight for p in ps)
        smp.run(20)
        smp.autotune()
        extra = figures(smp, S, B, topo.n_nodes, args.name, lambda Bm: setup(fx, B=Bm, seed=1)[2])
        dt = float(np.median(extra["gpu_us_per_lockstep_runs"])) * 1e-6 * S * args.iters
        rng = np.random.default_rng(0)
        twin.run(M.cycle_schedule(ps, 2, rng))
        t1 = time.perf_counter()
        twin.run(M.cycle_schedule(ps, args.cpu_iters, rng))
        dc = time.perf_counter() - t1
        print(json.dumps({"metric": "MH proposal steps/sec (chains x steps)", "dataset": args.name, "chains": B, "n_nodes": topo.n_nodes,
                          "steps_per_iteration": S, "gpu_steps_per_s": B * S * args.iters / dt, "gpu_us_per_lockstep": 1e6 * dt / (S * args.iters),
                          "cpu_twin_steps_per_s": B * S * args.cpu_iters / dc, "cpu_threads": os.cpu_count(),
                          **{k: v for k, v in extra.items() if k.endswith("_runs") or "checkpoint" in k or "record" in k or "summary" in k or k.startswith("host_") or k.startswith("order_") or k.endswith("_per_iteration") or k == "path"}}), flush=True)


if __name__ == "__main__":
    main()
