"""Monitors and node-age summaries of the batched sampler (reporting part).

Host-side mirror of
  * the monitor files of app/Definitions.hs:288-417 -- `params` (the five scalars, calibrated node ages, constrained
    node age differences, brace variances), `timetree` (absolute time tree), `ratetree`, `prior` (the three prior
    blocks), all with period 2 -- written per chain in the tab-separated layout of `mcmc`'s file monitors
    (first column `Iteration`);
  * the node-age summary of scripts/trees-monitor-summary-ultrametric:149-175: after dropping round(l * burn-in)
    samples, per node the mean, the maximum-likelihood variance, minimum, maximum and the 95 % interval taken from
    the sorted ages as slice(floor(0.025 l), floor(0.95 l)).

The states come from the device sampler -- `record`: kept on the device while it runs (mcd_mh_record_*) and fetched once per
chunk of iterations (`record_nuts`: the same for the NUTS driver, mcd_hmc_record_*); `collect`: `Sampler.state()` after every run of
`period` iterations --; nothing here computes a
likelihood or a prior on the host -- the prior blocks are evaluated by the device prior (`PriorFunction.logprior`).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from .prepare import to_newick
from .state import StateBatch
from .tree import Topology, height_tree_to_length_tree

PERIOD = 2   # every monitor file of the reference uses period 2 (app/Definitions.hs:358, 369, 372, 389)


@dataclass
class Trace:
    """Sampled states of all chains: arrays [n_samples, B, ...]; `iteration[k]` is the iteration of sample k."""
    iteration: np.ndarray
    time_birth_rate: np.ndarray
    time_death_rate: np.ndarray
    time_height: np.ndarray
    heights: np.ndarray
    rate_mean: np.ndarray
    rate_variance: np.ndarray
    rates: np.ndarray
    post: Optional[np.ndarray] = None    # [n_samples, B, 3] ln prior, ln likelihood, ln jacobianRootBranch (`record` only)
    beta: Optional[np.ndarray] = None    # [n_samples, B] reciprocal temperature of the chain when the sample was taken (`record` only)
    nuts: Optional[np.ndarray] = None    # [n_samples, B, 6] hmc.Leapfrog.NUTS_FIELDS of the transition behind the sample (`record_nuts` only)

    def ages(self) -> np.ndarray:
        """Absolute node ages tH * h_v, [n_samples, B, n_nodes] (getTimeTreeNodeHeight, app/Definitions.hs:300-304)."""
        return self.time_height[:, :, None] * self.heights

    def states(self, k: int) -> StateBatch:
        return StateBatch(self.heights[k], self.rates[k], self.time_height[k], self.rate_mean[k], self.time_birth_rate[k],
                          self.time_death_rate[k], self.rate_variance[k])


def collect(sampler, n_iter: int, period: int = PERIOD, accumulate: bool = False) -> Trace:
    """Advance the sampler by n_iter iterations and keep the state of every chain every `period` iterations."""
    cols: List[List[np.ndarray]] = [[] for _ in range(7)]
    its = []
    done = 0
    while done + period <= n_iter:
        sampler.run(period, accumulate=accumulate)
        done += period
        s = sampler.state()
        for col, a in zip(cols, (s.time_birth_rate, s.time_death_rate, s.time_height, s.heights, s.rate_mean, s.rate_variance, s.rates)):
            col.append(a)
        its.append(sampler.iterations_done)
    if done < n_iter:
        sampler.run(n_iter - done, accumulate=accumulate)
    st = [np.stack(c) if c else np.empty((0,)) for c in cols]
    return Trace(np.asarray(its, np.int64), *st)


def _record_chunks(driver, total: int, period: int, chunk: int, run, begun=None, fetched=None):
    """The loop of `record` and `record_nuts`: the driver's recorder holds what one chunk can add at most; run(k, done) advances the driver
    by the next k of `total` steps (`done` are behind it), one fetch per chunk.  begun(): called once behind record_begin; fetched(i): behind
    the fetch of chunk i (1, 2, ...), when the ring is empty.  Returns the six arrays of the fetches, concatenated, or None when nothing was
    recorded."""
    parts: List[tuple] = []
    driver.record_begin(period, (chunk + period - 1) // period)
    try:
        if begun is not None:
            begun()
        done = 0
        while done < total:
            k = min(chunk, total - done)
            run(k, done)
            done += k
            parts.append(driver.record_fetch())
            if fetched is not None:
                fetched(len(parts))
    finally:
        driver.record_end()
    if sum(len(p[0]) for p in parts) == 0:
        return None
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(6))


def record(sampler, n_iter: int, period: int = PERIOD, accumulate: bool = False, chunk: int = 256, checkpoint: Optional[str] = None,
           every: int = 1, resume: Optional[str] = None) -> Trace:
    """`collect` without cutting the run into pieces of one monitor period: the sampler's recorder keeps the samples on the device
    while `chunk` iterations run in one call, and they are fetched once per chunk.  The same samples at the same iterations as
    `collect` (the chains do not depend on how a run is cut, up to the rounding of the incremental likelihood, which every call
    restarts from a full product), with the posterior terms and the temperatures beside them.
    checkpoint: a file that `Sampler.checkpoint` rewrites behind the fetch of every `every`-th chunk, when the ring is empty -- a run that
    loses its process goes on from there: resume = that file, on a fresh sampler over the same configuration, with the same period and chunk
    and n_iter the iterations still to run, gives the samples the lost run would have given from the next chunk on, bit for bit, at the
    same iteration numbers (the recorder's period phase, the cycle's generator and the iteration count are in the file)."""
    if n_iter < 0 or period < 1 or chunk < 1 or every < 1:
        raise ValueError("record: need n_iter >= 0, period >= 1, chunk >= 1, every >= 1")
    base = [sampler.iterations_done]

    def begun():
        if resume is not None:                      # behind record_begin: the load continues the recorder's counts
            meta = sampler.restore(resume)
            base[0] = sampler.iterations_done - meta["rec_iter"]

    def fetched(i):
        if checkpoint is not None and i % every == 0:
            sampler.checkpoint(checkpoint)

    got = _record_chunks(sampler, n_iter, period, chunk, lambda k, done: sampler.run(k, accumulate=accumulate, chunk=k), begun, fetched)
    base = base[0]
    if got is None:
        e = np.empty((0,))
        return Trace(np.empty(0, np.int64), e, e, e, e, e, e, e, e, e)
    it, sc, H, R, post, beta = got
    return Trace(base + it, sc[..., 0], sc[..., 1], sc[..., 2], H, sc[..., 3], sc[..., 4], R, post, beta)


def record_nuts(lf, n_transitions: int, eps, inv_mass, period: int = PERIOD, chunk: int = 256, max_depth: int = 8, seed: int = 0,
                first_transition: int = 0, chain_offset: int = 0) -> Trace:
    """`record` for the NUTS driver (hmc.Leapfrog; runs with `--hamiltonian`): n_transitions transitions at fixed step sizes and masses in
    calls of up to `chunk` transitions (Leapfrog.nuts_run), the recorder keeping every `period`-th state on the device with the
    transition's diagnostics (Trace.nuts), one fetch per chunk.  `iteration` counts the transitions of the random streams
    (first_transition + ...), so a trace continues where the last one ended.  The trace feeds write_monitor_files as any other; for a
    summary without a fetch call summarize_recorded(lf) between lf.record_begin and lf.record_end instead."""
    if n_transitions < 0 or period < 1 or chunk < 1:
        raise ValueError("record_nuts: need n_transitions >= 0, period >= 1, chunk >= 1")
    got = _record_chunks(lf, n_transitions, period, chunk,
                         lambda k, done: lf.nuts_run(k, eps, inv_mass, adapt=False, max_depth=max_depth, seed=seed,
                                                     first_transition=first_transition + done, chain_offset=chain_offset))
    if got is None:
        e = np.empty((0,))
        return Trace(np.empty(0, np.int64), e, e, e, e, e, e, e, e, None, e)
    it, sc, H, R, post, nuts = got
    return Trace(first_transition + it, sc[..., 0], sc[..., 1], sc[..., 2], H, sc[..., 3], sc[..., 4], R, post, None, nuts)


def prior_components(prior, trace: Trace, piece: int = 1 << 16) -> np.ndarray:
    """The three prior blocks (node priors, birth-death, clock) of ALL samples of all chains, [n_samples, B, 3], by batched
    evaluations of the device prior over samples x chains (at most `piece` states per call) instead of one per sample and chain."""
    n, B = trace.heights.shape[:2]
    flat = StateBatch(trace.heights.reshape(n * B, -1), trace.rates.reshape(n * B, -1), trace.time_height.reshape(-1), trace.rate_mean.reshape(-1),
                      trace.time_birth_rate.reshape(-1), trace.time_death_rate.reshape(-1), trace.rate_variance.reshape(-1))
    out = np.empty((n * B, 3))
    for lo in range(0, n * B, piece):
        hi = min(n * B, lo + piece)
        out[lo:hi] = prior.logprior(flat.slice(lo, hi), want_components=True)[1]
    return out.reshape(n, B, 3)


# ---- monitor files ---------------------------------------------------------------------------------------------------
def _fmt(x: float) -> str:
    return repr(float(x))


def write_monitor_files(prefix: str, trace: Trace, chain: int, topo: Topology, calibrations: Sequence = (), constraints: Sequence = (),
                        braces: Sequence = (), prior=None, components: Optional[np.ndarray] = None) -> List[str]:
    """Write <prefix>.params.monitor, .timetree.monitor, .ratetree.monitor (and .prior.monitor when the device prior
    `prior` is given, or its blocks `components` = prior_components(prior, trace), which saves the evaluation per sample) for
    one chain.  Returns the file names."""
    files = []
    ages = trace.ages()[:, chain, :]
    names = (["TimeBirthRate", "TimeDeathRate", "TimeHeight", "RateMean", "RateVariance"]
             + [f"Calibration {c.name} ({c.lower if c.lower is not None else 0.0},{c.upper if c.upper is not None else 'Infinity'})" for c in calibrations]
             + [f"Constraint {k.name}" for k in constraints] + [f"Brace {b.name} variance" for b in braces])
    fn = prefix + ".params.monitor"
    with open(fn, "w") as f:
        f.write("\t".join(["Iteration"] + names) + "\n")
        for k, it in enumerate(trace.iteration):
            row = [trace.time_birth_rate[k, chain], trace.time_death_rate[k, chain], trace.time_height[k, chain], trace.rate_mean[k, chain],
                   trace.rate_variance[k, chain]]
            row += [ages[k, c.node] for c in calibrations]
            row += [ages[k, c.old] - ages[k, c.young] for c in constraints]                 # getTimeTreeDeltaNodeHeight, :321-322
            row += [float(np.var(ages[k, list(b.nodes)], ddof=1)) for b in braces]           # S.variance (unbiased), :335-339
            f.write("\t".join([str(int(it))] + [_fmt(x) for x in row]) + "\n")
    files.append(fn)
    for tag, col in (("timetree", "TimeTree"), ("ratetree", "RateTree")):
        fn = f"{prefix}.{tag}.monitor"
        with open(fn, "w") as f:
            f.write(f"Iteration\t{col}\n")
            for k, it in enumerate(trace.iteration):
                if tag == "timetree":     # absoluteTimeTree: heightTreeToLengthTree scaled by the time height, :360-364
                    lengths = height_tree_to_length_tree(topo, trace.heights[k, chain]) * trace.time_height[k, chain]
                else:
                    lengths = trace.rates[k, chain]
                f.write(f"{int(it)}\t{to_newick(topo, lengths)}\n")
        files.append(fn)
    if components is not None:
        fn = prefix + ".prior.monitor"
        with open(fn, "w") as f:
            f.write("Iteration\tPriorCsKsBs\tPriorBirthDeath\tPriorRelaxedMolecularClock\n")
            for k, it in enumerate(trace.iteration):
                f.write("\t".join([str(int(it))] + [_fmt(x) for x in components[k, chain]]) + "\n")
        files.append(fn)
    elif prior is not None:
        fn = prefix + ".prior.monitor"
        with open(fn, "w") as f:
            f.write("Iteration\tPriorCsKsBs\tPriorBirthDeath\tPriorRelaxedMolecularClock\n")
            for k, it in enumerate(trace.iteration):
                _, comp = prior.logprior(trace.states(k).slice(chain, chain + 1), want_components=True)
                f.write("\t".join([str(int(it))] + [_fmt(x) for x in comp[0]]) + "\n")
        files.append(fn)
    return files


# ---- node-age summary -- scripts/trees-monitor-summary-ultrametric:149-175, 222-255 --------------------------------------
SUMMARY_HEADER = "Index\tName\tMean\tVariance\tMin\tMax\t95CILower\t95CIUpper"


@dataclass
class AgeSummary:
    index: np.ndarray
    name: List[str]
    mean: np.ndarray
    variance: np.ndarray
    minimum: np.ndarray
    maximum: np.ndarray
    ci_lower: np.ndarray
    ci_upper: np.ndarray
    rhat: Optional[np.ndarray] = None      # split R-hat and effective sample size per node (summarize_recorded only)
    ess: Optional[np.ndarray] = None

    def render(self) -> str:
        rows = [SUMMARY_HEADER]
        for i in range(len(self.index)):
            rows.append("\t".join([str(int(self.index[i])), self.name[i]] + [_fmt(x) for x in (self.mean[i], self.variance[i], self.minimum[i],
                                                                                              self.maximum[i], self.ci_lower[i], self.ci_upper[i])]))
        return "\n".join(rows) + "\n"


def summarize_node_ages(ages: np.ndarray, burn_in: float = 0.25, names: Optional[Sequence[str]] = None) -> AgeSummary:
    """ages: [n_samples, n_nodes] of one chain (or of pooled chains, samples along axis 0).  The first
    round(n_samples * burn_in) samples are dropped (`scripts/analyze` passes 0.25 after its own thinning)."""
    a = np.asarray(ages, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("summarize_node_ages: expected [n_samples, n_nodes]")
    l0 = a.shape[0]
    a = a[int(round(l0 * burn_in)):]
    l = a.shape[0]
    if l == 0:
        raise ValueError("summarize_node_ages: no samples left after burn-in")
    mean = a.mean(axis=0)
    var = a.var(axis=0)                                   # statistics' meanVariance: maximum-likelihood estimate
    srt = np.sort(a, axis=0)
    i_ci = int(math.floor(l * 0.025))
    n_ci = int(math.floor(l * 0.95))
    if n_ci < 1:
        raise ValueError("summarize_node_ages: too few samples for the 95 % interval")
    n = a.shape[1]
    return AgeSummary(np.arange(n), list(names) if names is not None else [""] * n, mean, var, srt[0], srt[-1], srt[i_ci], srt[i_ci + n_ci - 1])


def summarize_recorded(sampler, burn_in: float = 0.25, names: Optional[Sequence[str]] = None, max_lag: int = 255,
                       rung: Optional[int] = None) -> AgeSummary:
    """`summarize_node_ages` of the pooled ages of the samples waiting in the sampler's recorder, after dropping the oldest
    round(waiting * burn_in) of them -- computed on the device where the samples lie (Sampler.record_summary): nothing is fetched and the
    samples stay where they are.  Also gives the split R-hat and the effective sample size of every node's age over the chains.
    `sampler`: a Sampler or an hmc.Leapfrog with an active recorder (both have record_count / record_summary).
    rung: for a Sampler under Metropolis-coupled MCMC, the rung of the ladder whose sequences are pooled (0: the cold ones, what the
    reference's monitors report; Sampler.record_summary_mc3) -- the chains themselves change temperature and are refused."""
    waiting = sampler.record_count()
    skip = int(round(waiting * burn_in))
    if skip >= waiting:
        raise ValueError("summarize_recorded: no samples left after burn-in")
    if rung is None:
        a = sampler.record_summary(skip=skip, max_lag=max_lag).ages
    else:
        a = sampler.record_summary_mc3(rung=rung, skip=skip, max_lag=max_lag).ages
    n = a.shape[0]
    return AgeSummary(np.arange(n), list(names) if names is not None else [""] * n, a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(),
                      a[:, 4].copy(), a[:, 5].copy(), a[:, 6].copy(), a[:, 7].copy())
