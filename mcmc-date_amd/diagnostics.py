"""Posterior summaries and convergence diagnostics of a trace x[n samples, B chains, Q quantities].

Three things live here:
  * a plain-numpy restatement of the definitions of include/mcmcdate_mvn.h (mcd_trace_summary) -- `split_rhat`, `ess`, `summary` --: the host
    mirror of csrc/k_summary.hip and the reference of its tests;
  * `trace_summary`: the same numbers from the device kernels, through the C ABI;
  * `power_posterior_points`, `marginal_likelihood`, `marginal_likelihood_device`: the marginal likelihood from power-posterior chains --
    the path points, the numpy restatement of mcd_ml_estimate (csrc/k_marginal.hip) and the kernels through the C ABI;
  * `rung_trace`, `replica_flow`: under Metropolis-coupled MCMC, the sequence of one temperature through the swaps and how the chains travel
    over the ladder -- the restatement of csrc/k_mc3_summary.hip (Sampler.record_summary_mc3).

Definitions, with l = n B pooled values per quantity:
  mean, variance (maximum likelihood, / l), minimum, maximum, and the two order statistics of monitor.summarize_node_ages,
  sorted[i] and sorted[i + m - 1] with i = floor(0.025 l), m = floor(0.95 l);
  split R-hat (Gelman et al., BDA3 11.4; Vehtari et al. 2021): the oldest sample is dropped if n is odd, every chain is halved into
  M = 2 B sequences of n_h = n // 2 samples; W = mean of their unbiased variances, Bv = n_h x unbiased variance of their means,
  var+ = (n_h - 1) / n_h W + Bv / n_h, rhat = sqrt(var+ / W);
  effective sample size on the same sequences: gamma_{m,t} = 1 / n_h sum_i (x_i - mean_m)(x_{i+t} - mean_m),
  rho_t = 1 - (W - mean_m gamma_{m,t}) / var+, P_k = rho_{2k} + rho_{2k+1}; tau = -1 + 2 sum_k min(P_k, P_{k-1}) while P_k > 0 and
  2 k + 1 <= max_lag (Geyer's initial monotone sequence); tau = max(tau, 1 / log10(M n_h)); ess = M n_h / tau.
A constant sequence has the variance 0 exactly.  W = 0, var+ = 0 or n_h < 2: rhat = ess = NaN.  A NaN anywhere in a quantity makes every output of that quantity NaN.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _capi
from ._arrays import dp, reduction_source

COLUMNS = ("mean", "variance", "minimum", "maximum", "ci_lower", "ci_upper", "rhat", "ess", "last_lag")


def _split(x: np.ndarray) -> np.ndarray:
    """[n, B, ...] -> the split sequences [n_h, 2 B, ...]; sequence 2 b + h is half h of chain b."""
    n = x.shape[0]
    nh = n // 2
    x = x[n - 2 * nh:]
    halves = np.stack([x[:nh], x[nh:]], axis=2)                       # [n_h, B, 2, ...]
    return halves.reshape((nh, 2 * x.shape[1]) + x.shape[2:])


def _var(x: np.ndarray, ddof: int) -> np.ndarray:
    """Variance along axis 0; a constant sequence has the variance 0 exactly, whatever the rounding of its mean."""
    return np.where(x.max(axis=0) == x.min(axis=0), 0.0, x.var(axis=0, ddof=ddof))


def _w_varp(seq: np.ndarray):
    nh = seq.shape[0]
    means = seq.mean(axis=0)
    w = _var(seq, 1).mean(axis=0)
    bv = nh * means.var(axis=0, ddof=1)
    return means, w, (nh - 1) / nh * w + bv / nh


def _degenerate(w, varp):
    return ~np.isfinite(w) | ~np.isfinite(varp) | (w == 0) | (varp == 0)


def split_rhat(x: np.ndarray) -> np.ndarray:
    """x [n, B] or [n, B, Q] -> rhat (scalar array or [Q])."""
    x = np.asarray(x, dtype=np.float64)
    shape = x.shape[2:]
    if x.shape[0] // 2 < 2:
        return np.full(shape, np.nan)
    with np.errstate(all="ignore"):
        _, w, varp = _w_varp(_split(x))
        r = np.sqrt(varp / w)
    return np.where(_degenerate(w, varp), np.nan, r)


def ess(x: np.ndarray, max_lag: int, details: bool = False):
    """x [n, B] or [n, B, Q] -> ess; details: (ess, last lag that entered the sum (-1: none), smallest |P_k| examined)."""
    x = np.asarray(x, dtype=np.float64)
    flat = x.reshape(x.shape[0], x.shape[1], -1)
    Q = flat.shape[2]
    nh = flat.shape[0] // 2
    out, last, pmin = np.full(Q, np.nan), np.full(Q, np.nan), np.full(Q, np.inf)
    if max_lag % 2 != 1 or not 1 <= max_lag <= nh - 1:
        raise ValueError("ess: max_lag must be odd and 1 <= max_lag <= n // 2 - 1")
    seq = _split(flat)
    M = seq.shape[1]
    with np.errstate(all="ignore"):
        means, w, varp = _w_varp(seq)
        c = seq - means
        g = np.stack([(c[:nh - t] * c[t:]).sum(axis=0).mean(axis=0) / nh for t in range(max_lag + 1)])     # [lags, Q]
        rho = 1.0 - (w - g) / varp
    bad = _degenerate(w, varp)
    for q in range(Q):
        if bad[q]:
            continue
        tau, prev, lag = -1.0, math.inf, -1.0
        k = 0
        while 2 * k + 1 <= max_lag:
            p = rho[2 * k, q] + rho[2 * k + 1, q]
            pmin[q] = min(pmin[q], abs(p))
            if not p > 0:
                break
            p = min(p, prev)
            tau += 2.0 * p
            prev = p
            lag = 2.0 * k + 1
            k += 1
        tau = max(tau, 1.0 / math.log10(M * nh))
        out[q] = M * nh / tau
        last[q] = lag
    shape = x.shape[2:]
    if details:
        return out.reshape(shape), last.reshape(shape), pmin.reshape(shape)
    return out.reshape(shape)


@dataclass
class Summary:
    """pooled [Q, 9] in the order of COLUMNS; per_chain [B, Q, 4] = mean, unbiased variance, minimum, maximum (or None);
    min_abs_p [Q]: the smallest |P_k| the effective sample size examined (host mirror only: how close a stop of Geyer's rule was)."""
    pooled: np.ndarray
    per_chain: Optional[np.ndarray] = None
    min_abs_p: Optional[np.ndarray] = None

    def __getattr__(self, name):
        if name in COLUMNS:
            return self.pooled[..., COLUMNS.index(name)]
        raise AttributeError(name)


def summary(x: np.ndarray, max_lag: int = 0, per_chain: bool = True) -> Summary:
    """The host restatement of mcd_trace_summary on x [n, B, Q]."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("summary: expected [n, B, Q]")
    n, B, Q = x.shape
    l = n * B
    i_ci, n_ci = int(math.floor(l * 0.025)), int(math.floor(l * 0.95))
    if n_ci < 1:
        raise ValueError("summary: too few samples for the 95 % interval")
    pooled = np.full((Q, len(COLUMNS)), np.nan)
    flat = x.reshape(l, Q)
    nan = np.isnan(flat).any(axis=0)
    with np.errstate(all="ignore"):
        srt = np.sort(flat, axis=0)
        pooled[:, 0] = flat.mean(axis=0)
        pooled[:, 1] = flat.var(axis=0)
        pooled[:, 2], pooled[:, 3], pooled[:, 4], pooled[:, 5] = srt[0], srt[-1], srt[i_ci], srt[i_ci + n_ci - 1]
        pooled[:, 6] = split_rhat(x)
        pmin = np.full(Q, np.inf)
        if max_lag and n // 2 >= 2:
            pooled[:, 7], pooled[:, 8], pmin = ess(x, max_lag, details=True)
        pc = None
        if per_chain:
            pc = np.stack([x.mean(axis=0), _var(x, 1) if n > 1 else np.full((B, Q), np.nan), x.min(axis=0), x.max(axis=0)], axis=2)
            pc[:, nan, :] = np.nan
    pooled[nan, :] = np.nan
    return Summary(pooled, pc, pmin)


def rung_trace(x: np.ndarray, beta: np.ndarray, value: float, n_chains: int):
    """Follow one temperature through the swaps of Metropolis-coupled MCMC -- the numpy restatement of csrc/k_mc3_summary.hip: k_mc3_gather.
    x [n, B, Q] and beta [n, B] (the reciprocal temperature every chain ran with, as record_fetch returns it); the B chains are B // n_chains
    groups of n_chains consecutive chains.  Returns (trace [n, B // n_chains, Q], holder [n, B // n_chains] int32): sample by sample the
    row of the one chain of each group whose beta EQUALS `value` (a rung of the ladder: the swap phase stores the ladder's doubles, so
    equality is exact), and that chain's index in its group.  ValueError where a (sample, group) does not have exactly one such chain."""
    x, beta = np.asarray(x, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    C = int(n_chains)
    if x.ndim != 3 or beta.shape != x.shape[:2] or C < 1 or x.shape[1] % C != 0:
        raise ValueError("rung_trace: expected x [n, B, Q], beta [n, B] and B a multiple of n_chains")
    n, B, Q = x.shape
    G = B // C
    hit = beta.reshape(n, G, C) == value
    count = hit.sum(axis=2)
    if np.any(count != 1):
        k, g = (int(v) for v in np.argwhere(count != 1)[0])
        raise ValueError(f"rung_trace: sample {k} of group {g} has {int(count[k, g])} chains at beta = {value!r}")
    holder = hit.argmax(axis=2).astype(np.int32)
    trace = np.take_along_axis(x.reshape(n, G, C, Q), holder[:, :, None, None].astype(np.int64), axis=2)[:, :, 0, :]
    return np.ascontiguousarray(trace), holder


def replica_flow(beta: np.ndarray, ladder: Sequence[float]):
    """How the chains travel over the temperature ladder (csrc/k_mc3_summary.hip: k_mc3_flow, restated): beta [n, B] as for rung_trace,
    ladder [C] strictly decreasing from 1.  Returns (visits [B, C] int64: the samples each chain spent at each rung, a beta mapped to its
    rung by equality; round_trips [B] int64: completed passages cold -> hottest -> cold -- armed at rung 0, marked at rung C - 1, counted at
    the next return to rung 0).  A beta that is not on the ladder counts nowhere."""
    beta, ladder = np.asarray(beta, dtype=np.float64), np.asarray(ladder, dtype=np.float64)
    if beta.ndim != 2 or ladder.ndim != 1 or len(ladder) < 2:
        raise ValueError("replica_flow: expected beta [n, B] and a ladder of at least two rungs")
    n, B = beta.shape
    C = len(ladder)
    on = beta[:, :, None] == ladder[None, None, :]                       # [n, B, C]
    visits = on.sum(axis=0).astype(np.int64)
    rung = np.where(on.any(axis=2), on.argmax(axis=2), -1)
    trips = np.zeros(B, np.int64)
    for b in range(B):
        state = 0                                                        # 0 idle, 1 armed at the cold rung, 2 has reached the hottest
        for r in rung[:, b]:
            if r == 0:
                trips[b] += state == 2
                state = 1
            elif r == C - 1 and state == 1:
                state = 2
    return visits, trips


def trace_summary(X, max_lag: int = 0, device=True, per_chain: bool = True, q: Optional[int] = None) -> Summary:
    """mcd_trace_summary on X [n, B, ldq]: a numpy array (copied to device 0, or to device `device` if that is an int) or a torch
    tensor on a GPU (read in place).  q: the quantities summarised (default: all ldq of them).  There is no host path: `device` False
    is refused -- the host restatement is `summary`."""
    if device is False:
        raise ValueError("trace_summary: the kernels run on the device; diagnostics.summary is the host restatement")
    ptr, on_device, dev, (n, B, ldq) = reduction_source(X, 3, device, "trace_summary", "[n, B, ldq]")
    Q = ldq if q is None else int(q)
    pooled = np.empty((max(Q, 0), len(COLUMNS)))
    pc = np.empty((B, max(Q, 0), 4)) if per_chain else None
    _capi.check(_capi.lib().mcd_trace_summary(n, B, Q, ldq, ptr, on_device, dev, int(max_lag), dp(pooled), dp(pc) if per_chain else None))
    return Summary(pooled, pc)


# ---- the marginal likelihood from power-posterior chains (include/mcmcdate_mvn.h: mcd_ml_estimate) ------------------------------------
ML_COLUMNS = ("mean", "variance", "minimum", "maximum", "ln_ratio")


def power_posterior_points(n_points: int, alpha: float = 0.3) -> np.ndarray:
    """The exponents (k / (K - 1))^(1 / alpha), k = 0 .. K - 1, of K path points: 0 (the prior) ... 1 (the posterior), dense near the prior
    where the ln likelihood changes fastest (Xie et al. 2011 take the quantiles of Beta(alpha, 1), alpha = 0.3).  This project's choice:
    what package `mcmc` spaces its points by is not restated."""
    K = int(n_points)
    if K < 2:
        raise ValueError("power_posterior_points: at least 2 points (the prior and the posterior)")
    if not alpha > 0:
        raise ValueError("power_posterior_points: alpha must be positive")
    b = (np.arange(K) / (K - 1.0)) ** (1.0 / alpha)
    b[0], b[-1] = 0.0, 1.0
    return b


@dataclass
class MarginalLikelihoodEstimate:
    """point [K, 5] (ML_COLUMNS, pooled over a point's values), replicate [C, 2] (stepping stones, trapezoid of each replicate's own chains),
    the pooled stepping-stone estimate ln_z_ss and trapezoid ln_z_ti with the standard errors sd(replicate column) / sqrt(C)."""
    point: np.ndarray
    replicate: np.ndarray
    ln_z_ss: float
    se_ss: float
    ln_z_ti: float
    se_ti: float
    n_samples: int = 0

    @classmethod
    def from_arrays(cls, point, replicate, out, n_samples=0):
        return cls(point, replicate, float(out[0]), float(out[1]), float(out[2]), float(out[3]), int(n_samples))


def _check_betas(betas, batch: int) -> np.ndarray:
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    K = betas.size
    if betas.ndim != 1 or K < 2 or K > 4096:
        raise ValueError("marginal likelihood: betas must hold 2 .. 4096 points")
    if betas[0] != 0.0 or betas[-1] != 1.0 or not np.all(np.diff(betas) > 0):
        raise ValueError("marginal likelihood: betas must start at 0, end at 1 and increase strictly")
    if batch % K != 0:
        raise ValueError(f"marginal likelihood: {batch} chains are not whole groups of {K} points")
    return betas


def _mean_exact(x: np.ndarray, axis) -> np.ndarray:
    """Mean along `axis`; equal values have that value as their mean, whatever the rounding of the sum."""
    mx, mn = x.max(axis=axis), x.min(axis=axis)
    return np.where(mx == mn, mx, x.mean(axis=axis))


def _se(v: np.ndarray) -> float:
    """sd(v) / sqrt(C), unbiased; equal values: 0 exactly; C = 1 or a NaN: NaN."""
    C_ = v.size
    if C_ < 2 or np.isnan(v).any():
        return float("nan")
    if v.max() == v.min():
        return 0.0
    return float(np.sqrt(((v - v.mean()) ** 2).sum() / (C_ - 1)) / np.sqrt(C_))


def marginal_likelihood(ll: np.ndarray, betas) -> MarginalLikelihoodEstimate:
    """The definitions of mcd_ml_estimate in numpy: ll [n, batch], chain b at point b mod K, replicate b // K."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim != 2:
        raise ValueError("marginal_likelihood: expected ll [n, batch]")
    n, B = ll.shape
    betas = _check_betas(betas, B)
    K = betas.size
    C_ = B // K
    if n < 1 or n * C_ < 2:
        raise ValueError("marginal_likelihood: need at least 2 values per point")
    delta = np.append(np.diff(betas), 0.0)                                       # [K]; the last point has no stone
    x = ll.reshape(n, C_, K)                                                     # [sample, replicate, point]
    with np.errstate(all="ignore"):
        bad = np.isnan(x).any(axis=0)                                            # [C, K]
        mx = np.where(bad, np.nan, x.max(axis=0))
        m = np.where(bad, np.nan, _mean_exact(x, 0))
        S = np.exp(delta * (x - mx)).sum(axis=0)                                 # [C, K]
        pbad = bad.any(axis=0)                                                   # [K]
        pooled = x.reshape(n * C_, K)
        MX, MN = pooled.max(axis=0), pooled.min(axis=0)
        mean = _mean_exact(pooled, 0)
        var = np.where(MX == MN, 0.0, ((pooled - mean) ** 2).sum(axis=0) / (n * C_ - 1.0))
        lnr = delta * MX + np.log((S * np.exp(delta * (mx - MX))).sum(axis=0) / (n * C_))
        lnr[K - 1] = np.nan
        point = np.stack([mean, var, MN, MX, lnr], axis=1)
        point[pbad] = np.nan
        d = delta[:K - 1]
        rep = np.stack([(d * mx[:, :K - 1] + np.log(S[:, :K - 1] / n)).sum(axis=1),
                        (d * (m[:, :K - 1] + m[:, 1:]) / 2.0).sum(axis=1)], axis=1)
        out = [point[:K - 1, 4].sum(), _se(rep[:, 0]), (d * (point[:K - 1, 0] + point[1:, 0]) / 2.0).sum(), _se(rep[:, 1])]
    return MarginalLikelihoodEstimate.from_arrays(point, rep, out, n)


def marginal_likelihood_device(ll, betas, device=True) -> MarginalLikelihoodEstimate:
    """mcd_ml_estimate on ll [n, batch]: a numpy array (copied to device 0, or to device `device` if that is an int) or a contiguous float64
    torch tensor on a GPU (read in place).  There is no host path: the host restatement is `marginal_likelihood`."""
    if device is False:
        raise ValueError("marginal_likelihood_device: the kernels run on the device; diagnostics.marginal_likelihood is the host restatement")
    ptr, on_device, dev, (n, B) = reduction_source(ll, 2, device, "marginal_likelihood_device", "[n, batch]")
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    K = int(betas.size)
    point = np.empty((max(K, 0), _capi.MCD_ML_COLS))
    rep = np.empty((max(B // K if K else 0, 1), 2))
    out = np.empty(4)
    _capi.check(_capi.lib().mcd_ml_estimate(n, B, ptr, on_device, dev, K, dp(betas), dp(point), dp(rep), dp(out)))
    return MarginalLikelihoodEstimate.from_arrays(point, rep, out, n)
