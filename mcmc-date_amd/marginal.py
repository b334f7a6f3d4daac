"""The marginal likelihood ln Z on the device: every path point a lock-step chain.

Replaces `runMarginalLikelihood` (app/Main.hs:511-543): `marginalLikelihood mlS p l c m i g` of package `mcmc` with the settings of
app/Definitions.hs:447-472 (128 points, 4000 iterations per point, the `repetitiveBurnIn` schedule).  The reference walks its one chain
along the path, point after point; here the K points are K chains of one `Sampler` that differ only in the exponent of the likelihood
(`Sampler.set_power`: prior x likelihood^beta), stepped in lock step, C = batch / K replicates of the whole path side by side.  There is
no walk along the path: every chain burns in at its own point with its own auto-tuned proposals, then all record together, and the
estimators read the recorded ln likelihoods in the device recorder's ring (`Sampler.record_marginal`, csrc/k_marginal.hip).

What `mcmc`'s marginalLikelihood does in detail (point spacing, forward and backward passes) is not restated here: the path points
(`diagnostics.power_posterior_points`), the estimators and their standard errors over the replicates are this project's definitions
(include/mcmcdate_mvn.h, mcd_ml_estimate), unpinned against `mcmc`'s own implementation.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from .diagnostics import MarginalLikelihoodEstimate, power_posterior_points
from .sampler import Sampler

N_POINTS = 128                                  # nPoints, app/Definitions.hs:452-453
ITERATIONS_MARGINAL_LH = 4000                   # iterationsMarginalLh, :448-449
REPETITIVE_BURN_IN_FAST = [20, 40, 60, 80]      # repetitiveBurnIn, :461-465
REPETITIVE_BURN_IN_SLOW = [100] * 6


class MarginalLikelihood:
    """Power-posterior chains over `sampler` (its state set, no recorder active, no MC3): chain b runs at point (first_chain + b) % n_points."""

    def __init__(self, sampler: Sampler, n_points: int = N_POINTS, alpha: float = 0.3):
        K = int(n_points)
        if K < 2 or K > 4096:
            raise ValueError("MarginalLikelihood: n_points must be 2 .. 4096")
        if sampler.batch % K != 0 or sampler.first_chain % K != 0:
            raise ValueError(f"MarginalLikelihood: the sampler's chains [{sampler.first_chain}, {sampler.first_chain + sampler.batch}) are not whole "
                             f"groups of {K} path points")
        self.sampler = sampler
        self.n_points = K
        self.replicates = sampler.batch // K
        self.betas = power_posterior_points(K, alpha)
        self.chain_beta = self.betas[(sampler.first_chain + np.arange(sampler.batch)) % K]
        sampler.set_power(self.chain_beta)

    def burn_in(self, fast: Sequence[int] = REPETITIVE_BURN_IN_FAST, slow: Sequence[int] = REPETITIVE_BURN_IN_SLOW):
        """The sampler's own burn-in with auto tuning after every period: the tuning parameters are per chain, so every point tunes at its own
        exponent."""
        self.sampler.burn_in(fast, slow)

    def run(self, n_iter: int = ITERATIONS_MARGINAL_LH, period: int = 2, chunk: int = 256) -> MarginalLikelihoodEstimate:
        """n_iter iterations of every chain with every `period`-th state recorded on the device, then the estimate from the recorded ln
        likelihoods.  The ring holds all n_iter // period samples of the run (batch x (2 ld + 16) doubles each) until the call returns."""
        n = int(n_iter) // int(period)
        if n < 1:
            raise ValueError("MarginalLikelihood.run: no sample would be recorded")
        s = self.sampler
        s.record_begin(period, n)
        try:
            s.run(int(n_iter), chunk=chunk)
            return s.record_marginal(self.betas)
        finally:
            s.record_end()
