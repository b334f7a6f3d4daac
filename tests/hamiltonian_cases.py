"""What tests/test_gpu_handover.py and tests/test_gpu_mh_hamiltonian.py share: the problems (tree, likelihood, prior, proposal table, initial
states), samplers and leapfrog handles on them, and the COMPOSITION that defines the attached run -- per iteration mcd_hmc_set_state of
mcd_mh_get_state, mcd_hmc_nuts, mcd_mh_set_state of mcd_hmc_get_state, mcd_mh_run of one iteration -- made of calls that existed before
the hand-over did, so that no expected value comes from the code under test."""
import os

import numpy as np

import mcmc_date_amd as M
from mcmc_date_amd import _capi
from mcmc_date_amd.hmc import NUTS_STREAM_DOMAIN

FIELDS = ("time_birth_rate", "time_death_rate", "time_height", "rate_mean", "rate_variance", "heights", "rates")
# name -> (likelihood, fixture or leaves, chains, knobs, the MCD_MH_PATH_* values the run may take)
CASES = {
    "23-nodes-chain-lds": ("golden", "12-leaves-variable-rate", 6, {}, (1,)),
    "23-nodes-sparse-segments": ("golden-sparse", "12-leaves-variable-rate", 6, {}, (9,)),
    "67-nodes-chain-streamed": ("dense", 34, 4, {}, (2,)),
    "67-nodes-per-phase": ("dense", 34, 4, {"MCD_MH_PER_PHASE": 1}, (3, 4)),       # two launches per step, the prior blocks kept
    "259-nodes-segments": ("dense", 130, 4, {}, (8,)),
}
_problems = {}


class Case:
    def __init__(self, name, knobs):
        from mcmc_date_amd import synthetic as S

        kind, what, self.B, self.knobs, self.paths = CASES[name]
        for k, v in self.knobs.items():                      # (MCD_MH_PER_PHASE is read by mcd_mh_create: set before any sampler exists)
            knobs.setenv(k, v)
        key = (kind, what)
        if key not in _problems:
            if kind.startswith("golden"):
                fx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", what + ".npz")))
                topo = M.Topology(fx["parent"])
                cal = [M.Calibration(f"c{i}", int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for i, r in enumerate(fx["cal"])]
                con = [M.Constraint(f"k{i}", int(r[0]), int(r[1]), r[2]) for i, r in enumerate(fx["con"])]
                ht = float(fx["prior_ht"])
                if kind == "golden":
                    lik = M.MvnLikelihood(M.Full(fx["mu"], fx["sigma_inv"], float(fx["logdet"]))).bind_tree(topo)
                else:
                    P = np.asarray(fx["sigma_inv"])
                    assoc = [((int(i), int(j)), float(P[i, j])) for i in range(P.shape[0]) for j in range(P.shape[1])]
                    lik = M.SparseLikelihood(M.Sparse(fx["mu"], assoc, float(fx["logdet"]))).bind_tree(topo)
                pf = M.PriorFunction(ht, "UncorrelatedGamma", cal, con, [], topo)
                ps, _ = M.proposals(topo, [], calibrations_available=True)
                x0 = M.init_with(topo, fx["mean_lengths"])
                x0.time_height = ht
                s0 = M.StateBatch.from_states([x0] * 8)
            else:
                topo = S.random_topology(what, seed=31)
                n = topo.n_nodes - 2
                mu, sigma = S.random_spd_problem(n, seed=n)
                lik = M.MvnLikelihood.from_covariance(mu, sigma).bind_tree(topo)
                inner = [v for v in range(1, topo.n_nodes) if (np.asarray(topo.parent) == v).any()]
                cal = [M.Calibration("root", 0, 0.9, 0.025, 1.3, 0.025), M.Calibration("c", int(inner[len(inner) // 2]), 1e-3, 0.025, 5.0, 0.025)]
                pf = M.PriorFunction(1.0, "UncorrelatedLogNormal", cal, [], [], topo)
                ps, _ = M.proposals(topo, [], calibrations_available=True)
                s0 = S.random_states(topo, 8, seed=5)
                s0.time_birth_rate = np.full(8, 1.0); s0.time_death_rate = np.full(8, 0.8); s0.rate_variance = np.full(8, 0.3)
            _problems[key] = (topo, lik, pf, ps, s0)
        self.topo, self.lik, self.pf, self.ps, self.s0 = _problems[key]

    def rows(self, lo, hi):
        s = self.s0
        return M.StateBatch(**{f: np.ascontiguousarray(getattr(s, f)[lo:hi]) for f in FIELDS})

    def sampler(self, seed=77, burn=True, batch=None, first_chain=0):
        """A sampler after a short burn-in with auto tuning (so the chains and their tuning parameters differ); two samplers made by the
        same call hold the same bits, step counter included."""
        B = self.B if batch is None else batch
        smp = M.Sampler(self.lik, self.pf, self.ps, B, seed=seed, first_chain=first_chain)
        smp.set_state(self.rows(first_chain, first_chain + B))
        if burn:
            for _ in range(2):
                smp.run(6)
                smp.autotune()
        return smp

    def leapfrog(self, batch=None):
        return M.Leapfrog(self.lik, self.pf, True, self.B if batch is None else batch)

    def schedule(self, n_iter, seed=4):
        return M.cycle_schedule(self.ps, n_iter, np.random.default_rng(seed))

    def check_path(self, smp):
        got = int(_capi.lib().mcd_mh_last_path(smp._h))
        assert got in self.paths, f"meant for launch structure {self.paths}, the run took {got}: {smp.last_path()}"

    def nuts_inputs(self, lf, smp):
        """(eps [B], inv_mass [dim]) for the chains `smp` holds: the starting masses of hmc.nuts_warmup, step sizes that differ per chain."""
        lf.set_state(smp.state())
        q = lf.position()[0]
        return np.linspace(0.01, 0.03, smp.batch), np.maximum((0.1 * np.abs(q)).mean(axis=0) ** 2, 1e-12)


def same_states(a, b):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def compose(smp, lf, sched, eps, inv_mass, max_depth, first_transition=0, accumulate=False, seed=None):
    """The definition of the attached run through the host: returns (trace_alpha, trace_accept, the states after every iteration, the
    sums of the transitions' alpha [B] added in order, of their depths [B])."""
    seed = (smp.seed ^ NUTS_STREAM_DOMAIN) if seed is None else seed
    ta, tk, states = [], [], []
    asum, dsum = np.zeros(smp.batch), np.zeros(smp.batch, np.int64)
    for it in range(sched.shape[0]):
        lf.set_state(smp.state())
        alpha, depth = lf.nuts(eps, inv_mass, max_depth=max_depth, seed=seed, transition=first_transition + it, chain_offset=smp.first_chain)
        asum += alpha
        dsum += depth
        smp.set_state(lf.state())
        a, k = smp.run_schedule(sched[it:it + 1], accumulate=accumulate, trace=True)
        ta.append(a)
        tk.append(k)
        states.append(smp.state())
    return np.concatenate(ta), np.concatenate(tk), states, asum, dsum
