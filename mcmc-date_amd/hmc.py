"""Device leapfrog of the Hamiltonian proposal (second part) and a plain HMC transition on top of it.

`Leapfrog` wraps `mcd_hmc_*` (include/mcmcdate_mvn.h): the state of B chains, their momenta and the gradient of
ln [prior x likelihood x jacobianRootBranch] (`htargetWith`, app/Hamiltonian.hs:72-92) live on the device; positions
use the reference's layout (`getMask` / `toVector`, :33-53; identical to `hamiltonian.to_vector`).

The reference's proposal is NUTS from the `mcmc` package (`nutsWith`, :95-105; dschrempf/mcmc 542c43f6, not vendored).
Restated here from the published algorithm it implements -- Hoffman & Gelman, "The No-U-Turn Sampler", JMLR 15 (2014):
`nuts_transition` is Algorithm 3 (efficient NUTS: slice variable, recursive doubling, U-turn and divergence stops,
uniform sampling from the admissible set), `DualAveraging` the step-size adaptation of Algorithm 6 -- with the device
doing every leapfrog step for all chains at once and the per-chain recursion as host-side control flow (one Python
generator per chain; the driver gathers the leapfrog requests of all active chains into one `mcd_hmc_step_from` call).
The product path is `Leapfrog.nuts` / `Leapfrog.nuts_run`: the same algorithm as a per-chain state machine ON THE DEVICE
(csrc/k_nuts.hip, mcd_hmc_nuts*), dual averaging inside the library, step-level parity with a CPU twin
(tests/test_gpu_nuts.py); the host-side recursion below stays as the readable restatement of the control flow.
`mcmc`'s own tuning (`HTuneLeapfrog HTuneAllMasses`) and its defaults are NOT restated: parity unpinned for this part.
`hmc_transition` is the textbook fixed-length HMC step, kept as the simplest end-to-end exercise of the integrator.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from . import _capi
from ._arrays import dp, ip
from .likelihood import SparseTreeLikelihood, TreeLikelihood
from .prior import PriorFunction
from .recorder import DriverCalls
from .state import StateBatch


def _odp(a):
    """dp of an optional array."""
    return None if a is None else dp(a)


# ---- the dense metric's algebra restated in numpy (what tests/test_gpu_dense_metric.py compares the device with) -------------------------
def shrunk_covariance(Q) -> np.ndarray:
    """The metric mcd_hmc_nuts_warmup_dense takes from the n positions Q [n, dim] of a window: n / (n + 5) Cov + 1e-3 5 / (n + 5) I,
    Cov the centred maximum-likelihood covariance (divided by n) -- Stan's regularisation, whose diagonal is nuts_warmup's rule."""
    Q = np.asarray(Q, np.float64)
    n, dim = Q.shape
    d = Q - Q.mean(axis=0)
    return (n / (n + 5.0)) * (d.T @ d / n) + 1e-3 * (5.0 / (n + 5.0)) * np.eye(dim)


def metric_factors(C):
    """(U, W) of a dense metric C = M^-1: U lower triangular with U U^T = C, W = U^-T (upper triangular), so W W^T = C^-1 = M and
    p = W z has covariance M for standard normal z."""
    U = np.linalg.cholesky(np.asarray(C, np.float64))
    W = np.triu(np.linalg.solve(U, np.eye(U.shape[0])).T)         # (the general solver leaves rounding dust below the diagonal)
    return U, W


_FACTOR_WHERE = {"host": _capi.MCD_HMC_FACTOR_HOST, "device": _capi.MCD_HMC_FACTOR_DEVICE}


class MetricRefused(_capi.McdError):
    """factor_metric refused C: `info` = (MCD_METRIC_FACTOR_* kind, row, column) of the first offender (the pivot twice)."""

    def __init__(self, code: int, message: str, info):
        _capi.McdError.__init__(self, code, message)
        self.info = tuple(int(v) for v in info)


def factor_metric(C, where: str = "host", device_id: int = 0):
    """(sym, U, Uinv) of a dense metric C [dim, dim] as the library takes them (mcd_metric_factor): sym = (C + C^T) / 2 with C's diagonal,
    U lower triangular with U U^T = sym, Uinv = U^-1 -- what a Leapfrog keeps on its device --, zeros above the diagonal.
    where="host": the long double loops behind set_metric's default, no GPU needed; "device": the kernels behind
    set_metric_factor("device") on GPU device_id (NoDevice without one: nothing falls back to the host).  Refused as set_metric refuses
    (MetricRefused with .info naming the offender); dim > 4098: McdError (unsupported)."""
    if where not in _FACTOR_WHERE:
        raise _capi.McdError(_capi.MCD_ERR_INVALID_ARG, f"factor_metric: where = {where!r} is none of {sorted(_FACTOR_WHERE)}")
    C = np.ascontiguousarray(C, dtype=np.float64)
    if C.ndim != 2 or C.shape[0] != C.shape[1]:
        raise ValueError("factor_metric: C must be [dim, dim]")
    dim = C.shape[0]
    if dim > _capi.MCD_HMC_DENSE_ACROSS_MAX_DIM:            # refused by the library before anything of this size is allocated here
        sym = U = W = None
    else:
        sym, U, W = np.empty((dim, dim)), np.empty((dim, dim)), np.empty((dim, dim))
    info = (ctypes.c_int64 * 3)()
    rc = _capi.lib().mcd_metric_factor(dim, dp(C), _FACTOR_WHERE[where], int(device_id), _odp(sym), _odp(U), _odp(W), info)
    if rc == _capi.MCD_ERR_INVALID_ARG and info[0] != _capi.MCD_METRIC_FACTOR_OK:
        raise MetricRefused(rc, _capi.lib().mcd_last_error().decode(), info)
    _capi.check(rc)
    return sym, U, W


def _metric_gemm(X, A, Y=None, lower: bool = False, rows: Optional[int] = None, rows_list=None, stride: int = 0, device_id: int = 0):
    """The product kernel of the across-chains form on host arrays (mcd_metric_gemm_, csrc/k_metric_gemm.hip: for tests).  X [mem_rows, dim],
    A [dim, dim]; Y [mem_rows, dim] goes to the device as it is (None: zeros) and is returned as the launch left it.  Without rows_list the
    first `rows` rows (default: all) are multiplied; with it, product row r is memory row (r // n_list) stride + rows_list[r % n_list].
    The device buffers have exactly the arrays' sizes; a list entry or a mapped row outside mem_rows is refused (McdError), nothing runs."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    A = np.ascontiguousarray(A, dtype=np.float64)
    if X.ndim != 2 or A.shape != (X.shape[1], X.shape[1]):
        raise ValueError("_metric_gemm: X must be [mem_rows, dim] and A [dim, dim]")
    Y = np.zeros_like(X) if Y is None else np.array(Y, dtype=np.float64, order="C")
    if Y.shape != X.shape:
        raise ValueError("_metric_gemm: Y must have X's shape")
    lst = None if rows_list is None else np.ascontiguousarray(rows_list, dtype=np.int32)
    if rows is None:
        rows = X.shape[0] if lst is None else lst.size
    f = _capi.lib().mcd_metric_gemm_
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(ctypes.c_double)] * 3 + [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                  ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
    _capi.check(f(dp(X), dp(A), dp(Y), X.shape[0], X.shape[1], int(bool(lower)), None if lst is None else ip(lst), 0 if lst is None else lst.size,
                  int(stride), int(rows), int(device_id)))
    return Y


def _hmc_cov(Q, device_id: int = 0):
    """(mean [dim], cov [dim, dim]) of the samples Q [n, dim] by the warm-up's covariance kernels (mcd_hmc_cov_, csrc/k_hmc_cov.hip: for
    tests): cov is the centred covariance divided by n."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    if Q.ndim != 2:
        raise ValueError("_hmc_cov: Q must be [n, dim]")
    n, dim = Q.shape
    mean, cov = np.empty(dim), np.empty((dim, dim))
    f = _capi.lib().mcd_hmc_cov_
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                  ctypes.c_int]
    _capi.check(f(dp(Q), n, dim, dp(mean), dp(cov), int(device_id)))
    return mean, cov


class _Metric:
    """M^-1 as the numpy helpers below use it: a vector (diagonal) or a symmetric matrix (dense)."""

    def __init__(self, inv_mass, dim: int):
        a = np.asarray(inv_mass, np.float64)
        self.dense = a.ndim == 2
        self.a = np.ascontiguousarray(a if self.dense else np.broadcast_to(a, (dim,)))
        self.W = metric_factors(self.a)[1] if self.dense else None

    def apply(self, r):
        """M^-1 r, for r [dim] or [B, dim]."""
        return r @ self.a if self.dense else r * self.a

    def kinetic(self, r):
        return 0.5 * np.sum(r * self.apply(r), axis=-1)

    def momenta(self, z):
        """z ~ N(0, I) [B, dim] -> p ~ N(0, M)."""
        return z @ self.W.T if self.dense else z / np.sqrt(self.a)

    def device_arg(self, lf):
        """What Leapfrog's calls take as inv_mass: the vector, or None after making sure the handle holds this dense metric."""
        if not self.dense:
            return self.a
        cur = lf.metric()
        if cur is None or not np.array_equal(cur, 0.5 * (self.a + self.a.T)):
            lf.set_metric(self.a)
        return None


class Leapfrog(DriverCalls):
    """B chains on one GPU.  `tree_lik` (a TreeLikelihood, or a SparseTreeLikelihood: the precision matrix stays sparse on the device,
    mcd_hmc_create_sparse, trees of up to 2048 nodes) and `prior` must live on the same device and outlive this object."""
    _API, _HANDLE = "mcd_hmc", ("_h", "mcd_hmc_destroy")

    def __init__(self, tree_lik: "TreeLikelihood | SparseTreeLikelihood", prior: PriorFunction, calibrations_available: bool, batch: int):
        self.topo = tree_lik.topo
        self.batch = int(batch)
        self._keep = (tree_lik, prior)
        self._create(tree_lik, prior._p, int(bool(calibrations_available)), self.batch)
        self.dim = int(_capi.lib().mcd_hmc_dim(self._h))

    def take_state(self, sampler):
        """The current states of the sampler.Sampler become this handle's, on the device (mcd_hmc_take_state): set_state(sampler.state())
        to the bit -- state, position, ln target and gradient -- without the host in between."""
        _capi.check(_capi.lib().mcd_hmc_take_state(self._h, sampler._h))

    def position(self):
        """(q [B, dim], ln target [B], gradient [B, dim]) of the current state."""
        q, g = np.empty((self.batch, self.dim)), np.empty((self.batch, self.dim))
        v = np.empty(self.batch)
        _capi.check(_capi.lib().mcd_hmc_get_position(self._h, dp(q), dp(v), dp(g)))
        return q, v, g

    def _inv_mass(self, inv_mass):
        """The vector argument of the diagonal metric, [dim] (a scalar is broadcast); None -- the handle's dense metric -- stays None."""
        if inv_mass is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(inv_mass, np.float64), (self.dim,)))

    # -- the dense metric (mcd_hmc_set_metric): the full inverse mass matrix C = M^-1 in the place of the vector inv_mass ------
    def set_metric(self, C):
        """C [dim, dim], symmetric positive definite, becomes the handle's metric (momenta p = U^-T z with C = U U^T, kinetic energy
        1/2 p^T C p, drift q += eps C p, U-turn test through C); leapfrog / step_from / nuts / nuts_run then take inv_mass=None.
        Refused (McdError, the handle untouched): a non-finite entry, an asymmetric pair, not positive definite, dim > 512 in the
        default per-chain form (set_metric_form("across_chains") serves every dim).  The factors are taken on the host, or on the device
        after set_metric_factor("device")."""
        C = np.ascontiguousarray(C, dtype=np.float64)
        if C.shape != (self.dim, self.dim):
            raise ValueError("set_metric: C must be [dim, dim]")
        _capi.check(_capi.lib().mcd_hmc_set_metric(self._h, dp(C)))

    _METRIC_FORMS = {"per_chain": _capi.MCD_HMC_METRIC_PER_CHAIN, "across_chains": _capi.MCD_HMC_METRIC_ACROSS_CHAINS}

    def set_metric_form(self, form: str):
        """How the dense metric's products are taken (mcd_hmc_set_metric_form): "per_chain" (the default: one workgroup's sum per chain,
        dim <= 512) or "across_chains" (the lock-step chains' products as one matrix product on the matrix cores, every dim).  Allowed
        only while no dense metric is set (McdError otherwise, the handle untouched); survives clear_metric."""
        if form not in self._METRIC_FORMS:
            raise ValueError(f"set_metric_form: {form!r} is none of {sorted(self._METRIC_FORMS)}")
        _capi.check(_capi.lib().mcd_hmc_set_metric_form(self._h, self._METRIC_FORMS[form]))

    @property
    def metric_form(self) -> str:
        """"per_chain" or "across_chains": the handle's form of the dense metric's products."""
        form = ctypes.c_int(-1)
        _capi.check(_capi.lib().mcd_hmc_get_metric_form(self._h, ctypes.byref(form)))
        return next(name for name, value in self._METRIC_FORMS.items() if value == form.value)

    def set_metric_factor(self, where: str):
        """Where set_metric and nuts_warmup_dense take the factors of C from now on (mcd_hmc_set_metric_factor): "host" (the default: long
        double loops on the CPU, C and U^-1 uploaded) or "device" (k_metric_factor.hip: the same definitions on the fp64 matrix cores, the
        window covariance never leaves the GPU; factors equal to the host's up to the last bits, the same bits on every call).  Allowed
        at any time; survives clear_metric."""
        if where not in _FACTOR_WHERE:
            raise ValueError(f"set_metric_factor: {where!r} is none of {sorted(_FACTOR_WHERE)}")
        _capi.check(_capi.lib().mcd_hmc_set_metric_factor(self._h, _FACTOR_WHERE[where]))

    @property
    def metric_factor(self) -> str:
        """"host" or "device": where the handle takes the factors of a dense metric."""
        where = ctypes.c_int(-1)
        _capi.check(_capi.lib().mcd_hmc_get_metric_factor(self._h, ctypes.byref(where)))
        return next(name for name, value in _FACTOR_WHERE.items() if value == where.value)

    _TRANSITION_FORMS = {"rounds": _capi.MCD_HMC_TRANSITION_ROUNDS, "one_launch": _capi.MCD_HMC_TRANSITION_ONE_LAUNCH}

    def set_transition_form(self, form: str):
        """How a transition is launched (mcd_hmc_set_transition_form): "rounds" (the default: three launches and one host poll per leapfrog
        step of a tree) or "one_launch" (csrc/k_nuts_chain.hip: a whole transition of every chain, and the steps of leapfrog(), as ONE
        kernel launch; the same bits as "rounds" with the substitution sweep as its likelihood gradient).  "one_launch" serves dense
        likelihoods of up to 64 distances (trees of up to 66 nodes) with the diagonal metric or a dense one in the per-chain form;
        refused otherwise (McdError, Unsupported, the handle untouched).  Allowed at any time between calls."""
        if form not in self._TRANSITION_FORMS:
            raise ValueError(f"set_transition_form: {form!r} is none of {sorted(self._TRANSITION_FORMS)}")
        _capi.check(_capi.lib().mcd_hmc_set_transition_form(self._h, self._TRANSITION_FORMS[form]))

    @property
    def transition_form(self) -> str:
        """"rounds" or "one_launch": how the handle launches a transition."""
        form = ctypes.c_int(-1)
        _capi.check(_capi.lib().mcd_hmc_get_transition_form(self._h, ctypes.byref(form)))
        return next(name for name, value in self._TRANSITION_FORMS.items() if value == form.value)

    def _metric_uinv(self):
        """The handle's U^-1 [dim, dim] read back from the device (mcd_hmc_metric_uinv_: for tests)."""
        f = _capi.lib().mcd_hmc_metric_uinv_
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        W = np.empty((self.dim, self.dim))
        _capi.check(f(self._h, dp(W)))
        return W

    def clear_metric(self):
        """Back to the diagonal metric: the handle is what it was before set_metric."""
        _capi.check(_capi.lib().mcd_hmc_set_metric(self._h, None))

    def metric(self):
        """The stored, exactly symmetric C [dim, dim] of the dense metric, or None when the handle has none."""
        dense = ctypes.c_int(0)
        _capi.check(_capi.lib().mcd_hmc_get_metric(self._h, ctypes.byref(dense), None))
        if not dense.value:
            return None
        C = np.empty((self.dim, self.dim))
        _capi.check(_capi.lib().mcd_hmc_get_metric(self._h, ctypes.byref(dense), dp(C)))
        return C

    def nuts_warmup_dense(self, eps0, inv_mass0, windows: int = 3, window: int = 60, delta: float = 0.65, max_depth: int = 6, seed: int = 0,
                          first_transition: int = 0, chain_offset: int = 0):
        """Step sizes and the FULL mass matrix tuned in the library (mcd_hmc_nuts_warmup_dense: the schedule of nuts_warmup, after every
        window C = shrunk_covariance of the positions it visited) from the diagonal inv_mass0.  The final metric stays set on the
        handle.  Returns (eps [B], C [dim, dim], mean acceptance statistic of the closing window [B])."""
        eps = np.array(np.broadcast_to(np.asarray(eps0, np.float64), (self.batch,)), dtype=np.float64, order="C")
        im = self._inv_mass(inv_mass0)
        ma, C = np.empty(self.batch), np.empty((self.dim, self.dim))
        _capi.check(_capi.lib().mcd_hmc_nuts_warmup_dense(self._h, int(windows), int(window), dp(eps), dp(im), float(delta), int(max_depth), int(seed),
                                                          int(chain_offset), int(first_transition), dp(ma), dp(C)))
        return eps, C, ma

    def leapfrog(self, p, eps, inv_mass, n_steps: int, direction=None):
        """n_steps leapfrog steps from the current state with momenta p [B, dim]; returns the new momenta (the state is
        advanced on the device; read it with position() / state()).  inv_mass=None: the handle's dense metric (set_metric)."""
        p = np.array(p, dtype=np.float64, order="C")
        eps = np.ascontiguousarray(np.broadcast_to(np.asarray(eps, np.float64), (self.batch,)))
        inv_mass = self._inv_mass(inv_mass)
        d = None if direction is None else np.ascontiguousarray(direction, dtype=np.float64)
        if p.shape != (self.batch, self.dim):
            raise ValueError("leapfrog: p must be [batch, dim]")
        _capi.check(_capi.lib().mcd_hmc_leapfrog(self._h, dp(p), dp(eps), _odp(d), _odp(inv_mass),
                                                 int(n_steps)))
        return p


    def nuts(self, eps, inv_mass, max_depth: int = 8, seed: int = 0, transition: int = 0, chain_offset: int = 0):
        """One NUTS transition of every chain ON THE DEVICE (mcd_hmc_nuts, csrc/k_nuts.hip: Hoffman & Gelman 2014, Algorithm 3
        as a per-chain state machine; counter-based random streams (seed, chain_offset + b, transition)).  Returns (mean
        acceptance statistic [B], tree depth [B]); the chains' new states are on the device.  inv_mass=None: the handle's dense metric."""
        eps = np.ascontiguousarray(np.broadcast_to(np.asarray(eps, np.float64), (self.batch,)))
        inv_mass = self._inv_mass(inv_mass)
        alpha = np.empty(self.batch)
        depth = np.empty(self.batch, np.int32)
        _capi.check(_capi.lib().mcd_hmc_nuts(self._h, dp(eps), _odp(inv_mass), int(max_depth), int(seed), int(chain_offset), int(transition),
                                             dp(alpha), ip(depth)))
        return alpha, depth

    def nuts_run(self, n_transitions: int, eps, inv_mass, adapt: bool = False, delta: float = 0.65, max_depth: int = 8, seed: int = 0,
                 first_transition: int = 0, chain_offset: int = 0):
        """n transitions in the library (mcd_hmc_nuts_run); adapt: dual averaging of the step sizes (Algorithm 6).  Returns
        (eps [B] -- the averaged step sizes when adapting --, mean acceptance statistic [B], position means [dim], pooled
        position variances [dim]).  inv_mass=None: the handle's dense metric."""
        eps = np.array(np.broadcast_to(np.asarray(eps, np.float64), (self.batch,)), dtype=np.float64, order="C")
        inv_mass = self._inv_mass(inv_mass)
        ma, qm, qv = np.empty(self.batch), np.empty(self.dim), np.empty(self.dim)
        _capi.check(_capi.lib().mcd_hmc_nuts_run(self._h, int(n_transitions), int(bool(adapt)), dp(eps), _odp(inv_mass),
                                                 float(delta), int(max_depth),
                                                 int(seed), int(chain_offset), int(first_transition), dp(ma), dp(qm), dp(qv)))
        return eps, ma, qm, qv

    def nuts_warmup(self, eps, inv_mass, windows: int = 3, window: int = 60, delta: float = 0.65, max_depth: int = 6, seed: int = 0,
                    first_transition: int = 0, chain_offset: int = 0):
        """Step sizes and diagonal masses tuned in the library (mcd_hmc_nuts_warmup: `HTuneLeapfrog HTuneAllMasses`,
        app/Hamiltonian.hs:62-63).  Returns (eps [B], inv_mass [dim], mean acceptance statistic of the closing window [B])."""
        eps = np.array(np.broadcast_to(np.asarray(eps, np.float64), (self.batch,)), dtype=np.float64, order="C")
        inv_mass = np.array(np.broadcast_to(np.asarray(inv_mass, np.float64), (self.dim,)), dtype=np.float64, order="C")
        ma = np.empty(self.batch)
        _capi.check(_capi.lib().mcd_hmc_nuts_warmup(self._h, int(windows), int(window), dp(eps), dp(inv_mass), float(delta), int(max_depth), int(seed),
                                                    int(chain_offset), int(first_transition), dp(ma)))
        return eps, inv_mass, ma

    # -- the sample recorder (mcd_hmc_record_*) ------------------------------------------------------------------------------
    NUTS_FIELDS = ("depth", "leapfrog_steps", "alpha", "diverged", "eps", "joint0")
    NUTS_STATS = ("divergent", "mean_depth", "max_depth", "leapfrog_steps")
    _REC_API, _REC_TAIL = "mcd_hmc_record", (len(NUTS_FIELDS),)

    def record_begin(self, period: int = 1, capacity: int = 128):
        """Keep the state of every chain and the diagnostics of the transition after every `period`-th NUTS transition (counted from
        this call, through nuts / nuts_run / nuts_warmup alike) on the device, in a ring of `capacity` samples; a call whose samples
        would not fit is refused before it starts (drain with record_fetch)."""
        super().record_begin(period, capacity)

    def record_fetch(self, max_samples: Optional[int] = None):
        """The oldest waiting samples (all of them, or at most max_samples), whose slots are free afterwards -- the arrays of
        Sampler.record_fetch with the transitions' diagnostics in the place of the temperatures:
        (transition [n] counted from record_begin, scalars [n, B, 5] = birth, death, tH, rMu, rVar, heights [n, B, n_nodes],
        rates [n, B, n_nodes], post [n, B, 3] = ln prior, ln likelihood, ln jacobianRootBranch, nuts [n, B, 6] = NUTS_FIELDS: tree
        depth, leapfrog steps, acceptance statistic, diverged (0 / 1), the step size used, -H at the start of the transition)."""
        return self._record_fetch(max_samples)

    def record_summary(self, skip: int = 0, n: Optional[int] = None, max_lag: int = 255, per_chain: bool = False):
        """Sampler.record_summary on this driver's recorder (mcd_hmc_record_summary: computed on the device from the ring, nothing is
        fetched, no slot is freed): a sampler.RecordSummary whose `nuts_stats` [B, 4] holds per chain NUTS_STATS -- divergent
        transitions, mean and maximum tree depth, leapfrog steps -- of the window."""
        from .sampler import RecordSummary

        stats = np.empty((self.batch, 4))
        pooled, used, lag, pc = self._record_summary(skip, n, max_lag, per_chain, stats)
        return RecordSummary(pooled, self.topo.n_nodes, used, lag, pc, stats)

    def step_from(self, q, p, grad, eps, inv_mass, direction=None, have_grad=True):
        """One leapfrog step from the given phase points (all [B, dim]); returns (q', p', grad', ln target').  inv_mass=None: the
        handle's dense metric."""
        q = np.array(q, dtype=np.float64, order="C")
        p = np.array(p, dtype=np.float64, order="C")
        g = np.array(grad, dtype=np.float64, order="C")
        eps = np.ascontiguousarray(np.broadcast_to(np.asarray(eps, np.float64), (self.batch,)))
        inv_mass = self._inv_mass(inv_mass)
        d = None if direction is None else np.ascontiguousarray(direction, dtype=np.float64)
        v = np.empty(self.batch)
        _capi.check(_capi.lib().mcd_hmc_step_from(self._h, dp(q), dp(p), dp(g), int(bool(have_grad)), dp(eps),
                                                  _odp(d), _odp(inv_mass), dp(v)))
        return q, p, g, v


def hmc_transition(lf: Leapfrog, rng: np.random.Generator, eps, inv_mass, n_steps: int) -> np.ndarray:
    """One fixed-length HMC transition for every chain: p ~ N(0, M), n leapfrog steps, accept with probability
    min(1, exp(H_old - H_new)), H = -ln target + 1/2 p^T M^-1 p.  Rejected chains (and chains that left the support:
    NaN) are put back.  inv_mass: [dim], or a dense metric [dim, dim] (set on the handle).  Returns the acceptance mask."""
    met = _Metric(inv_mass, lf.dim)
    old = lf.state()
    _, v0, _ = lf.position()
    p0 = met.momenta(rng.normal(size=(lf.batch, lf.dim)))
    h0 = -v0 + met.kinetic(p0)
    p1 = lf.leapfrog(p0, eps, met.device_arg(lf), n_steps)
    _, v1, _ = lf.position()
    h1 = -v1 + met.kinetic(p1)
    with np.errstate(over="ignore", invalid="ignore"):
        accept = np.log(rng.uniform(size=lf.batch)) < (h0 - h1)
    accept &= np.isfinite(h1)
    if not accept.all():
        new = lf.state()
        keep = accept
        merged = StateBatch(np.where(keep[:, None], new.heights, old.heights), np.where(keep[:, None], new.rates, old.rates),
                            np.where(keep, new.time_height, old.time_height), np.where(keep, new.rate_mean, old.rate_mean),
                            np.where(keep, new.time_birth_rate, old.time_birth_rate), np.where(keep, new.time_death_rate, old.time_death_rate),
                            np.where(keep, new.rate_variance, old.rate_variance))
        lf.set_state(merged)
    return accept


# ---- NUTS: Hoffman & Gelman (2014), Algorithm 3, one generator per chain -----------------------------------------------
DELTA_MAX = 1000.0


def _nuts_chain(q0, g0, logp0, r0, log_u, rng, inv_mass, max_depth, stats):
    """Generator of one chain's transition.  Yields leapfrog requests (q, r, grad, direction) and receives
    (q', r', grad', ln target'); returns the selected (q, grad, ln target).  inv_mass: [dim], or a dense metric [dim, dim]."""
    inv_mass = np.asarray(inv_mass, np.float64)
    dense = inv_mass.ndim == 2

    def kinetic(r):
        if dense:
            return 0.5 * float(np.dot(r, inv_mass @ r))
        return 0.5 * float(np.sum(r * r * inv_mass))

    def no_u_turn(qm, rm, qp, rp):
        d = qp - qm
        if dense:
            w = inv_mass @ d                                # one product serves both ends: the metric is symmetric
            return float(np.dot(w, rm)) >= 0.0 and float(np.dot(w, rp)) >= 0.0
        return float(np.dot(d, rm * inv_mass)) >= 0.0 and float(np.dot(d, rp * inv_mass)) >= 0.0

    def build_tree(q, r, g, v, j):
        if j == 0:
            q1, r1, g1, lp1 = yield (q, r, g, v)
            joint = lp1 - kinetic(r1)                       # -H
            if not math.isfinite(joint):
                joint = -math.inf
            n1 = 1 if log_u <= joint else 0
            s1 = log_u < DELTA_MAX + joint
            stats["alpha"] += min(1.0, math.exp(min(0.0, joint - stats["joint0"])))
            stats["n_alpha"] += 1
            return q1, r1, g1, q1, r1, g1, q1, g1, lp1, n1, s1
        qm, rm, gm, qp, rp, gp, qc, gc, lpc, n1, s1 = yield from build_tree(q, r, g, v, j - 1)
        if s1:
            if v == -1:
                qm, rm, gm, _, _, _, qc2, gc2, lpc2, n2, s2 = yield from build_tree(qm, rm, gm, v, j - 1)
            else:
                _, _, _, qp, rp, gp, qc2, gc2, lpc2, n2, s2 = yield from build_tree(qp, rp, gp, v, j - 1)
            if n2 > 0 and rng.uniform() < n2 / max(1, n1 + n2):
                qc, gc, lpc = qc2, gc2, lpc2
            s1 = s2 and no_u_turn(qm, rm, qp, rp)
            n1 += n2
        return qm, rm, gm, qp, rp, gp, qc, gc, lpc, n1, s1

    qm = qp = q0
    rm = rp = r0
    gm = gp = g0
    q_new, g_new, lp_new = q0, g0, logp0
    n, s, j = 1, True, 0
    while s and j < max_depth:
        v = -1 if rng.uniform() < 0.5 else 1
        if v == -1:
            qm, rm, gm, _, _, _, qc, gc, lpc, n1, s1 = yield from build_tree(qm, rm, gm, v, j)
        else:
            _, _, _, qp, rp, gp, qc, gc, lpc, n1, s1 = yield from build_tree(qp, rp, gp, v, j)
        if s1 and rng.uniform() < min(1.0, n1 / n):
            q_new, g_new, lp_new = qc, gc, lpc
        n += n1
        s = s1 and no_u_turn(qm, rm, qp, rp)
        j += 1
    stats["depth"] = j
    return q_new, g_new, lp_new


def nuts_transition(lf: Leapfrog, rng: np.random.Generator, eps, inv_mass, max_depth: int = 8):
    """One NUTS transition (Algorithm 3) for every chain of `lf`, all chains advancing their trees in lock step on the
    device.  eps: scalar or [B].  Returns (mean acceptance statistic alpha / n_alpha per chain [B], tree depth [B]);
    the chains' new states are on the device (lf.state(), lf.position()).  inv_mass: [dim], or a dense metric [dim, dim], which is
    set on the handle."""
    B, D = lf.batch, lf.dim
    met = _Metric(inv_mass, D)
    inv_mass, dev_mass = met.a, met.device_arg(lf)
    eps = np.ascontiguousarray(np.broadcast_to(np.asarray(eps, np.float64), (B,)))
    q0, lp0, g0 = lf.position()
    r0 = met.momenta(rng.normal(size=(B, D)))
    joint0 = lp0 - met.kinetic(r0)
    log_u = joint0 + np.log(rng.uniform(size=B))
    chain_rngs = [np.random.default_rng(rng.integers(0, 2 ** 63)) for _ in range(B)]
    stats = [{"alpha": 0.0, "n_alpha": 0, "joint0": float(joint0[b]), "depth": 0} for b in range(B)]
    gens = [_nuts_chain(q0[b].copy(), g0[b].copy(), float(lp0[b]), r0[b].copy(), float(log_u[b]), chain_rngs[b], inv_mass, max_depth, stats[b])
            for b in range(B)]
    result = [None] * B
    request = [None] * B
    for b in range(B):
        try:
            request[b] = next(gens[b])
        except StopIteration as done:               # cannot happen before the first leapfrog, kept for completeness
            result[b] = done.value
    q_in, p_in, g_in = q0.copy(), r0.copy(), g0.copy()
    direction = np.ones(B)
    while any(r is not None for r in request):
        for b in range(B):
            if request[b] is not None:
                q_in[b], p_in[b], g_in[b], v = request[b]
                direction[b] = float(v)
            else:                                    # finished chains ride along with a harmless step from their result
                q_in[b], g_in[b] = result[b][0], result[b][1]
                p_in[b] = 0.0
                direction[b] = 1.0
        q1, p1, g1, lp1 = lf.step_from(q_in, p_in, g_in, eps, dev_mass, direction=direction, have_grad=True)
        for b in range(B):
            if request[b] is None:
                continue
            try:
                request[b] = gens[b].send((q1[b].copy(), p1[b].copy(), g1[b].copy(), float(lp1[b])))
            except StopIteration as done:
                request[b] = None
                result[b] = done.value
    # the selected points become the chains' states (zero-length step: the device evaluates ln target and gradient there)
    q_sel = np.array([r[0] for r in result])
    lf.step_from(q_sel, np.zeros((B, D)), np.array([r[1] for r in result]), np.zeros(B), dev_mass, have_grad=True)
    alpha = np.array([s["alpha"] / max(1, s["n_alpha"]) for s in stats])
    return alpha, np.array([s["depth"] for s in stats])


class DualAveraging:
    """Step-size adaptation of Hoffman & Gelman, Algorithm 6 (one instance per chain set; vectorised over chains)."""

    def __init__(self, eps0, delta: float = 0.65, gamma: float = 0.05, t0: float = 10.0, kappa: float = 0.75):
        eps0 = np.asarray(eps0, np.float64)
        self.mu = np.log(10.0 * eps0)
        self.delta, self.gamma, self.t0, self.kappa = delta, gamma, t0, kappa
        self.h_bar = np.zeros_like(eps0)
        self.log_eps = np.log(eps0)
        self.log_eps_bar = np.zeros_like(eps0)
        self.m = 0

    def update(self, alpha):
        self.m += 1
        m = self.m
        self.h_bar = (1.0 - 1.0 / (m + self.t0)) * self.h_bar + (self.delta - np.asarray(alpha)) / (m + self.t0)
        self.log_eps = self.mu - math.sqrt(m) / self.gamma * self.h_bar
        w = m ** (-self.kappa)
        self.log_eps_bar = w * self.log_eps + (1.0 - w) * self.log_eps_bar
        return np.exp(self.log_eps)

    def final(self):
        return np.exp(self.log_eps_bar)


def nuts_warmup(lf: Leapfrog, rng: np.random.Generator, n_windows: int = 3, window: int = 60, eps0: float = 0.02, delta: float = 0.65,
                max_depth: int = 6, inv_mass=None):
    """Warm-up of step sizes and diagonal masses (the reference tunes both: `HTuningConf HTuneLeapfrog HTuneAllMasses`,
    app/Hamiltonian.hs:62-63; `mcmc`'s own scheme is not restated).  Windows of `window` transitions: dual averaging
    of the step sizes inside a window, then the inverse masses are set to the pooled variance of the positions visited
    in that window (over chains and transitions, shrunk towards their mean for stability).  The first window starts
    from inverse masses (0.1 q)^2, or from `inv_mass`; a 2-D `inv_mass` asks for the dense metric: every window then ends with
    shrunk_covariance of its later three quarters.  Returns (eps [B], inv_mass [dim] or [dim, dim])."""
    q0, _, _ = lf.position()
    dense = inv_mass is not None and np.ndim(inv_mass) == 2
    if inv_mass is None:
        inv_mass = np.maximum((0.1 * np.abs(q0)).mean(axis=0) ** 2, 1e-12)
    eps = np.full(lf.batch, float(eps0))
    for w in range(n_windows):
        da = DualAveraging(eps, delta=delta)
        qs = []
        for _ in range(window):
            alpha, _ = nuts_transition(lf, rng, eps, inv_mass, max_depth=max_depth)
            eps = da.update(alpha)
            qs.append(lf.position()[0])
        eps = da.final()
        if dense:
            inv_mass = shrunk_covariance(np.concatenate(qs[window // 4:]))
            continue
        var = np.concatenate(qs[window // 4:]).var(axis=0)
        n_eff = lf.batch * (window - window // 4)
        inv_mass = (n_eff / (n_eff + 5.0)) * var + 1e-3 * (5.0 / (n_eff + 5.0))      # Stan-style shrinkage
    da = DualAveraging(eps, delta=delta)
    for _ in range(window):
        alpha, _ = nuts_transition(lf, rng, eps, inv_mass, max_depth=max_depth)
        eps = da.update(alpha)
    return da.final(), inv_mass


NUTS_STREAM_DOMAIN = 0x4E5554535F524E47          # "NUTS_RNG": keeps the NUTS streams apart from the Metropolis-Hastings streams of the same seed


def run_cycle_with_nuts(sampler, lf: Leapfrog, rng: np.random.Generator, n_iter: int, eps, inv_mass, max_depth: int = 6,
                        accumulate: bool = False, device: bool = True, seed: Optional[int] = None, first_transition: Optional[int] = None,
                        chain_offset: Optional[int] = None):
    """The reference's `--hamiltonian` mode: the Metropolis-Hastings cycle plus one NUTS proposal per iteration
    (`maybeHamiltonianProposal`, weight 1, app/Definitions.hs:272-274, 104-105 of app/Hamiltonian.hs).  The cycle runs in the lock-step
    driver, the NUTS transition on the device (`device=True`: Leapfrog.nuts, tree building in csrc/k_nuts.hip; False: the
    host-side recursion nuts_transition, kept as the reference implementation of the control flow); the states move between
    the two handles through the host once per iteration (a few KB).  The reference shuffles the NUTS proposal into the
    cycle; here it closes every iteration.

    Random streams of the device transitions: Philox (seed ^ NUTS_STREAM_DOMAIN, chain_offset + b, transition).  `seed`
    defaults to the sampler's (the domain constant keeps the draws apart from the Metropolis-Hastings draws of the same
    (chain, step)); `chain_offset` to the sampler's first GLOBAL chain (shards.shard_sampler), so the ranks of a sharded run draw
    different numbers; `first_transition` to the number of transitions this Leapfrog has already made through this
    function, so a burn-in call followed by a sampling call does not replay its draws.
    Returns (mean acceptance statistic of the NUTS transitions, mean absolute node ages tH * h_v over chains and
    iterations [n_nodes] or None)."""
    seed = int(getattr(sampler, "seed", 0) if seed is None else seed) ^ NUTS_STREAM_DOMAIN
    chain_offset = int(getattr(sampler, "first_chain", 0) if chain_offset is None else chain_offset)
    t0 = int(getattr(lf, "cycle_transitions_done", 0) if first_transition is None else first_transition)
    alphas = []
    ages = np.zeros(lf.topo.n_nodes) if accumulate else None
    for it in range(n_iter):
        sampler.run(1)
        lf.set_state(sampler.state())
        if device:
            alpha, _ = lf.nuts(eps, inv_mass, max_depth=max_depth, seed=seed, transition=t0 + it, chain_offset=chain_offset)
        else:
            alpha, _ = nuts_transition(lf, rng, eps, inv_mass, max_depth=max_depth)
        alphas.append(alpha.mean())
        s = lf.state()
        sampler.set_state(s)
        if accumulate:
            ages += (s.time_height[:, None] * s.heights).mean(axis=0)
    lf.cycle_transitions_done = t0 + n_iter
    return (float(np.mean(alphas)) if alphas else float("nan")), (ages / max(1, n_iter) if accumulate else None)
