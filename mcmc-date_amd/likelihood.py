"""Host-side mirror of the reference's likelihood plugin surface (app/Probability.hs:152-281,
361-410) on top of the C ABI (include/mcmcdate_mvn.h).

Names follow the reference: `LikelihoodData` with constructors `Full | Sparse | Univariate |
NoData` (app/Probability.hs:210-235), `likelihood_function` (:277-281), `jacobian_root_branch`
(:408-410), `.data` files (app/Main.hs:75-99).  All four constructors run through the same HIP
kernels: `Univariate` is a diagonal covariance, `Sparse` a precision matrix given as an association
list.  There is no CPU evaluation path here.

Arrays may be numpy (host pointers: copied, evaluated, returned synchronously) or torch CUDA
tensors (device pointers: enqueued on torch's current stream, results returned as CUDA tensors).
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass
from typing import Callable, List, Sequence, Tuple, Union

import numpy as np

from . import _capi
from ._arrays import LIKELIHOOD_FIELDS, Staged, _check_cuda, _host, _is_torch, _ptr, _stream_ptr, dp, ip    # (the underscored names: importable from here as before)
from .state import State, StateBatch
from .tree import Topology


# ----------------------------------------------------------------------------------------------
# LikelihoodData -- app/Probability.hs:210-235
# ----------------------------------------------------------------------------------------------
@dataclass
class Full:
    """Multivariate normal with full inverted covariance matrix and log det of the covariance."""
    mu: np.ndarray
    sigma_inv: np.ndarray
    logdet_sigma: float


@dataclass
class Sparse:
    """Multivariate normal with sparse inverted covariance matrix, [((i, j), value), ...]."""
    mu: np.ndarray
    sigma_inv_assoc: List[Tuple[Tuple[int, int], float]]
    logdet_sigma: float


@dataclass
class Univariate:
    """Univariate normal distributions: means and variances."""
    mu: np.ndarray
    vs: np.ndarray


@dataclass
class NoData:
    """No likelihood; use prior only (likelihood 1.0, app/Probability.hs:281)."""


LikelihoodData = Union[Full, Sparse, Univariate, NoData]


def read_data_file(path: str) -> LikelihoodData:
    """`getData` -- app/Main.hs:85-99 (aeson default sum encoding of LikelihoodDataStore, :75-81)."""
    with open(path) as f:
        r = json.load(f)
    tag = r.get("tag")
    if tag == "FullS":
        mu, rows, logdet = r["contents"]
        return Full(np.asarray(mu, float), np.asarray(rows, float), float(logdet))
    if tag == "SparseS":
        mu, assoc, logdet = r["contents"]
        return Sparse(np.asarray(mu, float), [((int(ij[0]), int(ij[1])), float(v)) for ij, v in assoc], float(logdet))
    if tag == "UnivariateS":
        mu, vs = r["contents"]
        return Univariate(np.asarray(mu, float), np.asarray(vs, float))
    if tag == "NoLikelihoodS":
        return NoData()
    raise ValueError(f"getData: Could not decode data file: {path}.")  # app/Main.hs:89


def write_data_file(path: str, lhd: LikelihoodData) -> None:
    """Inverse of `read_data_file` (what `prepare` writes, app/Main.hs:240, 286)."""
    if isinstance(lhd, Full):
        obj = {"tag": "FullS", "contents": [list(map(float, lhd.mu)), [list(map(float, r)) for r in lhd.sigma_inv],
                                            float(lhd.logdet_sigma)]}
    elif isinstance(lhd, Sparse):
        obj = {"tag": "SparseS", "contents": [list(map(float, lhd.mu)),
                                              [[[int(i), int(j)], float(v)] for (i, j), v in lhd.sigma_inv_assoc],
                                              float(lhd.logdet_sigma)]}
    elif isinstance(lhd, Univariate):
        obj = {"tag": "UnivariateS", "contents": [list(map(float, lhd.mu)), list(map(float, lhd.vs))]}
    else:
        obj = {"tag": "NoLikelihoodS"}
    with open(path, "w") as f:
        json.dump(obj, f)


# ----------------------------------------------------------------------------------------------
# the likelihood object (owns the C handle)
# ----------------------------------------------------------------------------------------------
FORMS = {"auto": 0, "sweep": 1, "multiply": 2}    # MCD_FORM_* (include/mcmcdate_mvn.h)


def set_logpdf_form(form: str) -> str:
    """Choose the form of the log-density kernels for this process: "auto" (by dimension and batch size), "sweep" (one
    chain per wave, the latency form) or "multiply" (z = L^-1 (x - mu) on the fp64 matrix cores, the throughput form).
    Returns the previous setting.  The two forms agree to rounding, not bit for bit."""
    if form not in FORMS:
        raise ValueError(f"set_logpdf_form: expected one of {sorted(FORMS)}, got {form!r}")
    prev = _capi.lib().mcd_set_logpdf_form(FORMS[form])
    if prev < 0:
        _capi.check(prev)
    return {v: k for k, v in FORMS.items()}[prev]


class _Calls(_capi.OwnsHandle):
    """A handle whose entry points share the symbol prefix _API (the dense and the sparse classes differ in nothing else)."""

    def _call(self, op):
        return getattr(_capi.lib(), f"{self._API}_{op}")


class _VectorLikelihood(_Calls):
    """logpdf / grad on raw vectors over the handle `_h` of dimension `n` on `device` (<_API>_logpdf_batch, <_API>_grad_batch)."""
    _nodata = False

    def logpdf(self, X):
        """Batch of independent evaluations: X [batch, n] chain-major (numpy or CUDA tensor) -> ll[batch]."""
        s = Staged("logpdf", self.device, X=X).check_matrix(None if self._nodata else self.n)
        if self._nodata:
            return s.zeros(s.batch)
        X, = s.arrays
        ll = s.empty(s.batch)
        _capi.check(self._call("logpdf_batch")(self._h, _ptr(X), s.ld(X), s.batch, s.on_device, s.stream, _ptr(ll)))
        return ll

    def grad(self, X):
        """(ll, G) with G[b] = d ll / d x_b = -Sigma^-1 (x_b - mu)."""
        if self._nodata:
            raise ValueError("grad: NoData has no gradient path (the reference offers likelihoodFunctionG for Full only)")
        s = Staged("grad", self.device, X=X).check_matrix(self.n)
        X, = s.arrays
        ll, G = s.empty(s.batch), s.empty_like(X)
        _capi.check(self._call("grad_batch")(self._h, _ptr(X), s.ld(X), s.batch, s.on_device, s.stream, _ptr(ll), _ptr(G), s.ld(G)))
        return ll, G


class MvnLikelihood(_VectorLikelihood):
    """`likelihoodFunction lhd` with its operands staged once on one GPU.

    Equivalent of the closure built in getLikelihoodFunction (app/Main.hs:333-347).
    """
    _API, _HANDLE = "mcd_mvn", ("_h", "mcd_mvn_destroy")

    def __init__(self, lhd: LikelihoodData, device: int = 0):
        self._h = C.c_void_p()
        self.device = int(device)
        self.lhd = lhd
        self._nodata = isinstance(lhd, NoData)
        if self._nodata:
            self.n = 0
            return
        if isinstance(lhd, Full):
            mu = _host(lhd.mu)
            mat = _host(lhd.sigma_inv)
            kind, logdet = _capi.MCD_MAT_SIGMA_INV, float(lhd.logdet_sigma)
        elif isinstance(lhd, Sparse):
            mu = _host(lhd.mu)
            mat = np.zeros((len(mu), len(mu)))
            for (i, j), v in lhd.sigma_inv_assoc:      # L.mkSparse, app/Main.hs:95
                mat[i, j] += v
            kind, logdet = _capi.MCD_MAT_SIGMA_INV, float(lhd.logdet_sigma)
        elif isinstance(lhd, Univariate):
            mu = _host(lhd.mu)
            vs = _host(lhd.vs)
            mat = np.diag(vs)                           # Sigma = diag(vs); logdet = sum log vs (:274)
            kind, logdet = _capi.MCD_MAT_SIGMA, 0.0
        else:
            raise TypeError(f"not a LikelihoodData: {lhd!r}")
        n = len(mu)
        if mat.shape != (n, n):
            raise ValueError("LikelihoodData: matrix shape does not match the mean vector")
        self.n = n
        _capi.check(_capi.lib().mcd_mvn_create(C.byref(self._h), n, dp(mu), dp(mat), kind, C.c_double(logdet), self.device))

    @classmethod
    def from_covariance(cls, mu, sigma, device: int = 0) -> "MvnLikelihood":
        """Operands given as (mu, Sigma) -- what `meanCov` returns (app/Main.hs:208)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.device = int(device)
        self.lhd = None
        self._nodata = False
        mu = _host(mu)
        sigma = _host(sigma)
        self.n = len(mu)
        if sigma.shape != (self.n, self.n):
            raise ValueError("from_covariance: matrix shape does not match the mean vector")
        _capi.check(_capi.lib().mcd_mvn_create(C.byref(self._h), self.n, dp(mu), dp(sigma), _capi.MCD_MAT_SIGMA, C.c_double(0.0),
                                               self.device))
        return self

    def release_stream(self, stream) -> None:
        """mcd_mvn_release_stream: the scratch set the row-split kernels keep for `stream` (a torch.cuda.Stream or a raw
        hipStream_t value) goes back to the handle's pool; call it before destroying a short-lived stream."""
        raw = getattr(stream, "cuda_stream", stream)
        _capi.check(_capi.lib().mcd_mvn_release_stream(self._h, C.c_void_p(int(raw) if raw else 0)))

    def set_form(self, form: str) -> str:
        """Pin the form of the log-density kernels for THIS handle ("auto": follow the process default, "sweep",
        "multiply"); mcd_mvn_set_form.  Returns the previous choice."""
        if form not in FORMS:
            raise ValueError(f"set_form: expected one of {sorted(FORMS)}, got {form!r}")
        if self._nodata:
            return "auto"
        prev = _capi.lib().mcd_mvn_set_form(self._h, FORMS[form])
        if prev < 0:
            _capi.check(prev)
        return {v: k for k, v in FORMS.items()}[prev]

    @property
    def logdet_sigma(self) -> float:
        return 0.0 if self._nodata else float(_capi.lib().mcd_mvn_logdet(self._h))

    def cholesky_factor(self) -> np.ndarray:
        out = np.empty((self.n, self.n))
        _capi.check(_capi.lib().mcd_mvn_get_factor(self._h, dp(out)))
        return out

    # -- evaluation (logpdf and grad: _VectorLikelihood) ---------------------------------------
    def logpdf1(self, x: Sequence[float]) -> float:
        """One evaluation: drop-in for logDensityFullMultivariateNormal (app/Probability.hs:166-173)."""
        if self._nodata:
            return 0.0
        x = _host(x)
        if x.shape != (self.n,):
            raise ValueError("logpdf1: wrong vector length")
        out = C.c_double()
        _capi.check(_capi.lib().mcd_mvn_logpdf(self._h, dp(x), C.byref(out)))
        return out.value

    def logpdf_into(self, X, ll):
        """Device-resident variant writing into a caller-provided CUDA tensor (no allocation).  The unchecked fast path: nothing about
        X or ll is verified here (logpdf is the checked call); both must be contiguous float64 CUDA tensors on this handle's device,
        X [batch, n] and ll [batch]."""
        _capi.check(_capi.lib().mcd_mvn_logpdf_batch(self._h, _ptr(X), X.stride(0), X.shape[0], 1,
                                                     _stream_ptr(self.device), _ptr(ll)))
        return ll

    def bind_tree(self, topo: Topology) -> "TreeLikelihood":
        return TreeLikelihood(self, topo)


class _StateLikelihood(_Calls):
    """State -> ln likelihood and ln jacobianRootBranch over the tree handle `_t` bound to a vector likelihood (<_API>_create,
    <_API>_loglik_batch, <_API>_grad_batch).  `sparse` is what the drivers choose their constructor by."""

    def __init__(self, lik: _VectorLikelihood, topo: Topology):
        self._lik = lik
        self.topo = topo
        self._t = C.c_void_p()
        if lik._nodata:
            topo.root_children()
            return
        par = np.ascontiguousarray(topo.parent, dtype=np.int32)
        _capi.check(self._call("create")(C.byref(self._t), lik._h, len(par), ip(par)))

    def _stage(self, what: str, states: StateBatch) -> Staged:
        return Staged.state(what, self._lik.device, states, LIKELIHOOD_FIELDS).check_state(self.topo.n_nodes)

    def loglik(self, states: StateBatch, want_jacobian: bool = True):
        """(ll[batch], log jacobianRootBranch[batch] or None)."""
        s = self._stage("loglik", states)
        if self._lik._nodata:
            return s.zeros(s.batch), None
        H, R, tH, rMu = s.arrays
        ll = s.empty(s.batch)
        lj = s.empty(s.batch) if want_jacobian else None
        _capi.check(self._call("loglik_batch")(self._t, _ptr(H), _ptr(R), s.ld(H), _ptr(tH), _ptr(rMu), s.batch, s.on_device, s.stream,
                                               _ptr(ll), _ptr(lj) if want_jacobian else None))
        return ll, lj

    def grad(self, states: StateBatch):
        """(ll, g_heights[batch, n_nodes], g_rates[batch, n_nodes], g_time_height[batch], g_rate_mean[batch]): one launch; the sparse form
        (csrc/k_sparse_grad.hip) takes trees of up to 2048 nodes."""
        if self._lik._nodata:
            raise ValueError("grad: NoData has no gradient path")
        s = self._stage("grad", states)
        H, R, tH, rMu = s.arrays
        ll = s.empty(s.batch)
        gH, gR, gt, gm = (s.empty_like(a) for a in s.arrays)
        if s.ld(gH) != s.ld(H) or s.ld(gR) != s.ld(H):         # (the call takes one row stride for heights, rates and both gradients)
            raise ValueError("grad: heights and rates must share one row stride")
        _capi.check(self._call("grad_batch")(self._t, _ptr(H), _ptr(R), s.ld(H), _ptr(tH), _ptr(rMu), s.batch, s.on_device, s.stream,
                                             _ptr(ll), _ptr(gH), _ptr(gR), _ptr(gt), _ptr(gm)))
        return ll, gH, gR, gt, gm


class TreeLikelihood(_StateLikelihood):
    """State -> log-likelihood: likelihoodFunctionWrapper (app/Probability.hs:195-207) on device."""
    _API, _HANDLE, sparse = "mcd_tree", ("_t", "mcd_tree_destroy"), False

    def __init__(self, mvn: MvnLikelihood, topo: Topology):
        super().__init__(mvn, topo)
        self.mvn = mvn


# ----------------------------------------------------------------------------------------------
# the sparse form, natively (no densification; N up to MCD_MAX_SPARSE_DIM = 8192)
# ----------------------------------------------------------------------------------------------
MAX_SPARSE_DIM = 8192


class SparseLikelihood(_VectorLikelihood):
    """`likelihoodFunction (Sparse mu sigmaInvSparse logDetSigma)` (app/Probability.hs:279, 178-184) with the precision matrix kept
    sparse on the device (csrc/k_sparse.hip, mcd_sparse_*): the reference's route for trees with thousands of branches.  Takes the
    `Sparse` record of a `.data` file (read_data_file) or of `prepare`.  logpdf / grad on raw vectors, bind_tree(topo).loglik on
    states, bind_tree(topo).grad for the gradient of states (trees of up to 2048 nodes); `Sampler` and `hmc.Leapfrog` take the bound tree
    as it is.  `MvnLikelihood(Sparse ...)` densifies instead (N <= 1024)."""
    _API, _HANDLE = "mcd_sparse", ("_h", "mcd_sparse_destroy")

    def __init__(self, lhd: Sparse, device: int = 0):
        if not isinstance(lhd, Sparse):
            raise TypeError("SparseLikelihood: need a Sparse record")
        self._h = C.c_void_p()
        self.device = int(device)
        self.lhd = lhd
        mu = _host(lhd.mu)
        self.n = len(mu)
        row = np.ascontiguousarray([ij[0] for ij, _ in lhd.sigma_inv_assoc], dtype=np.int32)
        col = np.ascontiguousarray([ij[1] for ij, _ in lhd.sigma_inv_assoc], dtype=np.int32)
        val = np.ascontiguousarray([v for _, v in lhd.sigma_inv_assoc], dtype=np.float64)
        _capi.check(_capi.lib().mcd_sparse_create(C.byref(self._h), self.n, dp(mu), len(val), ip(row), ip(col), dp(val),
                                                  C.c_double(float(lhd.logdet_sigma)), self.device))
        self.nnz = int(_capi.lib().mcd_sparse_nnz(self._h))

    def bind_tree(self, topo: Topology) -> "SparseTreeLikelihood":
        return SparseTreeLikelihood(self, topo)


class SparseTreeLikelihood(_StateLikelihood):
    """State -> ln likelihood and ln jacobianRootBranch over a sparse precision matrix (mcd_sparse_tree_*)."""
    _API, _HANDLE, sparse = "mcd_sparse_tree", ("_t", "mcd_sparse_tree_destroy"), True

    def __init__(self, sp: SparseLikelihood, topo: Topology):
        super().__init__(sp, topo)
        self.sp = sp


# ----------------------------------------------------------------------------------------------
# the reference's plugin functions
# ----------------------------------------------------------------------------------------------
def likelihood_function(lhd: LikelihoodData, topo: Topology, device: int = 0) -> Callable[[State], float]:
    """`likelihoodFunction :: LikelihoodData -> LikelihoodFunction I` (app/Probability.hs:277-281).

    Returns a pure function State -> log-likelihood (log domain) that evaluates on the GPU.
    """
    if isinstance(lhd, Sparse) and len(lhd.mu) > 1024:           # beyond the dense kernels: the precision matrix stays sparse on the device
        tl = SparseLikelihood(lhd, device).bind_tree(topo)
    else:
        try:
            tl = MvnLikelihood(lhd, device).bind_tree(topo)
        except _capi.NotPositiveDefinite:
            # The dense kernels need a factor of the matrix; the reference evaluates dx . (P dx) with whatever P the record holds
            # (app/Probability.hs:169, 183).  An indefinite precision matrix therefore takes the product form on the device
            # (csrc/k_sparse.hip: P as given, nothing factored) -- same value as the reference's, on the GPU.
            if isinstance(lhd, Full):
                P = _host(lhd.sigma_inv)
                ii, jj = np.nonzero(P)
                lhd = Sparse(lhd.mu, [((int(i), int(j)), float(P[i, j])) for i, j in zip(ii, jj)], lhd.logdet_sigma)
            elif not isinstance(lhd, Sparse):
                raise
            tl = SparseLikelihood(lhd, device).bind_tree(topo)

    def f(x: State) -> float:
        ll, _ = tl.loglik(StateBatch.from_states([x]), want_jacobian=False)
        return float(ll[0])

    f.tree_likelihood = tl
    return f


def jacobian_root_branch(lhd: LikelihoodData, topo: Topology, device: int = 0) -> Callable[[State], float]:
    """`jacobianRootBranch` (app/Probability.hs:408-410): log (1 / rootBranch x), evaluated on the GPU
    as a by-product of the likelihood kernel."""
    tl = MvnLikelihood(lhd, device).bind_tree(topo)

    def j(x: State) -> float:
        _, lj = tl.loglik(StateBatch.from_states([x]), want_jacobian=True)
        return float(lj[0])

    j.tree_likelihood = tl
    return j
