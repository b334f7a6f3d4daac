"""What `Sampler` (mcd_mh_*) and `hmc.Leapfrog` (mcd_hmc_*) share: the handle's lifetime, the chains' state in and out (`DriverCalls`) and the
sample recorder's calls (`RecorderCalls`).  The drivers differ in the symbol prefix and in the last array of a fetch.  The library is looked
up through `_capi.lib()` at every call."""
import ctypes as C

import numpy as np

from . import _capi
from ._arrays import STATE_FIELDS, Staged, dp
from .state import StateBatch


class RecorderCalls:
    """Mixin of a driver with `_h`, `batch`, `topo`, _REC_API (the symbol prefix) and _REC_TAIL (shape of the fetch's last array behind [n, B])."""

    def _rec(self, op):
        return getattr(_capi.lib(), f"{self._REC_API}_{op}")

    def record_begin(self, period, capacity=128):
        _capi.check(self._rec("begin")(self._h, int(period), int(capacity)))

    def record_count(self) -> int:
        """Samples waiting to be fetched."""
        n = C.c_int64(0)
        _capi.check(self._rec("count")(self._h, C.byref(n)))
        return int(n.value)

    def record_end(self):
        _capi.check(self._rec("end")(self._h))

    def _record_fetch(self, max_samples):
        """(index [n], scalars [n, B, 5], heights, rates [n, B, n_nodes], post [n, B, 3], the last array [n, B, *_REC_TAIL])."""
        B, nn = self.batch, self.topo.n_nodes
        n = self.record_count() if max_samples is None else min(self.record_count(), int(max_samples))
        it = np.empty(n, np.int64)
        out = [np.empty((n, B) + s) for s in ((5,), (nn,), (nn,), (3,), self._REC_TAIL)]
        got = C.c_int64(0)
        _capi.check(self._rec("fetch")(self._h, n, C.byref(got), it.ctypes.data_as(C.POINTER(C.c_int64)), *[dp(a) for a in out]))
        if got.value != n:
            raise RuntimeError(f"record_fetch: asked for {n} samples, got {got.value}")
        return (it, *out)

    def _record_summary(self, skip, n, max_lag, per_chain, *extra):
        """(pooled, samples used, lag cap in force, per_chain or None); `extra`: the arrays the driver's call takes behind per_chain."""
        Q = C.c_int64(0)
        _capi.check(self._rec("quantities")(self._h, C.byref(Q)))
        Q = int(Q.value)
        count = self.record_count() - int(skip) if n is None else int(n)
        lag = min(int(max_lag), max(count, 0) // 2 - 1)
        lag = max(0, lag if lag % 2 == 1 else lag - 1)
        pooled = np.empty((Q, _capi.MCD_SUMMARY_COLS))
        pc = np.empty((self.batch, Q, 4)) if per_chain else None
        used = C.c_int64(0)
        _capi.check(self._rec("summary")(self._h, int(skip), -1 if n is None else int(n), lag, C.byref(used), dp(pooled),
                                         dp(pc) if per_chain else None, *[dp(a) for a in extra]))
        return pooled, int(used.value), lag, pc


class DriverCalls(_capi.OwnsHandle, RecorderCalls):
    """Base of a driver of `batch` chains over `topo` with the handle `_h`: _API is its symbol prefix ("mcd_mh", "mcd_hmc")."""

    def _create(self, tree_lik, *args):
        """<_API>_create, or <_API>_create_sparse for a bound tree over a precision matrix kept sparse on the device (`tree_lik.sparse`)."""
        self._h = C.c_void_p()
        create = getattr(_capi.lib(), self._API + ("_create_sparse" if tree_lik.sparse else "_create"))
        _capi.check(create(C.byref(self._h), tree_lik._t, *args))

    def set_state(self, s: StateBatch):
        """The states of all chains from host arrays: the seven fields, [batch, n_nodes] and [batch]."""
        st = Staged.state("set_state", None, s).check_state(self.topo.n_nodes, self.batch)
        _capi.check(getattr(_capi.lib(), self._API + "_set_state")(self._h, *[dp(a) for a in st.arrays], self.topo.n_nodes))

    def state(self) -> StateBatch:
        nn, B = self.topo.n_nodes, self.batch
        out = {f: np.empty((B, nn) if f in ("heights", "rates") else B) for f in STATE_FIELDS}
        _capi.check(getattr(_capi.lib(), self._API + "_get_state")(self._h, *[dp(a) for a in out.values()], nn))
        return StateBatch(**out)
