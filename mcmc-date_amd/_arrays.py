"""Array plumbing of the binding: everything that turns numpy arrays or torch CUDA tensors into the arguments of one C call
(include/mcmcdate_mvn.h) lives here -- the pointer helpers, `Staged` (the operands of one batched call with their shape checks, written
once for host and device arrays) and `reduction_source` (the input of a device-side reduction)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def _host(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    if _is_torch(a):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _stream_ptr(dev_index: int):
    import torch

    return C.c_void_p(torch.cuda.current_stream(dev_index).cuda_stream)


def _check_cuda(t, device: int, name: str):
    import torch

    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise TypeError(f"{name}: need a contiguous float64 CUDA tensor")
    if t.device.index != device:
        raise ValueError(f"{name}: tensor is on cuda:{t.device.index}, likelihood lives on cuda:{device}")


def ip(a):
    """int32 numpy array -> const int32_t*."""
    return a.ctypes.data_as(_capi._ip)


def dp(a):
    """float64 numpy array -> double*."""
    return a.ctypes.data_as(_capi._dp)


# the seven fields of a state in the order the C ABI takes them, and the four the likelihood reads
STATE_FIELDS = ("time_birth_rate", "time_death_rate", "time_height", "heights", "rate_mean", "rate_variance", "rates")
LIKELIHOOD_FIELDS = ("heights", "rates", "time_height", "rate_mean")


class Staged:
    """The named input arrays of one batched call, staged once: a HOST call (numpy arrays or array-likes, made contiguous float64;
    on_device 0, stream None: the library copies, evaluates and returns synchronously) or a DEVICE call (every operand a contiguous
    float64 CUDA tensor on `device`; on_device 1, torch's current stream of that device: enqueued, not synchronised).  A mixture is
    refused.  device None: a host-only call -- everything goes through numpy, which refuses CUDA tensors itself.
    `what` is the calling method's name, for the messages."""

    def __init__(self, what: str, device, **arrays):
        self.what, self.names = what, tuple(arrays)
        self.on_device = int(device is not None and any(_is_torch(a) for a in arrays.values()))
        self.stream = None
        if self.on_device:
            for name, a in arrays.items():
                if not _is_torch(a):
                    raise TypeError(f"{what}: {name} is a host array, the other operands are torch tensors")
                _check_cuda(a, device, name)
            self.stream = _stream_ptr(device)
            self.arrays = list(arrays.values())
        else:
            self.arrays = [_host(a) for a in arrays.values()]
        self.batch = None            # set by the shape check

    @classmethod
    def state(cls, what: str, device, s, fields=STATE_FIELDS) -> "Staged":
        """The `fields` of a StateBatch, none of them missing."""
        missing = [f for f in fields if getattr(s, f) is None]
        if missing:
            raise ValueError(f"{what}: the state batch lacks " + " / ".join(missing))
        return cls(what, device, **{f: getattr(s, f) for f in fields})

    def __getitem__(self, name):
        return self.arrays[self.names.index(name)]

    def pointers(self):
        return [_ptr(a) for a in self.arrays]

    # -- the shape checks, for both kinds --------------------------------------------------------------------------------------
    def check_matrix(self, n=None) -> "Staged":
        """The one operand is [batch, n] (n None: any width)."""
        X, = self.arrays
        if X.ndim != 2 or (n is not None and X.shape[1] != n):
            raise ValueError(f"{self.what}: {self.names[0]} must be [batch, n]")
        self.batch = int(X.shape[0])
        return self

    def check_state(self, n_nodes: int, batch=None) -> "Staged":
        """heights and rates are [B, n_nodes] with one row stride, every other field [B]; B = `batch`, or the rows of heights."""
        H, R = self["heights"], self["rates"]
        B = int(H.shape[0]) if batch is None and H.ndim == 2 else batch
        for name, a in zip(self.names, self.arrays):
            if tuple(a.shape) != ((B, n_nodes) if name in ("heights", "rates") else (B,)):
                raise ValueError(f"{self.what}: inconsistent state shapes")
        if self.ld(H) != self.ld(R):
            raise ValueError(f"{self.what}: heights and rates must share one row stride")
        self.batch = B
        return self

    # -- what the methods need -------------------------------------------------------------------------------------------------
    def ld(self, a) -> int:
        """Row stride of a 2-D operand, in elements."""
        return int(a.stride(0)) if self.on_device else int(a.shape[1])

    def empty(self, *shape):
        if self.on_device:
            import torch

            return torch.empty(*shape, dtype=torch.float64, device=self.arrays[0].device)
        return np.empty(shape)

    def zeros(self, *shape):
        if self.on_device:
            import torch

            return torch.zeros(*shape, dtype=torch.float64, device=self.arrays[0].device)
        return np.zeros(shape)

    def empty_like(self, a):
        if self.on_device:
            import torch

            return torch.empty_like(a)
        return np.empty_like(a)


def reduction_source(a, ndim: int, device, what: str, shape: str):
    """The input of a device-side reduction: a numpy array of `ndim` dimensions (the library copies it to device 0, or to `device` if that
    is an int), or a contiguous float64 GPU tensor, read in place after its stream is synchronised.  Returns (pointer, on_device, device
    index, shape); the pointer keeps a host array alive."""
    if hasattr(a, "data_ptr"):
        if not a.is_cuda or not a.is_contiguous() or str(a.dtype) != "torch.float64" or a.dim() != ndim:
            raise ValueError(f"{what}: expected a contiguous float64 GPU tensor {shape}")
        import torch

        torch.cuda.current_stream(a.device).synchronize()
        return C.c_void_p(a.data_ptr()), 1, a.device.index or 0, tuple(int(s) for s in a.shape)
    a = _host(a)
    if a.ndim != ndim:
        raise ValueError(f"{what}: expected {shape}")
    return a.ctypes.data_as(C.c_void_p), 0, 0 if device is True else int(device), tuple(int(s) for s in a.shape)
