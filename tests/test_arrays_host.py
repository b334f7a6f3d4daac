"""The binding's array plumbing on host arrays (mcmc_date_amd._arrays; no device): what `Staged` makes of the operands of a batched call,
the shape checks every public method shares, the source of a device-side reduction, and the handle-lifetime mixin on a stub library."""
import ctypes as C
import gc

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _arrays as A
from mcmc_date_amd import _capi

B, NN = 5, 11


def state(**over):
    rng = np.random.default_rng(0)
    f = dict(heights=rng.random((B, NN)), rates=rng.random((B, NN)), time_height=rng.random(B), rate_mean=rng.random(B),
             time_birth_rate=rng.random(B), time_death_rate=rng.random(B), rate_variance=rng.random(B))
    f.update(over)
    return M.StateBatch(**f)


def test_host_operands_come_out_contiguous_float64():
    wide = np.arange(B * 2 * NN, dtype=np.float32).reshape(B, 2 * NN)
    X = wide[:, ::2]                                           # float32, not contiguous
    s = A.Staged("logpdf", 0, X=X).check_matrix(NN)
    Xs, = s.arrays
    assert Xs.dtype == np.float64 and Xs.flags.c_contiguous and np.array_equal(Xs, X)
    assert (s.on_device, s.stream, s.batch) == (0, None, B) and s["X"] is Xs and s.names == ("X",)
    assert A._ptr(Xs).value == Xs.ctypes.data and [p.value for p in s.pointers()] == [Xs.ctypes.data]
    # array-likes, and a state whose fields are lists / float32
    assert A.Staged("logpdf", 0, X=[[1, 2], [3, 4], [5, 6]]).check_matrix(2).batch == 3
    st = state()
    st.heights, st.time_height = st.heights.astype(np.float32), list(st.time_height)
    s = A.Staged.state("logprior", 0, st).check_state(NN)
    assert s.names == A.STATE_FIELDS and s.batch == B and all(a.dtype == np.float64 and a.flags.c_contiguous for a in s.arrays)
    assert np.array_equal(s["heights"], st.heights) and np.array_equal(s["time_height"], st.time_height)
    assert A.Staged.state("loglik", 0, state(), A.LIKELIHOOD_FIELDS).check_state(NN).names == ("heights", "rates", "time_height", "rate_mean")


def test_matrix_shapes_are_refused():
    for X, n in ((np.zeros(NN), NN), (np.zeros((B, NN + 1)), NN), (np.zeros((B, NN - 1)), NN), (np.zeros((2, B, NN)), NN), (np.zeros(NN), None)):
        with pytest.raises(ValueError, match=r"grad: X must be \[batch, n\]"):
            A.Staged("grad", 0, X=X).check_matrix(n)
    assert A.Staged("logpdf", 0, X=np.zeros((B, 3))).check_matrix(None).batch == B       # (NoData: any width)


@pytest.mark.parametrize("field", A.STATE_FIELDS)
def test_each_state_field_is_checked(field):
    good = getattr(state(), field)
    wrong = [good[:-1], good[..., None]] + ([good[:, :-1], good[:, 0]] if good.ndim == 2 else [np.stack([good, good], axis=1)])
    for bad in wrong:
        with pytest.raises(ValueError, match="set_state: inconsistent state shapes"):
            A.Staged.state("set_state", None, state(**{field: bad})).check_state(NN, B)
        with pytest.raises(ValueError, match="logprior: inconsistent state shapes"):       # (no batch given: the rows of heights are the batch)
            A.Staged.state("logprior", 0, state(**{field: bad})).check_state(NN)
    # a batch that is consistent in itself but not the driver's
    with pytest.raises(ValueError, match="inconsistent state shapes"):
        A.Staged.state("set_state", None, state()).check_state(NN, B + 1)
    with pytest.raises(ValueError, match="inconsistent state shapes"):
        A.Staged.state("set_state", None, state()).check_state(NN + 1, B)


@pytest.mark.parametrize("field", ["time_birth_rate", "time_death_rate", "rate_variance"])
def test_a_missing_state_field_is_refused(field):
    with pytest.raises(ValueError, match=f"set_state: the state batch lacks {field}"):
        A.Staged.state("set_state", None, state(**{field: None}))
    assert A.Staged.state("loglik", 0, state(**{field: None}), A.LIKELIHOOD_FIELDS).check_state(NN).batch == B
    st = state()
    with pytest.raises(ValueError, match="lacks time_birth_rate / time_death_rate / rate_variance"):
        A.Staged.state("logprior", 0, M.StateBatch(st.heights, st.rates, st.time_height, st.rate_mean))


def test_two_d_fields_of_different_widths_are_refused():
    st = state()
    for over in (dict(rates=np.zeros((B, NN + 2))), dict(heights=np.zeros((B, NN + 2))), dict(heights=np.zeros((B, NN + 2)), rates=np.zeros((B, NN + 2)))):
        with pytest.raises(ValueError, match="inconsistent state shapes"):
            A.Staged.state("loglik", 0, state(**over), A.LIKELIHOOD_FIELDS).check_state(NN)
    assert A.Staged.state("loglik", 0, st, A.LIKELIHOOD_FIELDS).check_state(NN).batch == B


def test_row_stride_and_output_kinds():
    s = A.Staged.state("grad", 0, state(), A.LIKELIHOOD_FIELDS).check_state(NN)
    H = s["heights"]
    assert s.ld(H) == NN and s.ld(np.zeros((3, 7))) == 7
    for out, shape in ((s.empty(B), (B,)), (s.empty(B, 3), (B, 3)), (s.zeros(B), (B,)), (s.empty_like(H), (B, NN)), (s.empty_like(s["time_height"]), (B,))):
        assert type(out) is np.ndarray and out.dtype == np.float64 and out.shape == shape and out.flags.c_contiguous
    assert np.all(s.zeros(B) == 0.0)
    # a host-only call (device None) never becomes a device call; a device call refuses a host array beside a tensor
    import torch

    t = torch.arange(6, dtype=torch.float32).reshape(3, 2)
    s = A.Staged("set_state", None, X=t).check_matrix(2)
    assert s.on_device == 0 and type(s.arrays[0]) is np.ndarray and s.arrays[0].dtype == np.float64
    with pytest.raises(TypeError, match="Y is a host array"):
        A.Staged("logpdf", 0, Y=np.zeros(3), X=t)
    with pytest.raises(TypeError, match="X: need a contiguous float64 CUDA tensor"):
        A.Staged("logpdf", 0, X=t)                             # a tensor that is not on a GPU


def test_reduction_source():
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    ptr, on_device, dev, shape = A.reduction_source(x[:, :, ::2], 3, True, "trace_summary", "[n, B, ldq]")
    assert (on_device, dev, shape) == (0, 0, (2, 3, 2))
    got = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(12,))          # the pointer keeps the float64 copy alive
    gc.collect()
    assert np.array_equal(got.reshape(shape), x[:, :, ::2])
    assert A.reduction_source(np.zeros((4, 6)), 2, 3, "marginal_likelihood_device", "[n, batch]")[1:] == (0, 3, (4, 6))
    for a, ndim in ((np.zeros(6), 2), (np.zeros((2, 3, 4)), 2), (np.zeros((2, 3)), 3), (np.zeros((2, 3, 4, 5)), 3), (1.0, 2)):
        with pytest.raises(ValueError, match=r"what: expected \[shape\]"):
            A.reduction_source(a, ndim, True, "what", "[shape]")
    import torch

    with pytest.raises(ValueError, match=r"what: expected a contiguous float64 GPU tensor \[shape\]"):
        A.reduction_source(torch.zeros(2, 3, dtype=torch.float64), 2, True, "what", "[shape]")      # on the host
    # the two public functions keep their messages
    with pytest.raises(ValueError, match=r"trace_summary: expected \[n, B, ldq\]"):
        M.diagnostics.trace_summary(np.zeros((4, 6)))
    with pytest.raises(ValueError, match=r"marginal_likelihood_device: expected \[n, batch\]"):
        M.diagnostics.marginal_likelihood_device(np.zeros(6), [0.0, 1.0])


def test_handle_is_destroyed_exactly_once(monkeypatch):
    destroyed = []

    class Lib:
        def stub_destroy(self, h):
            destroyed.append(h.value)

    monkeypatch.setattr(_capi, "lib", lambda: Lib())

    class Owner(_capi.OwnsHandle):
        _HANDLE = ("_t", "stub_destroy")

        def __init__(self, value):
            if value is not None:
                self._t = C.c_void_p(value)

    o = Owner(1234)
    o.close()
    o.close()
    assert destroyed == [1234] and o._t.value is None
    del o
    gc.collect()
    assert destroyed == [1234]
    Owner(77)                                                  # never closed: the destructor does it
    gc.collect()
    assert destroyed == [1234, 77]
    for never_created in (Owner(0), Owner(None)):              # a null handle, and an object whose constructor failed before the handle
        never_created.close()
    del never_created
    gc.collect()
    assert destroyed == [1234, 77]
    # every owner in the package names an attribute it has and a symbol of the C ABI
    from mcmc_date_amd import hmc, likelihood, prior, sampler
    owners = (likelihood.MvnLikelihood, likelihood.TreeLikelihood, likelihood.SparseLikelihood, likelihood.SparseTreeLikelihood,
              prior.PriorFunction, sampler.Sampler, hmc.Leapfrog)
    assert [cls._HANDLE[0] for cls in owners] == ["_h", "_t", "_h", "_t", "_p", "_h", "_h"]
    assert all(cls._HANDLE[1] in _capi.SYMBOLS and cls._HANDLE[1].endswith("_destroy") for cls in owners)
    assert len({cls._HANDLE[1] for cls in owners}) == 7
