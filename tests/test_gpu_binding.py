"""The Python binding's one staging path on the device (mcmc_date_amd._arrays): inputs of a wrong shape, type, layout or place are refused
in Python -- none of them may reach a kernel or a host copy --, the handle goes on returning the same bits afterwards, host arrays and
CUDA tensors give the same bits, and the two drivers share their state code.  Nothing here depends on size: the smallest fixture, 5 chains
(a partial tile), and that fixture's precision matrix as an association list for the sparse classes."""
import dataclasses

import numpy as np
import pytest

import mcmc_date_amd as M

pytestmark = pytest.mark.gpu
B = 5
REFUSED = (ValueError, TypeError)        # (McdError, the C ABI's refusal, is neither)


class Case:
    def __init__(self, fx, gpu):
        import torch

        self.gpu = gpu
        self.topo = M.Topology(fx["parent"])
        self.nn = self.topo.n_nodes
        P, logdet = np.asarray(fx["sigma_inv"]), float(fx["logdet"])
        assoc = [((int(i), int(j)), float(P[i, j])) for i in range(P.shape[0]) for j in range(P.shape[1])]
        self.mvn = M.MvnLikelihood(M.Full(fx["mu"], P, logdet))
        self.sp = M.SparseLikelihood(M.Sparse(fx["mu"], assoc, logdet))
        self.tree = self.mvn.bind_tree(self.topo)
        self.sparse_tree = self.sp.bind_tree(self.topo)
        cal = [M.Calibration(f"c{i}", int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for i, r in enumerate(fx["cal"])]
        self.prior = M.PriorFunction(float(fx["prior_ht"]), "UncorrelatedGamma", cal, [], [], self.topo)
        self.host = M.StateBatch(fx["H"][:B].copy(), fx["R"][:B].copy(), fx["prior_tH"][:B].copy(), fx["rMu"][:B].copy(), fx["prior_birth"][:B].copy(),
                                 fx["prior_death"][:B].copy(), fx["prior_rvar"][:B].copy())
        self.dev = self.host.to(gpu)
        self.X = np.ascontiguousarray(fx["X"][:B])
        self.Xd = torch.as_tensor(self.X, device=gpu)
        # the calls on states: name -> (callable of a StateBatch, the state fields it reads)
        four = ("heights", "rates", "time_height", "rate_mean")
        seven = four + ("time_birth_rate", "time_death_rate", "rate_variance")
        self.state_calls = {"tree.loglik": (self.tree.loglik, four), "tree.grad": (self.tree.grad, four),
                            "sparse_tree.loglik": (self.sparse_tree.loglik, four), "sparse_tree.grad": (self.sparse_tree.grad, four),
                            "prior.logprior": (lambda s: self.prior.logprior(s, want_components=True), seven)}
        self.vector_calls = {"mvn.grad": self.mvn.grad, "sparse.grad": self.sp.grad}


@pytest.fixture(scope="module")
def case(gpu, golden):
    return Case(golden["06-leaves-constant-rate"], gpu)


def bits(out):
    """The arrays a call returned, on the host."""
    out = out if isinstance(out, tuple) else (out,)
    return [a if isinstance(a, np.ndarray) else a.cpu().numpy() for a in out if a is not None]


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def bad_states(case, fields):
    """(what is wrong, the state batch) for every field the call reads where the kind of fault applies."""
    import torch

    d = case.dev
    wide = torch.zeros(B, case.nn + 3, dtype=torch.float64, device=case.gpu)
    wide[:, :case.nn] = d.heights
    out = [("rates one column short", dataclasses.replace(d, rates=d.rates[:, :-1].contiguous())),
           ("heights one column short", dataclasses.replace(d, heights=d.heights[:, :-1].contiguous())),
           ("rates one row short", dataclasses.replace(d, rates=d.rates[:-1].contiguous())),
           ("heights not contiguous", dataclasses.replace(d, heights=wide[:, :case.nn]))]
    for f in fields:
        t = getattr(d, f)
        out.append((f"{f} float32", dataclasses.replace(d, **{f: t.float()})))
        out.append((f"{f} on the CPU (tensor)", dataclasses.replace(d, **{f: t.cpu()})))
        out.append((f"{f} on the CPU (numpy)", dataclasses.replace(d, **{f: t.cpu().numpy()})))
        if t.dim() == 1:
            out.append((f"{f} one element short", dataclasses.replace(d, **{f: t[:-1].contiguous()})))
            out.append((f"{f} one element long", dataclasses.replace(d, **{f: torch.cat([t, t[:1]])})))
    return out


@pytest.mark.parametrize("name", ["tree.loglik", "tree.grad", "sparse_tree.loglik", "sparse_tree.grad", "prior.logprior"])
def test_bad_device_states_are_refused_in_python(case, name):
    call, fields = case.state_calls[name]
    before = call(case.dev)
    assert all(np.all(np.isfinite(a)) for a in bits(before))
    for what, bad in bad_states(case, fields):
        with pytest.raises(REFUSED):
            call(bad)
            pytest.fail(f"{name}: {what} was accepted")
        assert same_bits(call(case.dev), before), (name, what)


@pytest.mark.parametrize("name", ["mvn.grad", "sparse.grad"])
def test_bad_device_vectors_are_refused_in_python(case, name):
    import torch

    call, Xd = case.vector_calls[name], case.Xd
    n = Xd.shape[1]
    before = call(Xd)
    wide = torch.zeros(B, n + 3, dtype=torch.float64, device=case.gpu)
    wide[:, :n] = Xd
    for what, bad in (("one column short", Xd[:, :-1].contiguous()), ("one column long", torch.cat([Xd, Xd[:, :1]], dim=1)), ("float32", Xd.float()),
                      ("not contiguous", wide[:, :n]), ("on the CPU", Xd.cpu()), ("one vector", Xd[0].contiguous()), ("three dimensions", Xd[None].contiguous())):
        with pytest.raises(REFUSED):
            call(bad)
            pytest.fail(f"{name}: X {what} was accepted")
        assert same_bits(call(Xd), before), (name, what)


def test_nodata_keeps_its_zeros(case):
    import torch

    nd = M.MvnLikelihood(M.NoData())
    ll = nd.logpdf(case.Xd)
    assert isinstance(ll, torch.Tensor) and ll.device == case.Xd.device and ll.dtype == torch.float64 and ll.shape == (B,) and bool((ll == 0).all())
    assert np.array_equal(nd.logpdf(case.X), np.zeros(B))
    tl = nd.bind_tree(case.topo)
    ll, lj = tl.loglik(case.dev)
    assert lj is None and isinstance(ll, torch.Tensor) and ll.shape == (B,) and bool((ll == 0).all())
    ll, lj = tl.loglik(case.host)
    assert lj is None and np.array_equal(ll, np.zeros(B))
    for call in (lambda: nd.grad(case.X), lambda: tl.grad(case.host)):
        with pytest.raises(ValueError, match="NoData has no gradient path"):
            call()


@pytest.mark.parametrize("name", ["tree.grad", "sparse_tree.loglik", "sparse_tree.grad", "prior.logprior", "sparse.grad"])
def test_host_and_device_agree_bit_for_bit(case, name):
    """(MvnLikelihood.logpdf / grad, TreeLikelihood.loglik, SparseLikelihood.logpdf and the ln prior itself: test_gpu_parity.py,
    test_gpu_sparse.py and test_gpu_prior.py assert the same beside their parity checks.)"""
    import torch

    if name in case.vector_calls:
        call, host, dev = case.vector_calls[name], case.X, case.Xd
    else:
        call, host, dev = case.state_calls[name][0], case.host, case.dev
    on_host, on_dev = call(host), call(dev)
    assert all(isinstance(a, np.ndarray) for a in on_host) and all(isinstance(a, torch.Tensor) and a.device == case.Xd.device for a in on_dev)
    assert len(on_host) == {"tree.grad": 5, "sparse_tree.loglik": 2, "sparse_tree.grad": 5, "prior.logprior": 2, "sparse.grad": 2}[name]
    assert same_bits(on_host, on_dev)


def driver_state(case, n):
    s = case.host.slice(0, n)
    return M.StateBatch(**{f.name: np.array(getattr(s, f.name)) for f in dataclasses.fields(s)})


@pytest.mark.parametrize("driver", ["Sampler", "Leapfrog"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_drivers_round_trip_their_state(case, driver, sparse):
    tl = case.sparse_tree if sparse else case.tree
    assert tl.sparse is sparse
    if driver == "Sampler":
        ps, _ = M.proposals(case.topo, [], calibrations_available=True)
        d = M.Sampler(tl, case.prior, ps, 3, seed=1)
    else:
        d = M.Leapfrog(tl, case.prior, True, 3)
    s = driver_state(case, 3)
    d.set_state(s)
    got = d.state()
    for f in dataclasses.fields(s):
        a, b = getattr(s, f.name), getattr(got, f.name)
        assert isinstance(b, np.ndarray) and b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b), f.name
    # a sparse bound tree took the sparse constructor: the dense one refuses it (and the other way round) -- the handle would not exist
    assert d._h.value
    # float32 and non-contiguous host arrays are converted, as before
    wide = np.zeros((3, 2 * case.nn))
    wide[:, ::2] = s.heights
    d.set_state(dataclasses.replace(s, heights=wide[:, ::2], time_height=list(s.time_height)))
    assert np.array_equal(d.state().heights, s.heights) and np.array_equal(d.state().time_height, s.time_height)
    d.close()
    d.close()
    assert not d._h.value


def test_leapfrog_refuses_what_the_sampler_refuses(case):
    s = driver_state(case, 3)
    bad = [("time_birth_rate missing", dataclasses.replace(s, time_birth_rate=None)), ("rate_variance missing", dataclasses.replace(s, rate_variance=None))]
    for f in ("time_birth_rate", "time_death_rate", "time_height", "rate_mean", "rate_variance"):
        bad.append((f"{f} short", dataclasses.replace(s, **{f: getattr(s, f)[:-1]})))
    bad += [("rates one column short", dataclasses.replace(s, rates=s.rates[:, :-1])), ("heights one row short", dataclasses.replace(s, heights=s.heights[:-1])),
            ("a batch of another size", driver_state(case, 4)), ("tensors on the device", case.dev.slice(0, 3))]
    ps, _ = M.proposals(case.topo, [], calibrations_available=True)
    for d in (M.Leapfrog(case.tree, case.prior, True, 3), M.Sampler(case.tree, case.prior, ps, 3, seed=1)):
        d.set_state(s)
        for what, b in bad:
            with pytest.raises(REFUSED):
                d.set_state(b)
                pytest.fail(f"{type(d).__name__}.set_state: {what} was accepted")
            assert np.array_equal(d.state().rate_variance, s.rate_variance) and np.array_equal(d.state().heights, s.heights), what
    # the prior's gradient is a host call like the drivers' set_state
    lp, g = case.prior.grad(case.host)
    assert lp.shape == (B,) and sorted(g) == sorted(f.name for f in dataclasses.fields(s)) and g["heights"].shape == (B, case.nn)
    with pytest.raises(REFUSED):
        case.prior.grad(case.dev)
    with pytest.raises(REFUSED):
        case.prior.grad(dataclasses.replace(case.host, time_death_rate=case.host.time_death_rate[:-1]))
    lp2, g2 = case.prior.grad(case.host)
    assert np.array_equal(lp2, lp, equal_nan=True) and all(np.array_equal(g2[k], g[k], equal_nan=True) for k in g)
