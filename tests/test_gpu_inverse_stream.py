"""The inverse factor stream of the column sweep (k_logpdf.hip, FS = 3): z = W (x - mu) with W = L^-1 streamed through the LDS-DMA ring in
the compact layout, every column's broadcast taken from the residual registers instead of from the running substitution.  It is
another algebra, so it is held to the substitution sweep by tolerance (1e-12 relative, the bound between forms) and to the CPU oracle
by the project's bound for synthetic problems; everything else -- batch independence, host against device-resident input, graph
replay, two loader waves, non-finite inputs -- is bit for bit.  mcd_set_option("MCD_FSTREAM", 3) forces the stream in the
two-compute-wave geometry; without the knob it is the default for 240 < N <= 256 at 129 .. 512 chains under form "auto"."""
import ctypes as C
import functools

import numpy as np
import pytest

import mcmc_date_amd as M
import oracle as O
from mcmc_date_amd import synthetic as S

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CHAINS = (1, 3, 5)                        # an odd batch leaves one compute wave of the last workgroup on clamped input
LN_SQRT_2PI = 0.9189385332046727


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@functools.lru_cache(maxsize=None)
def problem(n, batch):
    """operands, chains, the oracle's values and the bound 64 N eps cond(Sigma) max(1, q) of tests/test_gpu_parity.py"""
    mu, sigma = S.random_spd_problem(n, seed=5 * n)
    P = np.linalg.inv(sigma)
    logdet = np.linalg.slogdet(sigma)[1]
    X = S.sample_chains(mu, sigma, batch, seed=n + 1)
    ref = O.logpdf_full_batch(mu, P, logdet, X)
    q = -2.0 * (ref + LN_SQRT_2PI * n) - logdet
    return mu, sigma, X, ref, 64 * n * EPS * np.linalg.cond(sigma) * np.maximum(1.0, q)


def stream_of(n, form, batch):
    f = C.CDLL(M._capi.LIB_PATH).mcd_stream_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64]
    return f(n, (n + 63) // 64, {"auto": 0, "sweep": 1}[form], 1, 1, batch)


def on_sweep(lik, fn):
    """fn() with the handle pinned to form "sweep": the substitution stream, or whatever MCD_FSTREAM asks for"""
    lik.set_form("sweep")
    try:
        return fn()
    finally:
        lik.set_form("auto")


def check_bounds(inv, sub, ref, tol, tag):
    print(tag, "max |inv - oracle|", np.abs(inv - ref).max(), "bound", tol.min(), "max rel inv - substitution", rel(inv, sub).max())
    assert np.all(np.abs(inv - ref) <= tol), (tag, np.abs(inv - ref).max(), tol.min())
    assert np.max(rel(inv, sub)) <= 1e-12, (tag, rel(inv, sub).max())


# 1. the knob: the first dimension of R = 3, sweeps that stop before the last chunks (140, 200), the window's N, a full R = 4
@pytest.mark.parametrize("n", [129, 140, 200, 241, 255, 256])
def test_knob_forced_stream(gpu, n, knobs):
    mu, sigma, X, ref, tol = problem(n, max(CHAINS))
    lik = M.MvnLikelihood.from_covariance(mu, sigma)
    sub = on_sweep(lik, lambda: [np.asarray(lik.logpdf(X[:B])) for B in CHAINS])
    knobs.setenv("MCD_FSTREAM", "3")
    assert stream_of(n, "sweep", max(CHAINS)) == 3
    inv = on_sweep(lik, lambda: [np.asarray(lik.logpdf(X[:B])) for B in CHAINS])
    for i, B in enumerate(CHAINS):
        check_bounds(inv[i], sub[i], ref[:B], tol[:B], (n, B))
        assert np.array_equal(bits(inv[i]), bits(inv[-1][:B]))          # a chain's value does not depend on the batch


# 2. the window in which the stream is the default
@pytest.mark.parametrize("n,batch", [(241, 129), (256, 130), (256, 512)])
def test_auto_window(gpu, n, batch):
    import torch

    mu, sigma, X, ref, tol = problem(n, 512)
    X, ref, tol = X[:batch], ref[:batch], tol[:batch]
    lik = M.MvnLikelihood.from_covariance(mu, sigma)
    assert stream_of(n, "auto", batch) == 3
    ll = np.asarray(lik.logpdf(X))                                       # host pointer
    sub = on_sweep(lik, lambda: np.asarray(lik.logpdf(X)))
    check_bounds(ll, sub, ref, tol, (n, batch))
    if batch == 512:
        assert not np.array_equal(bits(ll), bits(sub))                   # really the other stream
        assert np.array_equal(bits(lik.logpdf(X[:200])), bits(ll[:200]))
    assert np.array_equal(bits(lik.logpdf(X)), bits(ll))                 # twice in a row
    ld = n + 3                                                           # device-resident, padded leading dimension
    Xd = torch.full((batch, ld), np.nan, dtype=torch.float64, device=gpu)
    Xd[:, :n] = torch.as_tensor(X, device=gpu)
    out = torch.zeros(batch, dtype=torch.float64, device=gpu)
    for _ in range(2):
        out.zero_()
        M._capi.check(M._capi.lib().mcd_mvn_logpdf_batch(lik._h, Xd.data_ptr(), ld, batch, 1, None, out.data_ptr()))
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(ll))


# 3. outside the window the choice did not move
@pytest.mark.parametrize("n,batch", [(256, 128), (256, 513), (240, 512), (200, 256)])
def test_outside_window(gpu, n, batch, knobs):
    mu, sigma, X, ref, tol = problem(n, 513 if batch == 513 else 512)
    X = X[:batch]
    lik = M.MvnLikelihood.from_covariance(mu, sigma)
    ll = np.asarray(lik.logpdf(X))
    assert np.all(np.abs(ll - ref[:batch]) <= tol[:batch])
    if (n, batch) == (256, 128):                                         # the row split's batch
        assert stream_of(n, "auto", batch) == -1
        knobs.setenv("MCD_SPLIT", "1")
        assert np.array_equal(bits(lik.logpdf(X)), bits(ll))
    else:
        assert stream_of(n, "auto", batch) == (0 if batch == 513 else 2)
        assert np.array_equal(bits(on_sweep(lik, lambda: lik.logpdf(X))), bits(ll))


# 4. W from the reverse Cholesky factor of an ill-conditioned precision matrix (tests/test_gpu_parity.py's construction)
def test_ill_conditioned_precision_matrix_inverse_stream(gpu):
    n, batch = 256, 200
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, 9.0, n)
    P = (Q * lam) @ Q.T
    P = 0.5 * (P + P.T)
    logdet = -float(np.sum(np.log(lam)))                 # log det Sigma
    mu = rng.uniform(0.01, 1.0, n)
    X = mu + rng.standard_normal((batch, n)) * 1e-3
    Pl, dxl = P.astype(np.longdouble), (X - mu).astype(np.longdouble)
    q_ref = np.einsum("bi,ij,bj->b", dxl, Pl, dxl)
    ll_ref = (-LN_SQRT_2PI * n - 0.5 * (np.longdouble(logdet) + q_ref)).astype(np.float64)
    lik = M.MvnLikelihood(M.Full(mu, P, logdet))
    assert stream_of(n, "auto", batch) == 3
    ll = np.asarray(lik.logpdf(X))
    q = -2.0 * (ll + LN_SQRT_2PI * n) - logdet
    eq = np.max(np.abs(q - q_ref.astype(np.float64)) / q_ref.astype(np.float64))
    el = np.max(np.abs(ll - ll_ref) / np.abs(ll_ref))
    print("ill-conditioned: q", eq, "ll", el)
    assert eq <= 1e-9 and el <= 1e-9


# 5. the counted waits of a loader wave of two
def test_two_loader_waves_inverse_stream(gpu, knobs):
    mu, sigma, X, _, _ = problem(256, 512)
    lik = M.MvnLikelihood.from_covariance(mu, sigma)
    four = np.asarray(lik.logpdf(X))
    knobs.setenv("MCD_FSTREAM", "3")
    four_few = on_sweep(lik, lambda: np.asarray(lik.logpdf(X[:3])))
    knobs.setenv("MCD_LOADERS", "2")
    two_few = on_sweep(lik, lambda: np.asarray(lik.logpdf(X[:3])))
    knobs.delenv("MCD_FSTREAM")
    two = np.asarray(lik.logpdf(X))
    assert np.array_equal(bits(two), bits(four)) and np.array_equal(bits(two_few), bits(four_few))
    assert np.array_equal(bits(four_few), bits(four[:3]))


# 6. a non-finite x makes its own chain non-finite and leaves the others alone
def test_non_finite_inverse_stream(gpu, knobs):
    mu, sigma, X, _, _ = problem(256, 512)
    lik = M.MvnLikelihood.from_covariance(mu, sigma)
    Xb = X.copy()
    Xb[2, 100] = np.inf
    Xb[7, 0] = np.nan
    Xb[300, 255] = -np.inf
    Xb[511, :] = np.inf
    poisoned = [2, 7, 300, 511]
    keep = np.setdiff1d(np.arange(512), poisoned)
    good, bad = np.asarray(lik.logpdf(X)), np.asarray(lik.logpdf(Xb))   # the window's default
    assert np.isfinite(good).all() and not np.isfinite(bad[poisoned]).any()
    assert np.array_equal(bits(bad[keep]), bits(good[keep]))
    knobs.setenv("MCD_FSTREAM", "3")
    few = on_sweep(lik, lambda: np.asarray(lik.logpdf(Xb[:5])))
    assert not np.isfinite(few[2]) and np.array_equal(bits(few[[0, 1, 3, 4]]), bits(good[[0, 1, 3, 4]]))


# 7. graph replay, two alternating batches, the knob at three chains (tests/test_gpu_prologue.py covers the default at 256 x 512)
def test_graph_replay_alternating_batches_inverse_stream(gpu, knobs):
    import torch

    n, B = 256, 3
    mu, sigma, X0, _, _ = problem(n, 512)
    X0 = X0[:B]
    X1 = X0 + 0.125 * np.sqrt(np.diag(sigma))                           # shifted inputs
    lik = M.MvnLikelihood.from_covariance(mu, sigma, device=0)
    knobs.setenv("MCD_FSTREAM", "3")
    lik.set_form("sweep")
    X = [torch.as_tensor(x, device=gpu) for x in (X0, X1)]
    eager = [lik.logpdf(x).cpu().numpy() for x in X]
    assert not np.array_equal(bits(eager[0]), bits(eager[1]))
    ll = [torch.zeros(B, dtype=torch.float64, device=gpu) for _ in range(2)]
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        lik.logpdf_into(X[0], ll[0])
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        for i in range(50):
            lik.logpdf_into(X[i & 1], ll[i & 1])
    for rep in range(4):
        for o in ll:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for i in range(2):
            assert np.array_equal(bits(ll[i].cpu().numpy()), bits(eager[i])), (rep, i)
    knobs.delenv("MCD_FSTREAM")
    lik.set_form("auto")
    sub = on_sweep(lik, lambda: np.asarray(lik.logpdf(X0)))
    assert np.max(rel(eager[0], sub)) <= 1e-12
