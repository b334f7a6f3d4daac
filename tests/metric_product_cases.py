"""Inputs, references and bounds shared by tests/test_metric_product_host.py, tests/test_gpu_metric_gemm.py and tests/test_gpu_hmc_cov.py:
what the product kernel of the across-chains dense metric (csrc/k_metric_gemm.hip) and the covariance kernels of the dense warm-up
(csrc/k_hmc_cov.hip) must deliver.  numpy only; references and bounds in np.longdouble (64 bits of mantissa), gamma_k = k 2^-53 / (1 - k 2^-53).

Product, componentwise (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: holds for any order of summation, with or
without fused multiply-adds, so also for whatever the matrix cores do inside four terms; no margin, from the inputs alone):

    |Y - X A|_rk <= gamma_dim (|X| |A|)_rk

Covariance of n samples Q [n][dim] by two passes, one accumulator per entry.  With m the exact mean, d = Q - m,
S_ij = sum_s |d_si| |d_sj| / n, a_i = sum_s |d_si| / n and e_k = gamma_{n+3} max_s |Q[s][k]| (the fp64 mean's error, gamma_n + 2^-53, plus one
rounded subtraction):

    |mean_k - m_k| <= gamma_n sum_s |Q_sk| / n + 2^-53 |m_k|
    |cov_ij - C_ij| <= tol_ij = gamma_{n+2} S_ij + (1 + gamma_{n+2}) (a_i e_j + a_j e_i + e_i e_j)

(n products and additions and one division: gamma_{n+2} on the sum of the computed centred values' products; each computed centred value is
within e of the exact one.)  The inputs must leave the bound sharp enough to tell a two-pass sum from a sum of squares: check_cov asserts,
on the reference alone, tol_ij <= 1e-12 sqrt(C_ii C_jj) on ordinary columns and <= 1e-6 sqrt(C_ii C_jj) on entries that touch an offset
column (a mean thousands of standard deviations from 0)."""
import numpy as np

from metric_factor_cases import gamma, need_long_double

LD = np.longdouble
MARK = 7.25                                          # what an untouched output holds (the suite's convention)


# ---- the product ----------------------------------------------------------------------------------------------------------------------
def int_inputs(rows, dim, seed=0):
    """X [rows][dim] and A [dim][dim] of integers in [-512, 512]: every sum stays below 516 x 2^18 < 2^28, exact in fp64 in any order."""
    rng = np.random.default_rng(100000 * seed + 1000 * rows + dim)
    X = rng.integers(-512, 513, size=(rows, dim))
    A = rng.integers(-512, 513, size=(dim, dim))
    return X.astype(np.float64), A.astype(np.float64)


def int_product(X, A):
    """X A of integer-valued fp64 arrays, in int64."""
    Xi, Ai = X.astype(np.int64), A.astype(np.int64)
    assert np.array_equal(Xi, X) and np.array_equal(Ai, A)
    P = Xi @ Ai
    assert np.abs(P).max(initial=0) < 2 ** 28
    return P


def real_rows(rows, dim, seed=0):
    """X [rows][dim]: standard normal entries with a scale per row and per column (a few decades), no zeros."""
    rng = np.random.default_rng(200000 * seed + 1000 * rows + dim)
    return rng.standard_normal((rows, dim)) * np.exp(rng.standard_normal((rows, 1))) * np.exp(2.0 * rng.standard_normal(dim))


def product_ratio(Y, X, A):
    """max over entries of |Y - X A| / (gamma_dim |X| |A|) (0 where the bound is 0 and met), the references in long double."""
    need_long_double()
    Xl, Al = X.astype(LD), A.astype(LD)
    err = np.abs(Y.astype(LD) - Xl @ Al)
    bound = gamma(X.shape[1]) * (np.abs(Xl) @ np.abs(Al))
    assert np.all(np.isfinite(bound))
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    return float(np.max(ratio))


def check_product(Y, X, A, label):
    """The componentwise product bound; prints the worst error / bound."""
    assert Y.shape == X.shape and np.all(np.isfinite(Y)), label
    ratio = product_ratio(Y, X, A)
    print(f"{label}: |Y - X A| / bound {ratio:.3f}")
    assert ratio <= 1.0, (label, ratio)
    return ratio


def list_rows(lst, slots, stride):
    """Memory rows of the product rows 0 .. slots n_list - 1 through the list: (r // n_list) stride + lst[r % n_list]."""
    lst = np.asarray(lst, np.int64)
    return (np.arange(slots)[:, None] * stride + lst[None, :]).ravel()


def listed_product(X, A, Y0, lst, rows, stride):
    """What a launch through the list must leave: Y0 with the memory rows of the `rows` product rows replaced by their rows of X A (numpy's
    fp64 product: exact on int_inputs).  The other rows of X are not looked at."""
    n_list = len(lst)
    Y = Y0.copy()
    for r in range(rows):
        m = (r // n_list) * stride + int(lst[r % n_list])
        Y[m] = X[m] @ A
    return Y


def check_listed(Y, X, A, lst, slots, stride, label):
    """Y after a launch of slots x n_list rows through the list from Y0 = MARK everywhere, X and A from int_inputs (unlisted rows of X may
    hold anything): the listed rows are the exact product, every other row still holds the mark."""
    mem = list_rows(lst, slots, stride)
    assert len(set(mem.tolist())) == mem.size and mem.max() < Y.shape[0], label
    want = np.full(Y.shape, MARK)
    want[mem] = int_product(X[mem], A)
    bad = np.flatnonzero(np.any(Y != want, axis=1))
    assert bad.size == 0, (label, "rows that differ", bad[:8].tolist(), "listed" if np.isin(bad[0], mem) else "unlisted")


# ---- the covariance -------------------------------------------------------------------------------------------------------------------
def cov_inputs(n, dim, seed=0):
    """(Q [n][dim], offset columns): standard normal columns scaled by exp(N(0, 1)); from dim 3 on, column dim // 3 is 1e6 + N(0, 1) and
    column (2 dim) // 3 has its mean at -3000 standard deviations."""
    rng = np.random.default_rng(300000 * seed + 1000 * n + dim)
    Q = rng.standard_normal((n, dim)) * np.exp(rng.standard_normal(dim))
    offset = []
    if dim >= 3:
        a, b = dim // 3, (2 * dim) // 3
        Q[:, a] = 1e6 + rng.standard_normal(n)
        sd = np.exp(rng.standard_normal())
        Q[:, b] = sd * (-3000.0 + rng.standard_normal(n))
        offset = [a, b]
    return Q, offset


def cov_reference(Q):
    """(m, C, mean bound, tol) of the module's docstring, in long double."""
    need_long_double()
    n, dim = Q.shape
    Ql = Q.astype(LD)
    m = Ql.sum(axis=0) / n
    d = Ql - m
    C = d.T @ d / n
    S = np.abs(d).T @ np.abs(d) / n
    a = np.abs(d).sum(axis=0) / n
    e = gamma(n + 3) * np.abs(Ql).max(axis=0)
    g = gamma(n + 2)
    tol = g * S + (1 + g) * (np.outer(a, e) + np.outer(e, a) + np.outer(e, e))
    mean_bound = gamma(n) * np.abs(Ql).sum(axis=0) / n + LD(2.0) ** -53 * np.abs(m)
    return m, C, mean_bound, tol


def cov_sharpness(Q, offset):
    """(worst tol_ij / sqrt(C_ii C_jj) on ordinary entries, on entries that touch an offset column): the reference alone."""
    _, C, _, tol = cov_reference(Q)
    dim = Q.shape[1]
    scale = np.sqrt(np.outer(np.diag(C), np.diag(C)))
    assert np.all(scale > 0)
    off = np.zeros(dim, bool)
    off[list(offset)] = True
    touches = off[:, None] | off[None, :]
    rel = tol / scale
    return float(np.max(rel[~touches], initial=0)), float(np.max(rel[touches], initial=0))


def check_cov(mean, cov, Q, offset, label):
    """Mean and covariance against their bounds; from two samples on, the caps on the inputs first.  Prints the worst error / bound of
    either."""
    n, dim = Q.shape
    assert mean.shape == (dim,) and cov.shape == (dim, dim), label
    if n >= 2:                                       # one sample: C = 0 exactly, there is no scale to be sharp against
        plain, shifted = cov_sharpness(Q, offset)
        assert plain <= 1e-12 and shifted <= 1e-6, (label, plain, shifted)
    m, C, mean_bound, tol = cov_reference(Q)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov)), label
    err_m, err_c = np.abs(mean.astype(LD) - m), np.abs(cov.astype(LD) - C)
    ratio_m = float(np.max(np.where(mean_bound > 0, err_m / np.where(mean_bound > 0, mean_bound, 1), np.where(err_m > 0, np.inf, 0))))
    ratio_c = float(np.max(np.where(tol > 0, err_c / np.where(tol > 0, tol, 1), np.where(err_c > 0, np.inf, 0))))
    print(f"{label}: |mean - m| / bound {ratio_m:.3f}, |cov - C| / bound {ratio_c:.3f}")
    assert ratio_m <= 1.0, (label, "mean", ratio_m)
    assert ratio_c <= 1.0, (label, "cov", ratio_c)
    return ratio_m, ratio_c
