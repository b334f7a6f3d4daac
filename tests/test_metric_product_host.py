"""The bounds of tests/metric_product_cases.py are neither vacuous nor too tight (no GPU): numpy's fp64 product and two-pass covariance
satisfy them, and every planted fault -- a dropped term, exchanged rows, a slot written at the wrong stride, the sum-of-squares covariance,
the division by n - 1 -- is reported as outside its bound.

Measured here: numpy's X A sits at 0.13 of the product bound at dim 99 and at 0.024 at dim 513; its two-pass covariance at 0.021 of the
covariance bound or below and its mean at 0.09 or below from 31 samples on (0.19 and 0.24 at two samples); the sum-of-squares form at 14
to 1.3e5 times the bound on the offset diagonals; the caps' ratios are <= 7.5e-14 on ordinary entries and <= 1.8e-8 on entries that touch
an offset column."""
import numpy as np
import pytest

import metric_product_cases as P
from metric_factor_cases import need_long_double, scaled_matrix

COV_SHAPES = [(33, 17), (100, 65), (65, 130)]


def two_pass(Q):
    n = Q.shape[0]
    mean = Q.sum(axis=0) / n
    d = Q - mean
    return mean, d.T @ d / n


@pytest.mark.parametrize("rows,dim", [(65, 99), (130, 513)])
def test_numpy_product_meets_the_bound_and_planted_faults_do_not(rows, dim):
    need_long_double()
    X = P.real_rows(rows, dim)
    A = scaled_matrix(dim)
    Y = X @ A
    assert P.check_product(Y, X, A, f"numpy, rows {rows}, dim {dim}") < 0.5
    # one term of one sum dropped: the one through A's diagonal (terms far from the diagonal of this A vanish below the sum's rounding)
    r, k = rows - 1, dim // 2
    bad = Y.copy()
    bad[r, k] -= X[r, k] * A[k, k]
    with pytest.raises(AssertionError):
        P.check_product(bad, X, A, "one term dropped")
    # two rows exchanged
    bad = Y.copy()
    bad[[rows - 2, rows - 1]] = bad[[rows - 1, rows - 2]]
    with pytest.raises(AssertionError):
        P.check_product(bad, X, A, "rows exchanged")
    # lower: the product with the triangle alone meets the triangle's bound, not the full matrix's
    L = np.tril(A)
    P.check_product(X @ L, X, L, "numpy, lower triangle")
    with pytest.raises(AssertionError):
        P.check_product(X @ L, X, A, "triangle in the place of the matrix")


def test_integer_products_are_exact_in_fp64():
    X, A = P.int_inputs(130, 516)
    want = P.int_product(X, A)
    assert np.array_equal(X @ A, want) and np.array_equal(X[:, ::-1] @ A[::-1], want)      # in another order of the sum too
    assert np.abs(X).max() == 512 and np.abs(A).max() == 512 and X.min() == -512


@pytest.mark.parametrize("slots,n_list", [(1, 5), (3, 47), (13, 65), (13, 130)])
def test_the_list_check_catches_a_slot_at_the_wrong_stride(slots, n_list):
    B, dim = 130, 33
    X, A = P.int_inputs(13 * B, dim)
    lst = np.random.default_rng(n_list).permutation(B)[:n_list]
    Y0 = np.full_like(X, P.MARK)
    rows = slots * n_list
    good = P.listed_product(X, A, Y0, lst, rows, B)
    P.check_listed(good, X, A, lst, slots, B, "numpy through the list")
    # unlisted rows of X are never looked at: NaN there changes nothing
    Xn = np.full_like(X, np.nan)
    mem = P.list_rows(lst, slots, B)
    Xn[mem] = X[mem]
    assert np.array_equal(P.listed_product(Xn, A, Y0, lst, rows, B), good)
    if slots > 1 and n_list < B:                                          # slot s of the list written at s n_list instead of s B
        bad = P.listed_product(X, A, Y0, lst, rows, n_list)
        with pytest.raises(AssertionError):
            P.check_listed(bad, X, A, lst, slots, B, "stride = n_list")
    # a listed row left unwritten; an unlisted row written; two listed rows exchanged
    for fault in ("missing", "extra", "exchanged"):
        bad = good.copy()
        if fault == "missing":
            bad[mem[-1]] = P.MARK
        elif fault == "extra":
            if n_list == B and slots == 13:
                continue
            free = np.setdiff1d(np.arange(13 * B), mem)[0]
            bad[free] = X[free] @ A
        else:
            if mem.size < 2:
                continue
            bad[[mem[0], mem[-1]]] = bad[[mem[-1], mem[0]]]
        with pytest.raises(AssertionError):
            P.check_listed(bad, X, A, lst, slots, B, fault)


@pytest.mark.parametrize("n,dim", COV_SHAPES + [(2, 15), (31, 16), (32, 1), (1, 17)])
def test_numpy_two_pass_covariance_meets_the_bound(n, dim):
    need_long_double()
    Q, offset = P.cov_inputs(n, dim)
    mean, cov = two_pass(Q)
    rm, rc = P.check_cov(mean, cov, Q, offset, f"numpy two-pass, n {n}, dim {dim}")
    assert rm <= 0.5 and rc <= 0.5
    if n == 1:
        assert np.all(cov == 0.0) and np.array_equal(mean, Q[0])


@pytest.mark.parametrize("n,dim", COV_SHAPES)
def test_the_caps_hold_and_planted_covariance_faults_are_outside_the_bound(n, dim):
    need_long_double()
    Q, offset = P.cov_inputs(n, dim)
    plain, shifted = P.cov_sharpness(Q, offset)
    print(f"n {n}, dim {dim}: tol / sqrt(C_ii C_jj) {plain:.1e} on ordinary entries, {shifted:.1e} on offset entries")
    assert plain <= 1e-12 and shifted <= 1e-6
    mean, cov = two_pass(Q)
    # E[x^2] - m^2: outside the bound on both offset diagonals
    sumsq = Q.T @ Q / n - np.outer(mean, mean)
    _, C, _, tol = P.cov_reference(Q)
    over = np.abs(sumsq.astype(P.LD) - C) / tol
    print(f"n {n}, dim {dim}: sum-of-squares form at {[float(over[k, k]) for k in offset]} of the bound on the offset diagonals")
    assert all(over[k, k] > 1 for k in offset)
    with pytest.raises(AssertionError):
        P.check_cov(mean, sumsq, Q, offset, "sum of squares")
    # divided by n - 1
    with pytest.raises(AssertionError):
        P.check_cov(mean, cov * (n / (n - 1.0)), Q, offset, "n - 1")
    # a mean taken over n - 1 samples; a neighbouring entry in the place of one
    with pytest.raises(AssertionError):
        P.check_cov(Q[:-1].mean(axis=0), cov, Q, offset, "mean of n - 1 samples")
    bad = cov.copy()
    bad[0, 1], bad[1, 0] = cov[0, 2], cov[2, 0]
    with pytest.raises(AssertionError):
        P.check_cov(mean, bad, Q, offset, "a neighbour's entry")
