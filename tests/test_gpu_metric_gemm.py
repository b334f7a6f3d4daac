"""csrc/k_metric_gemm.hip on its own (mcd_metric_gemm_ through hmc._metric_gemm: the launcher unchanged, on device buffers of exactly the
arrays' sizes): the product kernel of the dense metric's across-chains form at the row counts it is used at -- every wave of a 64-row
tile, a second and a third row tile, rows through the index list of a NUTS round.

What is held, and against what (tests/metric_product_cases.py):
  exact      integer X and A in [-512, 512]: Y is the int64 product as numbers, full and lower, direct and through the list;
  bounded    real X, A = S R S (metric_factor_cases.scaled_matrix) and its U^-1: |Y - X A| <= gamma_dim |X| |A| componentwise, references
             in long double;
  contracts  lower = 1 and lower = 0 give the same bits on a lower-triangular A; a listed row has the bits it has alone and in the direct
             launch, whatever the order of the list; unlisted rows are neither read (NaN) nor written (7.25); a row of NaN or Inf changes
             no other row; two calls give the same bits; a list that leaves the buffers is refused before anything runs.

Measured on the MI355X, worst error / bound of the bounded group (the exact and contract groups have no tolerance): C = S R S 0.130 and
0.120 at dim 99 (65 and 130 rows), 0.024 at dim 513; U^-1 0.037 and 0.038 at dim 99, 0.007 and 0.008 at dim 513 -- numpy's own fp64
product sits at 0.130 and 0.024 of the same bound (tests/test_metric_product_host.py)."""
import numpy as np
import pytest

import mcmc_date_amd as M
import metric_product_cases as P
from mcmc_date_amd import _capi
from mcmc_date_amd.hmc import _metric_gemm
from metric_factor_cases import scaled_matrix

pytestmark = pytest.mark.gpu

SLOTS = 13                                           # kNutsRhsMaxSlots: the slots of the NUTS workspace
B = 130
# every row count around the waves' 16 rows and the tile's 64, every dim around the 32-term chunk, the 64-column tile and four-term steps
EXACT = [(1, 513), (15, 1), (16, 3), (17, 31), (47, 32), (48, 33), (49, 63), (63, 64), (64, 65), (65, 99), (128, 516), (130, 513), (130, 65),
         (65, 1), (49, 516)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("rows,dim", EXACT)
def test_integer_products_are_exact(gpu, rows, dim):
    X, A = P.int_inputs(rows, dim)
    assert np.array_equal(_metric_gemm(X, A), P.int_product(X, A))
    L = np.tril(A)
    assert np.array_equal(_metric_gemm(X, L, lower=True), P.int_product(X, L))
    assert np.array_equal(_metric_gemm(X, L, lower=False), P.int_product(X, L))
    if rows > 1:                                     # the first rows alone: the rest of Y keeps what it held
        Y0 = np.full_like(X, P.MARK)
        part = _metric_gemm(X, A, Y0, rows=rows - 1)
        assert np.array_equal(part[:-1], P.int_product(X[:-1], A)) and np.all(part[-1] == P.MARK)


@pytest.mark.parametrize("rows,dim", [(65, 99), (130, 99), (65, 513), (130, 513)])
def test_real_products_within_the_bound(gpu, rows, dim):
    X = P.real_rows(rows, dim)
    C = scaled_matrix(dim)
    sym, _, W = M.factor_metric(C, where="host")
    assert np.array_equal(W, np.tril(W))
    Y = _metric_gemm(X, sym)
    P.check_product(Y, X, sym, f"C = S R S, rows {rows}, dim {dim}")
    Yw = _metric_gemm(X, W, lower=True)
    P.check_product(Yw, X, W, f"U^-1 (lower), rows {rows}, dim {dim}")
    # the terms a lower-triangular A lets the kernel skip are exact zeros: the same bits without the skip
    assert np.array_equal(bits(_metric_gemm(X, W, lower=False)), bits(Yw))
    # the same bits on every call
    assert np.array_equal(bits(_metric_gemm(X, sym)), bits(Y)) and np.array_equal(bits(_metric_gemm(X, W, lower=True)), bits(Yw))


def random_list(n_list, seed):
    return np.random.default_rng(1000 * seed + n_list).permutation(B)[:n_list].astype(np.int32)


@pytest.mark.parametrize("n_list", [1, 5, 47, 64, 65, 130])
@pytest.mark.parametrize("slots", [1, 3, 13])
def test_rows_through_the_list(gpu, slots, n_list):
    dim = 65
    lst = random_list(n_list, slots)
    mem = P.list_rows(lst, slots, B)
    Xi, Ai = P.int_inputs(SLOTS * B, dim)
    X = np.full_like(Xi, np.nan)                     # unlisted rows and the rows of unused slots: NaN in X, the mark in Y
    X[mem] = Xi[mem]
    Y0 = np.full_like(Xi, P.MARK)
    Y = _metric_gemm(X, Ai, Y0, rows=slots * n_list, rows_list=lst, stride=B)
    P.check_listed(Y, Xi, Ai, lst, slots, B, f"slots {slots}, n_list {n_list}")
    # the order of the list (the order in which the chains reported themselves) changes no row
    perm = np.random.default_rng(7).permutation(n_list)
    Yp = _metric_gemm(X, Ai, Y0, rows=slots * n_list, rows_list=lst[perm], stride=B)
    assert np.array_equal(bits(Yp), bits(Y))
    # real rows: the bits of a listed row are those of the direct launch and of the row alone, wherever the list puts it
    Xr = P.real_rows(SLOTS * B, dim)
    Ar = scaled_matrix(dim)
    direct = _metric_gemm(Xr, Ar)
    Xn = np.full_like(Xr, np.nan)
    Xn[mem] = Xr[mem]
    Yr = _metric_gemm(Xn, Ar, Y0, rows=slots * n_list, rows_list=lst, stride=B)
    assert np.array_equal(bits(Yr[mem]), bits(direct[mem]))
    untouched = np.setdiff1d(np.arange(SLOTS * B), mem)
    assert np.all(Yr[untouched] == P.MARK)
    assert np.array_equal(bits(_metric_gemm(Xn, Ar, Y0, rows=slots * n_list, rows_list=lst[perm], stride=B)), bits(Yr))
    edges = sorted({r for r in (0, 15, 16, 47, 48, 63, 64, slots * n_list - 1) if r < slots * n_list})      # product rows at the waves' and tiles' edges
    for r in edges:
        alone = _metric_gemm(Xr[mem[r]:mem[r] + 1], Ar)
        assert np.array_equal(bits(alone[0]), bits(Yr[mem[r]])), r


def test_a_list_that_leaves_the_buffers_is_refused(gpu):
    dim = 5
    X, A = P.int_inputs(2 * B, dim)
    Y0 = np.full_like(X, P.MARK)
    cases = [dict(rows_list=[3, 2 * B], rows=2, stride=B),                       # an entry outside the rows
             dict(rows_list=[3, -1], rows=2, stride=B),
             dict(rows_list=[3, 129], rows=6, stride=B),                          # slot 2 of two
             dict(rows_list=[3, 129], rows=3, stride=2 * B - 3)]                  # row 3 + stride is the first outside
    for kw in cases:
        with pytest.raises(M.McdError) as ei:
            _metric_gemm(X, A, Y0, **kw)
        assert ei.value.code == _capi.MCD_ERR_INVALID_ARG, kw
    with pytest.raises(M.McdError):
        _metric_gemm(X, A, Y0, rows=2 * B + 1)
    ok = _metric_gemm(X, A, Y0, rows_list=[3, 129], rows=4, stride=B)            # the last row of the buffers is allowed
    assert np.array_equal(ok[[3, 129, B + 3, B + 129]], P.int_product(X[[3, 129, B + 3, B + 129]], A))
    assert _metric_gemm(X, A, Y0, rows_list=[3, 129], rows=3, stride=2 * B - 4)[2 * B - 1, 0] == P.int_product(X[-1:], A)[0, 0]


def test_a_row_of_nan_or_inf_touches_no_other_row(gpu):
    rows, dim = 130, 99
    X = P.real_rows(rows, dim)
    A = scaled_matrix(dim)
    assert np.all(A > 0)                             # so a row of +Inf is +Inf in every sum
    clean = _metric_gemm(X, A)
    special = {15: np.full(dim, np.nan), 16: np.full(dim, np.inf), 47: np.full(dim, -np.inf), 48: np.where(np.arange(dim) % 2, np.inf, -np.inf),
               63: X[63].copy(), 64: X[64].copy(), 129: X[129].copy()}
    special[63][98] = np.nan                         # one NaN in the ragged last chunk of the sum
    special[64][0] = np.inf
    special[129][33] = -np.inf
    Xs = X.copy()
    for r, row in special.items():
        Xs[r] = row
    Y = _metric_gemm(Xs, A)
    others = np.setdiff1d(np.arange(rows), list(special))
    assert np.array_equal(bits(Y[others]), bits(clean[others]))
    assert np.all(np.isnan(Y[[15, 48, 63]]))
    assert np.all(Y[[16, 64]] == np.inf) and np.all(Y[[47, 129]] == -np.inf)
    # the same through the list: the special rows listed among ordinary ones
    lst = np.array([16, 3, 129, 64, 70, 15, 48, 0], np.int32)
    Yl = _metric_gemm(Xs, A, np.full_like(X, P.MARK), rows_list=lst, stride=rows)
    assert np.array_equal(bits(Yl[lst]), bits(Y[lst]))
    assert np.all(Yl[np.setdiff1d(np.arange(rows), lst)] == P.MARK)
