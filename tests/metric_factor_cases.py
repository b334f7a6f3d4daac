"""Matrices, bounds and structure checks shared by tests/test_metric_factor_host.py and tests/test_gpu_metric_factor.py: what
hmc.factor_metric (mcd_metric_factor) must deliver, on the host and on the device alike.

Bounds (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3 and Thm 8.5), componentwise, with
gamma_k = k 2^-53 / (1 - k 2^-53), evaluated in np.longdouble (64 bits of mantissa: the check's own rounding stays below 2^-10 of the bound):

    |sym - U U^T|_ij <= gamma_{dim+1} (|U| |U|^T)_ij          |U W - I|_ij <= gamma_dim (|U| |W|)_ij

They hold for any order of summation, with or without fused multiply-adds, for factors computed entry by entry as one sum followed by one
division or square root -- so they carry no extra margin."""
import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi

U53 = 2.0 ** -53
DIMS = [1, 2, 63, 64, 65, 129, 257]                 # the edges of a 64-tile, one to five block columns
FAMILIES = ["scaled", "window"]


def scaled_matrix(dim, seed=1):
    """(a) C = S R S, R_ij = 0.5^|i-j|, S = diag(1e-2 exp(2 z)), z standard normal clipped at +-2.6: cond(C) up to about 1e10 (the shape of
    metric_for in tests/test_gpu_dense_metric.py)."""
    z = np.clip(np.random.default_rng(1000 * seed + dim).standard_normal(dim), -2.6, 2.6)
    s = 1e-2 * np.exp(2.0 * z)
    k = np.arange(dim)
    C = s[:, None] * 0.5 ** np.abs(k[:, None] - k[None, :]) * s[None, :]
    return 0.5 * (C + C.T)


def window_matrix(dim, seed=2):
    """(b) hmc.shrunk_covariance of max(8, dim // 2) positions: the warm-up's rank-deficient window, positive definite by the shrinkage
    term alone."""
    rng = np.random.default_rng(1000 * seed + dim)
    n = max(8, dim // 2)
    Q = rng.standard_normal((n, dim)) * (0.05 * np.exp(rng.standard_normal(dim)))
    C = M.shrunk_covariance(Q)
    return 0.5 * (C + C.T)


def matrix(family, dim):
    return scaled_matrix(dim) if family == "scaled" else window_matrix(dim)


def indefinite_matrix(dim, k, seed=3):
    """C = U0 U0^T with C_kk lowered by 2 (U0)_kk^2: the pivots before k are those of U0 U0^T, the sum at pivot k is about -(U0)_kk^2.  The
    rows of U0 carry enough weight below the diagonal that C_kk itself stays positive for k >= 16 (at k = 0 the pivot IS C_00)."""
    rng = np.random.default_rng(1000 * seed + dim)
    U0 = 0.3 * np.tril(rng.standard_normal((dim, dim)), -1) + np.diag(1.0 + 0.5 * rng.random(dim))
    C = U0 @ U0.T
    C = 0.5 * (C + C.T)
    C[k, k] -= 2.0 * U0[k, k] ** 2
    assert k == 0 or C[k, k] > 0
    return C


def need_long_double():
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble has fewer than 64 bits of mantissa here: the bounds cannot be evaluated")


def gamma(k):
    k = np.longdouble(k)
    u = np.longdouble(2.0) ** -53
    return k * u / (1 - k * u)


def check_factors(C, sym, U, W, label):
    """Both bounds and the structure of (sym, U, W) = factor_metric(C); prints the largest ratio error / bound of either."""
    need_long_double()
    dim = C.shape[0]
    ld = np.longdouble
    want_sym = 0.5 * (C + C.T)
    want_sym[np.diag_indices(dim)] = np.diag(C)
    assert np.array_equal(sym, want_sym), label
    iu = np.triu_indices(dim, 1)
    for A in (U, W):
        assert np.all(A[iu] == 0.0) and not np.any(np.signbit(A[iu])), label      # exactly +0.0 above the diagonal
    assert np.all(np.diag(U) > 0), label
    assert np.array_equal(np.diag(W), 1.0 / np.diag(U)), label
    Ul, Wl = U.astype(ld), W.astype(ld)
    r_chol = np.abs(sym.astype(ld) - Ul @ Ul.T)
    b_chol = gamma(dim + 1) * (np.abs(Ul) @ np.abs(Ul).T)
    r_inv = np.abs(Ul @ Wl - np.eye(dim, dtype=ld))
    b_inv = gamma(dim) * (np.abs(Ul) @ np.abs(Wl))
    ratio_chol = float(np.max(np.where(b_chol > 0, r_chol / np.where(b_chol > 0, b_chol, 1), 0)))
    ratio_inv = float(np.max(np.where(b_inv > 0, r_inv / np.where(b_inv > 0, b_inv, 1), 0)))
    print(f"{label}: |sym - U U^T| / bound {ratio_chol:.3f}, |U W - I| / bound {ratio_inv:.3f}")
    assert np.all(r_chol <= b_chol), (label, ratio_chol)
    assert np.all(r_inv <= b_inv), (label, ratio_inv)


def refusal_cases(dim=131):
    """(name, C, kind, row, column, words of the message): what factor_metric refuses, the offender as info names it."""
    base = scaled_matrix(dim)
    out = []
    for name, value, at in (("nan", np.nan, (7, 3)), ("inf", np.inf, (64, 65))):
        bad = base.copy()
        bad[at] = value
        out.append((name, bad, _capi.MCD_METRIC_FACTOR_NOT_FINITE, at[0], at[1], [f"C[{at[0]}][{at[1]}]", "not finite"]))
    bad = base.copy()
    bad[2, 70] += 1e-9 * np.sqrt(base[2, 2] * base[70, 70])                       # ten times the symmetry bound
    out.append(("asymmetric", bad, _capi.MCD_METRIC_FACTOR_ASYMMETRIC, 2, 70, ["not symmetric", "C[2][70]", "C[70][2]"]))
    for name, value in (("negative-diagonal", -1.0), ("zero-diagonal", 0.0)):
        bad = base.copy()
        bad[66, 66] *= value
        out.append((name, bad, _capi.MCD_METRIC_FACTOR_DIAGONAL, 66, 66, ["not positive definite", "C[66][66]"]))
    for k in (0, 63, 64, 130):
        if k == 0:      # the sum at pivot 0 is C_00 itself: the check of the diagonal names it
            out.append(("pivot-0", indefinite_matrix(dim, 0), _capi.MCD_METRIC_FACTOR_DIAGONAL, 0, 0, ["not positive definite", "C[0][0]"]))
        else:
            out.append((f"pivot-{k}", indefinite_matrix(dim, k), _capi.MCD_METRIC_FACTOR_PIVOT, k, k, ["not positive definite", f"pivot {k}"]))
    return out


def check_refusal(case, where):
    """factor_metric(C, where) refuses the case as named; returns the message."""
    name, C, kind, row, col, words = case
    with pytest.raises(M.McdError) as ei:
        M.factor_metric(C, where=where)
    assert ei.value.code == _capi.MCD_ERR_INVALID_ARG, (name, str(ei.value))
    assert ei.value.info == (kind, row, col), (name, ei.value.info)
    assert all(w in str(ei.value) for w in words), (name, str(ei.value))
    return str(ei.value)
