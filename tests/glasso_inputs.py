"""The deterministic inputs of the graphical-lasso tests (tests/test_glasso_host.py, tests/test_gpu_glasso.py), rho = 0.1 throughout:
AR(1)-correlated samples -> correlation matrices, drawn in one fixed order from one generator, and the host solver's results on them,
computed once per session."""
import functools

import numpy as np

RHO = 0.1
BLOCKS = (33, 1, 30, 1, 5)


def ar(rng, p, n, a=0.6):
    z = rng.standard_normal((n, p))
    for i in range(1, p):
        z[:, i] = a * z[:, i - 1] + np.sqrt(1 - a * a) * z[:, i]
    return z


@functools.lru_cache(maxsize=None)
def inputs():
    rng = np.random.default_rng(2024)                      # drawn in this order
    out = {}
    out["S16"] = np.corrcoef(ar(rng, 16, 200), rowvar=False)
    out["S70"] = np.corrcoef(ar(rng, 70, 300), rowvar=False)        # crosses one wave
    out["S70s"] = np.corrcoef(ar(rng, 70, 40), rowvar=False)        # singular: fewer samples than dimensions, the real-data case
    # blocks 33 + 1 + 30 + 1 + 5, and a symmetric perturbation below rho outside the blocks (the matrix is then indefinite, which is fine)
    n = sum(BLOCKS)
    S = np.eye(n)
    inside = np.eye(n, dtype=bool)
    at = 0
    for b in BLOCKS:
        if b > 1:
            S[at:at + b, at:at + b] = np.corrcoef(ar(rng, b, 150), rowvar=False)
            inside[at:at + b, at:at + b] = True
        at += b
    U = np.triu(rng.uniform(-0.08, 0.08, (n, n)), 1)
    U = U + U.T
    S[~inside] = U[~inside]
    out["blocks"] = S
    # the 11 x 11 input of tests/test_prepare.py::test_graphical_lasso_optimality_conditions
    r0 = np.random.default_rng(0)
    X = r0.standard_normal((9, 11))
    X[:, 3] += X[:, 2]
    X[:, 7] -= 0.7 * X[:, 1]
    out["S11"] = np.corrcoef(X, rowvar=False)
    for v in out.values():
        v.setflags(write=False)
    return out


def block_labels():
    return np.repeat(np.arange(len(BLOCKS)), BLOCKS)


@functools.lru_cache(maxsize=None)
def host_solution(name, penalize_diagonal=True):
    """(W, Theta) of prepare.graphical_lasso on inputs()[name], read-only."""
    from mcmc_date_amd.prepare import graphical_lasso

    W, T = graphical_lasso(inputs()[name], RHO, penalize_diagonal=penalize_diagonal)
    W.setflags(write=False)
    T.setflags(write=False)
    return W, T


def optimality_violations(S, W, T, rho, penalize_diagonal):
    """The conditions that characterise the unique optimum (Friedman et al. 2008, eq. 2.4) as tests/test_prepare.py:138-144 states them:
    the largest violation of each, for its bound there -- (|W Theta - I|, |diag W - diag S - rho pen|, |(W - S)_ij - rho sign Theta_ij| where
    Theta_ij != 0, |(W - S)_ij| - rho where Theta_ij = 0, the smallest eigenvalue of Theta)."""
    p = S.shape[0]
    off = ~np.eye(p, dtype=bool)
    nz = (T != 0) & off
    z = off & ~nz
    return (np.abs(W @ T - np.eye(p)).max(),
            np.abs(np.diag(W) - np.diag(S) - (rho if penalize_diagonal else 0.0)).max(),
            np.abs((W - S)[nz] - rho * np.sign(T[nz])).max() if nz.any() else 0.0,
            (np.abs((W - S)[z]).max() - rho) if z.any() else -rho,
            np.linalg.eigvalsh(T).min())
