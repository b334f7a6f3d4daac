"""The deterministic inputs of the graphical-lasso tests (tests/test_glasso_host.py, tests/test_gpu_glasso.py), rho = 0.1 throughout:
AR(1)-correlated samples -> correlation matrices, drawn in one fixed order from one generator, and the host solver's results on them,
computed once per session.  The inputs added later (unequal diagonals, one component per stride count, the permuted blocks) each draw
from a generator of their own, so the draws above them never move."""
import functools

import numpy as np

RHO = 0.1
BLOCKS = (33, 1, 30, 1, 5)
STRIDE_SIZES = (256, 512, 513, 1025, 2048)                 # 1, 2, 3, 5, 8 coordinates per thread; 256, 512, 2048 fill their last stride
PACKED_BLOCKS = (2, 3, 33, 65, 257, 600, 1, 1)             # stride counts 1, 1, 1, 1, 2, 3 in one launch, and two singletons


def ar(rng, p, n, a=0.6):
    z = rng.standard_normal((n, p))
    for i in range(1, p):
        z[:, i] = a * z[:, i - 1] + np.sqrt(1 - a * a) * z[:, i]
    return z


def scaled_cov(seed, p, n):
    """The covariance of n AR(1) samples of p variables, every variable scaled by exp(U(ln 0.5, ln 2))."""
    rng = np.random.default_rng(seed)
    z = ar(rng, p, n)
    return np.cov(z * np.exp(rng.uniform(np.log(0.5), np.log(2.0), p)), rowvar=False)


@functools.lru_cache(maxsize=None)
def c300():
    """C300: the recipe of C16 and C48 at p = 300 (600 samples), diagonal 0.23 ... 4.1; read-only."""
    S = scaled_cov(13, 300, 600)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def stride_input(p):
    """One component of p variables, built as tools/bench_glasso.py builds its problems (2 p samples); read-only."""
    S = np.corrcoef(ar(np.random.default_rng(1000 + p), p, 2 * p), rowvar=False)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def packed():
    """(S, label): independent AR(1) correlation blocks of PACKED_BLOCKS (max(150, 2 p) samples), off-block entries uniform in +-0.08 as
    in "blocks", then one fixed permutation of rows and columns: every component's members are scattered over 0 ... n - 1.  label[i] is
    the index into PACKED_BLOCKS of variable i's block.  Read-only."""
    rng = np.random.default_rng(31)
    n = sum(PACKED_BLOCKS)
    S = np.eye(n)
    inside = np.eye(n, dtype=bool)
    at = 0
    for b in PACKED_BLOCKS:
        if b > 1:
            S[at:at + b, at:at + b] = np.corrcoef(ar(rng, b, max(150, 2 * b)), rowvar=False)
            inside[at:at + b, at:at + b] = True
        at += b
    U = np.triu(rng.uniform(-0.08, 0.08, (n, n)), 1)
    U = U + U.T
    S[~inside] = U[~inside]
    perm = rng.permutation(n)
    S = np.ascontiguousarray(S[np.ix_(perm, perm)])
    label = np.repeat(np.arange(len(PACKED_BLOCKS)), PACKED_BLOCKS)[perm]
    S.setflags(write=False)
    label.setflags(write=False)
    return S, label


def by_smallest_member(label):
    """The same partition numbered by each part's smallest member, as mcd_glasso_components numbers its components."""
    _, first = np.unique(label, return_index=True)
    rank = np.empty(len(first), int)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[label]


def closed_form_2x2(S, rho):
    """(W, Theta) of the graphical lasso at p = 2 with the diagonal penalised and |S_01| > rho: W = S + rho I with
    W_01 = S_01 - rho sign S_01, Theta = W^-1 by the 2 x 2 formula."""
    w = S[0, 1] - rho * np.sign(S[0, 1])
    W = np.array([[S[0, 0] + rho, w], [w, S[1, 1] + rho]])
    det = W[0, 0] * W[1, 1] - w * w
    return W, np.array([[W[1, 1], -w], [-w, W[0, 0]]]) / det


def two_by_two(s):
    return np.array([[1.3, s], [s, 0.7]])


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
    # covariances with unequal diagonals (0.26 ... 3.4): W_kk differs from coordinate to coordinate (c300() gives the second stride its own).
    # The seeds of C16 and C48 were taken for the host solver's margins on them (tests/test_glasso_host.py: smallest non-zero |Theta|
    # 3.0e-4, closest inactive entry 4.8e-4 below rho), which is what makes the pattern comparison with the device well posed
    out["C16"] = scaled_cov(11, 16, 200)
    out["C48"] = scaled_cov(16, 48, 300)
    # 3 x 3, every |off-diagonal| above rho: one wave owns all three coordinates, three own none
    out["S3"] = np.array([[1.0, 0.5, -0.3], [0.5, 1.0, 0.2], [-0.3, 0.2, 1.0]])
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
