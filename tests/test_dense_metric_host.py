"""The dense metric of the device leapfrog and NUTS (mcd_hmc_set_metric / _get_metric / _nuts_warmup_dense) -- what needs no GPU: the C ABI's
surface, and the numpy restatements of the algebra (hmc.metric_factors, hmc.shrunk_covariance, the 2-D `inv_mass` of the host-side
NUTS recursion) that tests/test_gpu_dense_metric.py compares the device with."""
import math
import os
import re

import numpy as np

import mcmc_date_amd as M
from mcmc_date_amd import _capi, hmc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcd_hmc_set_metric", "mcd_hmc_get_metric", "mcd_hmc_nuts_warmup_dense")


def test_the_three_calls_are_in_the_header_and_in_the_ctypes_table_with_equal_arity():
    src = open(os.path.join(ROOT, "include", "mcmcdate_mvn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in include/mcmcdate_mvn.h"
        assert name in _capi.SYMBOLS, f"{name} is not in _capi.SYMBOLS"
        assert len(m.group(1).split(",")) == len(_capi.SYMBOLS[name][1]), name
        assert hasattr(_capi.lib(), name), f"{name} is not exported"
    assert re.search(r"#define\s+MCD_HMC_DENSE_MAX_DIM\s+512\b", code) and _capi.MCD_HMC_DENSE_MAX_DIM == 512


def random_spd(dim, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(dim, dim))
    s = np.exp(rng.uniform(-3.0, 1.0, dim))
    return s[:, None] * (A @ A.T / dim + 0.2 * np.eye(dim)) * s[None, :]


def test_metric_factors():
    C = random_spd(37, 1)
    U, W = M.metric_factors(C)
    cond = np.linalg.cond(C)
    assert np.array_equal(U, np.tril(U)) and np.array_equal(W, np.triu(W))
    assert np.max(np.abs(W @ W.T @ C - np.eye(37))) <= 1e-10 * cond
    assert np.max(np.abs(U @ U.T - C)) <= 1e-10 * cond


def test_shrunk_covariance_is_the_formula():
    rng = np.random.default_rng(2)
    n, dim = 200, 9
    Q = rng.normal(size=(n, dim)) @ rng.normal(size=(dim, dim)) + rng.normal(size=dim) * 50.0
    ref = n / (n + 5.0) * np.cov(Q, rowvar=False, bias=True) + 1e-3 * 5.0 / (n + 5.0) * np.eye(dim)
    got = M.shrunk_covariance(Q)
    assert np.max(np.abs(got - ref) / np.sqrt(np.outer(np.diag(ref), np.diag(ref)))) <= 1e-13
    # its diagonal is the rule of the diagonal warm-up (mcd_hmc_nuts_warmup)
    assert np.allclose(np.diag(got), n / (n + 5.0) * Q.var(axis=0) + 1e-3 * 5.0 / (n + 5.0), rtol=1e-12)


def _drive(gen, eps, prec, metric_apply):
    """Runs hmc._nuts_chain's generator on the Gaussian target ln pi(q) = -1/2 q^T prec q with a leapfrog of the test's own."""
    def grad(q):
        return -prec @ q

    def logp(q):
        return -0.5 * float(q @ prec @ q)

    try:
        req = next(gen)
        while True:
            q, r, g, v = req
            e = eps * v
            r = r + 0.5 * e * g
            q = q + e * metric_apply(r)
            g = grad(q)
            r = r + 0.5 * e * g
            req = gen.send((q, r, g, logp(q)))
    except StopIteration as done:
        return done.value


def test_nuts_chain_with_a_diagonal_matrix_is_the_vector_form():
    dim = 6
    A = np.random.default_rng(3).normal(size=(dim, dim))
    prec = np.linalg.inv(A @ A.T / dim + 0.5 * np.eye(dim))        # a correlated Gaussian target of unit scale
    v = np.exp(np.random.default_rng(4).uniform(-1.0, 1.0, dim))
    n_moved = 0
    for trial in range(8):
        rng = np.random.default_rng(100 + trial)
        q0 = rng.normal(size=dim)
        r0 = rng.normal(size=dim) / np.sqrt(v)
        g0, lp0 = -prec @ q0, -0.5 * float(q0 @ prec @ q0)
        joint0 = lp0 - 0.5 * float(np.sum(r0 * r0 * v))
        log_u = joint0 + math.log(rng.uniform())
        out = []
        for inv_mass in (v, np.diag(v)):
            stats = {"alpha": 0.0, "n_alpha": 0, "joint0": joint0, "depth": 0}
            gen = hmc._nuts_chain(q0.copy(), g0.copy(), lp0, r0.copy(), log_u, np.random.default_rng(7 + trial), inv_mass, 6, stats)
            out.append((_drive(gen, 0.15, prec, lambda r: v * r), stats))
        (qa, ga, la), sa = out[0]
        (qb, gb, lb), sb = out[1]
        assert sa["depth"] == sb["depth"] and sa["n_alpha"] == sb["n_alpha"] and sa["depth"] >= 1
        assert np.array_equal(qa, qb) and np.array_equal(ga, gb) and la == lb
        assert abs(sa["alpha"] - sb["alpha"]) <= 1e-12 * sa["n_alpha"]
        n_moved += int(not np.array_equal(qa, q0))
    assert n_moved >= 4
