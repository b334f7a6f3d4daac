"""The host side of the device graphical lasso (mcd_glasso, mcd_glasso_components; csrc/glasso_capi.cpp): the exact screening into
connected components, what the library refuses before any launch, and the `glasso` keyword of `prepare`.  No GPU involved."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse.csgraph as csgraph

import glasso_inputs as GI
import mcmc_date_amd as M
from mcmc_date_amd import _capi
from mcmc_date_amd import prepare as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("name", ["S16", "S70", "S70s", "blocks"])
@pytest.mark.parametrize("rho", [0.05, 0.1, 0.3])
def test_components_match_scipy(name, rho):
    S = GI.inputs()[name]
    adj = np.abs(S) > rho
    np.fill_diagonal(adj, False)
    nc, ref = csgraph.connected_components(adj, directed=False)
    lab = M.glasso_components(S, rho)
    assert lab.max() + 1 == nc and same_partition(lab, ref)
    # numbered by smallest member
    firsts = [int(np.flatnonzero(lab == c)[0]) for c in range(nc)]
    assert firsts == sorted(firsts)
    if name == "blocks" and rho == 0.1:
        assert same_partition(lab, GI.block_labels()) and sorted(np.bincount(lab).tolist()) == [1, 1, 5, 30, 33]
    if name != "blocks" and rho == 0.1:
        assert nc == 1


def _call(S, rho=0.1, n=None, tol=1e-10, max_iter=100):
    S = np.ascontiguousarray(S, float)
    n = S.shape[0] if n is None else n
    W, T = np.zeros_like(S), np.zeros_like(S)
    info = (C.c_int64 * _capi.MCD_GLASSO_INFO_LEN)()
    rc = _capi.lib().mcd_glasso(n, S.ctypes.data_as(_capi._dp), rho, 1, tol, max_iter, 0, W.ctypes.data_as(_capi._dp),
                                T.ctypes.data_as(_capi._dp), info)
    return rc, _capi.lib().mcd_last_error().decode()


def test_bad_arguments_are_refused_with_a_message():
    S = np.array(GI.inputs()["S16"])
    rc, msg = _call(S, n=0)
    assert rc == _capi.MCD_ERR_INVALID_ARG and "n = 0" in msg
    rc, msg = _call(S, rho=-0.1)
    assert rc == _capi.MCD_ERR_INVALID_ARG and "rho" in msg
    bad = S.copy()
    bad[3, 5] = np.nan
    rc, msg = _call(bad)
    assert rc == _capi.MCD_ERR_INVALID_ARG and "S[3][5] is not finite" in msg
    bad = S.copy()
    bad[2, 9] += 1e-6
    rc, msg = _call(bad)
    assert rc == _capi.MCD_ERR_INVALID_ARG and "not symmetric" in msg and "S[2][9]" in msg
    bad = S.copy()
    bad[4, 4] = 0.0
    rc, msg = _call(bad)
    assert rc == _capi.MCD_ERR_INVALID_ARG and "S[4][4]" in msg and "positive" in msg
    for kw in ({"tol": -1.0}, {"max_iter": 0}):
        rc, msg = _call(S, **kw)
        assert rc == _capi.MCD_ERR_INVALID_ARG and next(iter(kw)) in msg
    # the Python wrapper raises what the library refuses; rounding-level asymmetry (below MCD_GLASSO_SYMMETRY_TOL) is not refused as such
    with pytest.raises(M.McdError, match="not finite"):
        M.graphical_lasso_device(np.full((2, 2), np.inf), 0.1)
    with pytest.raises(ValueError):
        M.graphical_lasso_device(np.zeros((2, 3)), 0.1)
    with pytest.raises(M.McdError, match="not finite"):
        M.glasso_components(np.full((2, 2), np.nan), 0.1)


def test_a_component_above_the_limit_is_unsupported():
    """2049 variables chained by |S_i,i+1| = 0.4 > rho: one component above MCD_GLASSO_MAX_DIM; refused before any device is looked for."""
    n = _capi.MCD_GLASSO_MAX_DIM + 1
    S = np.eye(n)
    i = np.arange(n - 1)
    S[i, i + 1] = S[i + 1, i] = 0.4
    rc, msg = _call(S)
    assert rc == _capi.MCD_ERR_UNSUPPORTED and "2049" in msg and "2048" in msg


def test_python_constants_are_the_kernels():
    import re

    hpp = open(os.path.join(ROOT, "mcmc-date_amd", "csrc", "glasso_device.hpp")).read()
    hdr = open(os.path.join(ROOT, "include", "mcmcdate_mvn.h")).read()
    assert int(re.search(r"kGlassoThreads = (\d+);", hpp).group(1)) == PP.GLASSO_LANE_STRIDE
    assert int(re.search(r"kGlassoMaxDim = (\d+);", hpp).group(1)) == _capi.MCD_GLASSO_MAX_DIM
    assert int(re.search(r"#define MCD_GLASSO_INFO_LEN (\d+)", hdr).group(1)) == _capi.MCD_GLASSO_INFO_LEN >= len(PP.GLASSO_INFO_FIELDS)


@pytest.fixture(scope="module")
def mtcdnapri_paths(tmp_path_factory):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "mtCDNApri_prior_samples.json")))
    d = tmp_path_factory.mktemp("mtcdnapri")
    paths = {}
    for k in ("rooted_tree", "tree_list"):
        paths[k] = str(d / k)
        open(paths[k], "w").write(fx["inputs"][k])
    return paths


def test_prepare_device_without_a_gpu_is_the_no_device_error(mtcdnapri_paths):
    if _capi.lib().mcd_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(M.NoDevice, match="no CPU fallback"):
        PP.prepare(mtcdnapri_paths["tree_list"], mtcdnapri_paths["rooted_tree"], "SparseMultivariateNormal 0.1", glasso="device")
    with pytest.raises(M.NoDevice):
        M.graphical_lasso_device(GI.inputs()["S16"], 0.1)


def test_prepare_keyword_default_is_the_host_solver_byte_for_byte(mtcdnapri_paths, tmp_path):
    a = PP.prepare(mtcdnapri_paths["tree_list"], mtcdnapri_paths["rooted_tree"], "SparseMultivariateNormal 0.1")
    b = PP.prepare(mtcdnapri_paths["tree_list"], mtcdnapri_paths["rooted_tree"], "SparseMultivariateNormal 0.1", glasso="host")
    PP.write_prepared(str(tmp_path / "a"), a)
    PP.write_prepared(str(tmp_path / "b"), b)
    assert open(tmp_path / "a.data", "rb").read() == open(tmp_path / "b.data", "rb").read()
    assert open(tmp_path / "a.meantree", "rb").read() == open(tmp_path / "b.meantree", "rb").read()
    for spec in ("SparseMultivariateNormal 0.1", "FullMultivariateNormal", "NoLikelihood"):
        with pytest.raises(ValueError, match="glasso"):
            PP.prepare(mtcdnapri_paths["tree_list"], mtcdnapri_paths["rooted_tree"], spec, glasso="gpu")


def test_screening_claim_on_the_host_solver():
    """What the device solver's grid rests on, in numpy alone: graphical_lasso per connected component, assembled block-diagonally, is
    graphical_lasso on the whole matrix (here the two differed by 7e-11 in W and 2e-11 in Theta)."""
    S = GI.inputs()["blocks"]
    W_all, T_all = GI.host_solution("blocks")
    lab = GI.block_labels()
    W = np.zeros_like(S)
    T = np.zeros_like(S)
    for c in range(lab.max() + 1):
        idx = np.flatnonzero(lab == c)
        w, t = PP.graphical_lasso(S[np.ix_(idx, idx)], GI.RHO)
        W[np.ix_(idx, idx)] = w
        T[np.ix_(idx, idx)] = t
    print("screening: max |dW| %.3g, max |dTheta| %.3g" % (np.abs(W - W_all).max(), np.abs(T - T_all).max()))
    assert np.abs(W - W_all).max() <= 1e-8 and np.abs(T - T_all).max() <= 1e-7
    assert np.array_equal(T != 0, T_all != 0)


# --- the host solver on the inputs that tests/test_gpu_glasso.py compares the device with: what makes it a reference there

@pytest.mark.parametrize("name", ["C16", "C48", "S3"])
@pytest.mark.parametrize("pen", [True, False])
def test_host_solver_on_unequal_diagonals_and_three_variables(name, pen):
    """tests/test_prepare.py:138-144's conditions with its tolerances, and the premise of the pattern comparison of the gpu tests: no
    non-zero of the host's Theta below 4e-5."""
    S = GI.inputs()[name]
    d = np.diag(S)
    assert name == "S3" or (d.min() < 0.3 and d.max() > 3.0)                  # the diagonal is far from constant
    W, T = GI.host_solution(name, pen)
    inv, diag, active, inactive, lam = GI.optimality_violations(S, W, T, GI.RHO, pen)
    smallest = np.abs(T[T != 0]).min()
    print(f"{name} pen={pen}: diagonal of S {d.min():.3g} ... {d.max():.3g}; |W Theta - I| {inv:.3g}, diagonal {diag:.3g}, active {active:.3g}, "
          f"inactive - rho {inactive:.3g}, min eig {lam:.3g}; smallest non-zero |Theta| {smallest:.3g}, max |W| {np.abs(W).max():.3g}, "
          f"max |Theta| {np.abs(T).max():.3g}")
    assert inv <= 1e-8 and diag <= 1e-12 and active <= 1e-7 and inactive <= 1e-9
    assert np.array_equal(T, T.T) and lam > 0
    assert smallest > 4e-5
    assert max(np.abs(W).max(), np.abs(T).max()) < 6.0                        # the absolute tolerances 1e-8, 1e-7 mean what they meant at 1


@pytest.mark.parametrize("s", [0.5, -0.5, 0.1000001])
def test_host_solver_two_variables_closed_form(s):
    """p = 2, |s| > rho: W = S + rho I with W_01 = s - rho sign s, Theta = W^-1.  A handful of fp64 roundings on O(1) numbers:
    16 eps max(1, max |Theta|) for both matrices."""
    S = GI.two_by_two(s)
    Wc, Tc = GI.closed_form_2x2(S, GI.RHO)
    W, T = PP.graphical_lasso(S, GI.RHO)
    bound = 16 * np.finfo(float).eps * max(1.0, np.abs(Tc).max())
    print(f"s = {s}: host against the closed form |dW| {np.abs(W - Wc).max():.3g}, |dTheta| {np.abs(T - Tc).max():.3g}, bound {bound:.3g}")
    assert np.abs(W - Wc).max() <= bound and np.abs(T - Tc).max() <= bound
    assert T[0, 1] != 0 and np.sign(T[0, 1]) == -np.sign(s)


def test_host_solver_without_a_penalty_inverts():
    """rho = 0: the soft threshold zeroes nothing, the optimum is W = S, Theta = S^-1 (the stopping tolerance 1e-10 limits the
    agreement, not rounding)."""
    S = GI.inputs()["S16"]
    W, T = PP.graphical_lasso(S, 0.0)
    dW, dT = np.abs(W - S).max(), np.abs(T - np.linalg.inv(S)).max()
    print(f"rho = 0: host |W - S| {dW:.3g}, |Theta - inv S| {dT:.3g}")
    assert dW <= 1e-8 and dT <= 1e-7
    assert np.all(T != 0)


def test_the_permuted_blocks_are_what_the_screening_finds():
    """GI.packed(): 8 components, every one of two or more variables scattered over the whole index range (no component is a run of
    consecutive indices), numbered by smallest member."""
    S, lab = GI.packed()
    assert S.shape == (962, 962) and np.bincount(lab).tolist() == list(GI.PACKED_BLOCKS)
    got = M.glasso_components(S, GI.RHO)
    assert np.array_equal(got, GI.by_smallest_member(lab))
    for c in range(got.max() + 1):
        m = np.flatnonzero(got == c)
        assert len(m) == 1 or m[-1] - m[0] > len(m) - 1                       # interleaved with the others, not a contiguous run
