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
