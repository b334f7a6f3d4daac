"""The graphical lasso on the device (mcd_glasso, csrc/k_glasso.hip) against the conditions that characterise its unique optimum --
tests/test_prepare.py:138-144's assertions with that test's tolerances -- and against the host solver prepare.graphical_lasso on the same
inputs (|dW| <= 1e-8, |dTheta| <= 1e-7, the project's solver-against-solver tolerances, tests/test_prepare.py:151; equal zero patterns:
every non-zero of the host's Theta on these inputs is above 4e-5, so a pattern difference is a defect, not rounding)."""
import json
import os
import warnings

import numpy as np
import pytest

import glasso_inputs as GI
import mcmc_date_amd as M
from mcmc_date_amd import prepare as PP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("S16", True), ("S16", False), ("S11", True), ("S11", False), ("S70", True), ("S70s", True), ("blocks", True)]


def assert_optimal(S, W, T, rho, pen, label):
    inv, diag, active, inactive, lam = GI.optimality_violations(S, W, T, rho, pen)
    print(f"{label}: |W Theta - I| {inv:.3g}, diagonal {diag:.3g}, active {active:.3g}, inactive - rho {inactive:.3g}, min eig {lam:.3g}")
    assert inv <= 1e-8
    assert diag <= 1e-12
    assert active <= 1e-7
    assert inactive <= 1e-9
    assert np.array_equal(T, T.T) and lam > 0


@pytest.mark.parametrize("name,pen", CASES)
def test_optimality_and_host_solver(gpu, name, pen):
    S = GI.inputs()[name]
    W, T, info = M.graphical_lasso_device(S, GI.RHO, penalize_diagonal=pen, return_info=True)
    assert info["converged"] == 1 and info["sweep_cap_hit"] == 0 and info["passes"] >= 2
    assert_optimal(S, W, T, GI.RHO, pen, f"{name} pen={pen}")
    Wh, Th = GI.host_solution(name, pen)
    dW, dT = np.abs(W - Wh).max(), np.abs(T - Th).max()
    print(f"{name} pen={pen}: against the host max |dW| {dW:.3g}, max |dTheta| {dT:.3g}; passes {info['passes']}, updates {info['coordinate_updates']}, "
          f"smallest non-zero |Theta| {np.abs(Th[Th != 0]).min():.3g}")
    assert dW <= 1e-8 and dT <= 1e-7
    assert np.array_equal(T != 0, Th != 0)


def test_blocks_are_independent_problems(gpu):
    S = GI.inputs()["blocks"]
    W, T, info = M.graphical_lasso_device(S, GI.RHO, return_info=True)
    assert info["n_components"] == 5 and info["largest_component"] == 33 and info["n_problems"] == 3
    lab = GI.block_labels()
    between = lab[:, None] != lab[None, :]
    assert np.all(W[between] == 0.0) and np.all(T[between] == 0.0)
    for i in np.flatnonzero(np.bincount(lab)[lab] == 1):
        assert W[i, i] == 1.0 + GI.RHO and T[i, i] == 1.0 / (1.0 + GI.RHO)
    assert len(np.flatnonzero(np.bincount(lab)[lab] == 1)) == 2


def test_one_size_above_the_lane_stride(gpu):
    """p = lane stride + 1: thread 0 owns two coordinates, the second stride holds one.  The optimality conditions only (the host solver
    is too slow to serve as reference at this size)."""
    p = PP.GLASSO_LANE_STRIDE + 1
    assert p <= 1100
    S = np.corrcoef(GI.ar(np.random.default_rng(7), p, 400), rowvar=False)
    assert M.glasso_components(S, GI.RHO).max() == 0
    W, T, info = M.graphical_lasso_device(S, GI.RHO, return_info=True)
    assert info["converged"] == 1 and info["largest_component"] == p
    assert_optimal(S, W, T, GI.RHO, True, f"p = {p}")


def test_same_bits_on_every_call(gpu):
    S = GI.inputs()["S70"]
    a = M.graphical_lasso_device(S, GI.RHO, return_info=True)
    b = M.graphical_lasso_device(S, GI.RHO, return_info=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_max_iter_reached_is_reported_not_raised(gpu):
    S = GI.inputs()["S70"]
    with pytest.warns(RuntimeWarning, match="not converged"):
        W, T, info = M.graphical_lasso_device(S, GI.RHO, max_iter=1, return_info=True)
    assert info["converged"] == 0 and info["passes"] == 1 and np.all(np.isfinite(W)) and np.all(np.isfinite(T))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M.graphical_lasso_device(S, GI.RHO)                  # converged: no warning


def test_prepare_sparse_on_the_device_end_to_end(gpu, tmp_path):
    """`prepare ... "SparseMultivariateNormal 0.1"` on the reference's mtCDNApri trees with glasso="device" against glasso="host": the same
    association-list pattern, entries within 1e-7 max |P|, ln det within 1e-6 relative (tests/test_prepare.py:176's tolerance), and the ln
    likelihood of states through SparseTreeLikelihood within the bound those two imply:
        |d ll| <= 1/2 |d logdet| + 1/2 max |dP| (sum |dx|)^2 + rounding <= 1/2 1e-6 |logdet| + 1/2 1e-7 max |P| (sum |dx|)^2 + 1e-11 |ll|."""
    import oracle as O

    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "mtCDNApri_prior_samples.json")))
    paths = {}
    for k in ("rooted_tree", "tree_list"):
        paths[k] = str(tmp_path / k)
        open(paths[k], "w").write(fx["inputs"][k])
    h = PP.prepare(paths["tree_list"], paths["rooted_tree"], "SparseMultivariateNormal 0.1", glasso="host")
    d = PP.prepare(paths["tree_list"], paths["rooted_tree"], "SparseMultivariateNormal 0.1", glasso="device")
    assert isinstance(d.lhd, M.Sparse) and [ij for ij, _ in d.lhd.sigma_inv_assoc] == [ij for ij, _ in h.lhd.sigma_inv_assoc]
    vh = np.array([v for _, v in h.lhd.sigma_inv_assoc])
    vd = np.array([v for _, v in d.lhd.sigma_inv_assoc])
    pmax = np.abs(vh).max()
    assert np.abs(vd - vh).max() <= 1e-7 * pmax
    assert abs(d.lhd.logdet_sigma - h.lhd.logdet_sigma) <= 1e-6 * abs(h.lhd.logdet_sigma)
    topo = h.topology
    rng = np.random.default_rng(1)
    st = M.StateBatch.from_states([M.init_with(topo, h.mean_lengths)] * 5)
    st.time_height = np.array([15.0, 17.0, 19.0, 21.0, 30.0])
    st.rate_mean = np.full(5, 0.004)
    st.rates = st.rates * np.exp(0.2 * rng.standard_normal(st.rates.shape))
    ll_h, _ = M.SparseLikelihood(h.lhd).bind_tree(topo).loglik(st)
    ll_d, _ = M.SparseLikelihood(d.lhd).bind_tree(topo).loglik(st)
    ll_h, ll_d = np.asarray(ll_h), np.asarray(ll_d)
    for b in range(5):
        dx = O.distances(topo.parent, st.heights[b], st.rates[b], st.time_height[b], st.rate_mean[b]) - h.mu
        bound = 0.5e-6 * abs(h.lhd.logdet_sigma) + 0.5e-7 * pmax * np.abs(dx).sum() ** 2 + 1e-11 * abs(ll_h[b])
        print(f"state {b}: ll host {ll_h[b]:.12g}, device {ll_d[b]:.12g}, difference {abs(ll_d[b] - ll_h[b]):.3g}, bound {bound:.3g}")
        assert abs(ll_d[b] - ll_h[b]) <= bound
