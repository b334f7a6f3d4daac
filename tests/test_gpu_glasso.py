"""The graphical lasso on the device (mcd_glasso, csrc/k_glasso.hip) against the conditions that characterise its unique optimum --
tests/test_prepare.py:138-144's assertions with that test's tolerances -- and against the host solver prepare.graphical_lasso on the same
inputs (|dW| <= 1e-8, |dTheta| <= 1e-7, the project's solver-against-solver tolerances, tests/test_prepare.py:151; equal zero patterns:
every non-zero of the host's Theta on these inputs is above 4e-5, so a pattern difference is a defect, not rounding).

Beyond the host solver's reach the optimality conditions alone are the reference: every stride count of the kernel (1, 2, 3, 5, 8
coordinates per thread) and every size that fills its last stride, diagonals that differ from coordinate to coordinate, components whose
members are scattered over the matrix and differ in stride count within one launch, the smallest problems against their closed forms, and
rho = 0."""
import functools
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
CASES = [("S16", True), ("S16", False), ("S11", True), ("S11", False), ("S70", True), ("S70s", True), ("blocks", True),
         ("C16", True), ("C16", False), ("C48", True), ("C48", False)]


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


# --- every stride count, and the sizes that fill their last stride

@pytest.mark.parametrize("p", GI.STRIDE_SIZES)
def test_every_stride_count(gpu, p):
    """One component of p = 256, 512, 513, 1025, 2048 variables: a thread owns 1, 2, 3, 5, 8 coordinates, and 256, 512 and 2048
    (the limit) are whole multiples of the lane stride.  The optimality conditions only, as at p = 257; both halves of W come from one
    value, so W is symmetric to the bit."""
    S = GI.stride_input(p)
    assert -(-p // PP.GLASSO_LANE_STRIDE) in (1, 2, 3, 5, 8) and p <= M._capi.MCD_GLASSO_MAX_DIM
    assert M.glasso_components(S, GI.RHO).max() == 0
    W, T, info = M.graphical_lasso_device(S, GI.RHO, return_info=True)
    print(f"p = {p}: passes {info['passes']}, updates {info['coordinate_updates']}, non-zeros of Theta {int((T != 0).sum())}")
    assert info["converged"] == 1 and info["sweep_cap_hit"] == 0 and info["largest_component"] == p
    assert_optimal(S, W, T, GI.RHO, True, f"p = {p}")
    assert np.array_equal(W, W.T)


# --- unequal diagonals in the second stride

def test_unequal_diagonals_in_the_second_stride(gpu):
    """C300: a covariance with diagonal 0.23 ... 4.1 in one component of 300 variables, so the coordinates 256 ... 299 divide by a W_kk
    that differs from the one of the same thread's first coordinate.  The optimality conditions only."""
    S = GI.c300()
    d = np.diag(S)
    assert d.min() < 0.3 and d.max() > 3.0 and M.glasso_components(S, GI.RHO).max() == 0
    for pen in (True, False):
        W, T, info = M.graphical_lasso_device(S, GI.RHO, penalize_diagonal=pen, return_info=True)
        print(f"C300 pen={pen}: passes {info['passes']}, updates {info['coordinate_updates']}")
        assert info["converged"] == 1 and info["sweep_cap_hit"] == 0 and info["largest_component"] == 300
        assert_optimal(S, W, T, GI.RHO, pen, f"C300 pen={pen}")
        assert np.array_equal(W, W.T)


# --- packing: interleaved members, mixed stride counts in one launch

@functools.lru_cache(maxsize=None)
def packed_joint():
    """(W, Theta, info) of one call on GI.packed(), read-only."""
    W, T, info = M.graphical_lasso_device(GI.packed()[0], GI.RHO, return_info=True)
    W.setflags(write=False)
    T.setflags(write=False)
    return W, T, info


def packed_members():
    """The member lists of GI.packed()'s components of two or more variables, by block size."""
    lab = GI.packed()[1]
    return {GI.PACKED_BLOCKS[c]: np.flatnonzero(lab == c) for c in range(len(GI.PACKED_BLOCKS)) if GI.PACKED_BLOCKS[c] > 1}


def test_packed_components_scatter_and_optimum(gpu):
    """Components of 2, 3, 33, 65, 257 and 600 variables and two singletons, permuted: the partition, exact zeros between components,
    the singletons' closed form, and the optimality conditions on the whole matrix."""
    S, lab = GI.packed()
    W, T, info = packed_joint()
    assert info["n_components"] == 8 and info["n_problems"] == 6 and info["largest_component"] == 600
    assert info["converged"] == 1 and info["sweep_cap_hit"] == 0
    assert np.array_equal(M.glasso_components(S, GI.RHO), GI.by_smallest_member(lab))
    between = lab[:, None] != lab[None, :]
    assert np.all(W[between] == 0.0) and np.all(T[between] == 0.0)
    single = np.flatnonzero(np.bincount(lab)[lab] == 1)
    assert len(single) == 2
    for i in single:
        assert W[i, i] == S[i, i] + GI.RHO and T[i, i] == 1.0 / (S[i, i] + GI.RHO)
    print(f"packed: passes {info['passes']}, updates {info['coordinate_updates']}")
    assert_optimal(S, W, T, GI.RHO, True, "packed")
    assert np.array_equal(W, W.T)


def test_packed_components_against_each_alone(gpu):
    """Every component's principal sub-matrix solved alone on the device, and the four small ones by the host solver, against the joint
    call's block: |dW| <= 1e-8, |dTheta| <= 1e-7, equal zero patterns (not the same bits: the stopping rule is global, the joint call
    gives the small components extra passes)."""
    S = GI.packed()[0]
    W, T, _ = packed_joint()
    for p, m in packed_members().items():
        sub = np.ascontiguousarray(S[np.ix_(m, m)])
        others = [("device", M.graphical_lasso_device(sub, GI.RHO))]
        if p <= 65:
            others.append(("host", PP.graphical_lasso(sub, GI.RHO)))
        for who, (w, t) in others:
            dW, dT = np.abs(W[np.ix_(m, m)] - w).max(), np.abs(T[np.ix_(m, m)] - t).max()
            print(f"packed, component of {p}: joint against {who} alone max |dW| {dW:.3g}, max |dTheta| {dT:.3g}")
            assert w.shape == (p, p) and dW <= 1e-8 and dT <= 1e-7
            assert np.array_equal(T[np.ix_(m, m)] != 0, t != 0)


def test_packed_same_bits_under_a_fixed_pass_count(gpu):
    """Four outer passes for everybody (max_iter = 4, not converged): the components of 33, 65, 257 and 600 variables in one launch give
    the bits that each gives alone -- workgroups do not communicate and every sum is in index order.  A wrong offset into the packed
    arrays, a problem reading its neighbour's coefficients or a Theta kernel indexing by the launch's largest dimension breaks this.
    (max_iter also caps the sweeps of a column's descent, so sweep_cap_hit is expected here and is not asserted.)"""
    S = GI.packed()[0]
    mem = {p: m for p, m in packed_members().items() if p >= 33}
    idx = np.sort(np.concatenate(list(mem.values())))
    assert len(idx) == 33 + 65 + 257 + 600

    def four_passes(A):
        with pytest.warns(RuntimeWarning, match="not converged"):
            W, T, info = M.graphical_lasso_device(np.ascontiguousarray(A), GI.RHO, max_iter=4, return_info=True)
        assert info["passes"] == 4 and info["converged"] == 0
        return W, T, info

    W, T, info = four_passes(S[np.ix_(idx, idx)])
    assert info["n_problems"] == 4 and info["n_components"] == 4
    for p, m in mem.items():
        w, t, _ = four_passes(S[np.ix_(m, m)])
        at = np.searchsorted(idx, m)
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(t)) and np.count_nonzero(t) > p
        assert W[np.ix_(at, at)].tobytes() == w.tobytes(), f"W of the component of {p}"
        assert T[np.ix_(at, at)].tobytes() == t.tobytes(), f"Theta of the component of {p}"


# --- the smallest problems and the paths without a launch

@pytest.mark.parametrize("s", [0.5, -0.5, 0.1000001])
def test_two_variables_closed_form(gpu, s):
    """p = 2: one wave owns both coordinates, three own none and still take part in every ballot and barrier.  W = S + rho I with
    W_01 = s - rho sign s, Theta = W^-1; a handful of fp64 roundings on O(1) numbers: 16 eps max(1, max |Theta|) for both."""
    S = GI.two_by_two(s)
    Wc, Tc = GI.closed_form_2x2(S, GI.RHO)
    W, T, info = M.graphical_lasso_device(S, GI.RHO, return_info=True)
    bound = 16 * np.finfo(float).eps * max(1.0, np.abs(Tc).max())
    print(f"s = {s}: device against the closed form |dW| {np.abs(W - Wc).max():.3g}, |dTheta| {np.abs(T - Tc).max():.3g}, bound {bound:.3g}; "
          f"passes {info['passes']}")
    assert info["n_problems"] == 1 and info["largest_component"] == 2 and info["converged"] == 1 and info["sweep_cap_hit"] == 0
    assert np.abs(W - Wc).max() <= bound and np.abs(T - Tc).max() <= bound
    assert np.array_equal(W, W.T) and np.array_equal(T, T.T) and T[0, 1] != 0


@pytest.mark.parametrize("pen", [True, False])
def test_three_variables(gpu, pen):
    S = GI.inputs()["S3"]
    assert np.abs(S[~np.eye(3, dtype=bool)]).min() > GI.RHO
    W, T, info = M.graphical_lasso_device(S, GI.RHO, penalize_diagonal=pen, return_info=True)
    assert info["converged"] == 1 and info["sweep_cap_hit"] == 0 and info["largest_component"] == 3 and info["n_problems"] == 1
    assert_optimal(S, W, T, GI.RHO, pen, f"S3 pen={pen}")
    Wh, Th = GI.host_solution("S3", pen)
    dW, dT = np.abs(W - Wh).max(), np.abs(T - Th).max()
    print(f"S3 pen={pen}: against the host max |dW| {dW:.3g}, max |dTheta| {dT:.3g}; passes {info['passes']}")
    assert dW <= 1e-8 and dT <= 1e-7
    assert np.array_equal(T != 0, Th != 0)


@pytest.mark.parametrize("pen", [True, False])
def test_nothing_to_launch(gpu, pen):
    """All singletons (p = 2 with |s| = 0.05 < rho) and n = 1: no problem, no pass; W = diag S (+ rho), Theta its reciprocal, exactly."""
    for S in (GI.two_by_two(0.05), np.array([[1.7]])):
        n = S.shape[0]
        W, T, info = M.graphical_lasso_device(S, GI.RHO, penalize_diagonal=pen, return_info=True)
        assert info["n_problems"] == 0 and info["converged"] == 1 and info["passes"] == 0
        assert info["n_components"] == n and info["largest_component"] == 1 and info["coordinate_updates"] == 0
        d = np.diag(S) + (GI.RHO if pen else 0.0)
        assert np.array_equal(W, np.diag(d)) and np.array_equal(T, np.diag(1.0 / d))


# --- no penalty

def test_without_a_penalty_inverts(gpu):
    """rho = 0: nothing is thresholded, the optimum is W = S, Theta = S^-1; the stopping tolerance limits the agreement."""
    S = GI.inputs()["S16"]
    W, T, info = M.graphical_lasso_device(S, 0.0, return_info=True)
    Wh, Th = PP.graphical_lasso(S, 0.0)
    figures = (np.abs(W - S).max(), np.abs(T - np.linalg.inv(S)).max(), np.abs(W - Wh).max(), np.abs(T - Th).max())
    print("rho = 0: |W - S| %.3g, |Theta - inv S| %.3g, against the host |dW| %.3g, |dTheta| %.3g; passes %d" % (*figures, info["passes"]))
    assert info["converged"] == 1 and info["n_problems"] == 1 and info["largest_component"] == 16
    assert figures[0] <= 1e-8 and figures[1] <= 1e-7
    assert figures[2] <= 1e-8 and figures[3] <= 1e-7
    assert np.all(T != 0)
