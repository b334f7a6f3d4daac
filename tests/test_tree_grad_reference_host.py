"""The 50-digit reference of the likelihood gradient (tests/golden/tree_grad_reference*.npz) and its tolerance rule
(tests/tree_grad_reference.py) checked on the host:

* the same route in plain numpy fp64 stays within a quarter of every tolerance (the device has room; a larger ratio would mean that the
  construction of A is wrong), and the worst ratio per case is printed;
* the tolerances have teeth: each of seven defects a hand-written chain rule can have, applied to that fp64 route, misses its
  tolerance on every case it applies to;
* the pinned C oracle (oracle/mvn_oracle.c: orc_tree_grad_full, orc_tree_loglik_full_batch) agrees with the stored values to its own
  accuracy, 1e-9 x the largest entry;
* where mpmath is installed, the committed arrays of two small cases are what the generator produces today."""
import importlib.util
import os

import numpy as np
import pytest

import oracle as O
import tree_grad_reference as TG

CASES = TG.load_all()
NAMES = sorted(CASES)
MUTATIONS = ["drop_last_child_of_3", "drop_only_child", "root_right_out_of_gd", "exchange_root_children", "neighbour_slot_parent",
             "omit_17th_entry", "scale_component_of_b"]


def ratios(out, case, sparse=None):
    """name -> (worst err / tol, index) of every output array."""
    ref, tol = TG.reference(case), TG.tolerances(case, sparse)
    worst = {}
    for k in TG.OUTPUTS:
        err = np.abs(np.asarray(out[k]) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / tol[k])
        r = np.where(np.isfinite(np.asarray(out[k])), r, np.inf)
        at = np.unravel_index(np.argmax(r), r.shape)
        worst[k] = (float(r[at]), tuple(int(i) for i in at))
    return worst


def routes(case):
    """The handles a case is evaluated through: its own, and for the cases of the position layout the sparse one as well."""
    return [None, True] if not TG.is_sparse(case) and "jac_tH" in case else [None]


def test_the_cases_are_all_there():
    dense = sorted(len(c["parent"]) - 2 for n, c in CASES.items() if n.startswith("d"))
    sparse = sorted(len(c["parent"]) - 2 for n, c in CASES.items() if n.startswith("s"))
    assert set(dense) >= {1, 5, 63, 64, 65, 129, 200, 255, 256, 257, 390, 513, 769, 1022} and max(dense) == 1022
    assert set(sparse) >= {1, 255, 256, 257, 1022, 2046} and max(sparse) == 2046
    assert {n for n in CASES if n.startswith("p_")} == {"p_n3", "p_n65", "p_n257", "p_fx24"}
    for name, c in CASES.items():
        nn = len(c["parent"])
        if not name.startswith("p_"):
            assert len(c["tH"]) == (6 if nn <= 257 else 4) and c["tH"][1] == 1.0
        assert c["H"].shape == c["R"].shape == c["gH"].shape == c["gR"].shape == (len(c["tH"]), nn)
        assert np.all(c["H"][:, c["parent"][1:]] > c["H"][:, 1:]) and np.all(c["H"][:, 0] == 1.0)          # valid height trees
        for k in TG.OUTPUTS:
            assert np.all(np.isfinite(c[k])), (name, k)
        assert np.all(c["gR"][:, 0] == 0.0)
    for fname in TG.FILES.values():
        assert os.path.getsize(os.path.join(TG.GOLDEN, fname)) <= 512 * 1024, fname


@pytest.mark.parametrize("name", NAMES)
def test_matrices_are_what_their_families_promise(name):
    c = CASES[name]
    P, mu = TG.matrix(c)                                                            # (asserts the stored SHA-256)
    family, n = int(c["family"]), len(P)
    assert mu.shape == (n,)
    if family < 3:
        assert np.array_equal(P, P.T) and np.array_equal(P * 2.0 ** 3, np.round(P * 2.0 ** 3))          # integers over 8
        K = P
        if family == 1:
            D = 2.0 ** (np.arange(n) % 12)
            K = P / D[:, None] / D[None, :]
            assert n < 12 or P.max() / np.abs(P).min() >= 2.0 ** 22
        assert np.all(np.diag(K) > np.abs(K).sum(axis=1) - np.diag(K))               # strictly diagonally dominant
    if family < 2:
        assert np.all(P != 0)
    if family == 2 and n >= 64:
        counts = np.count_nonzero(P, axis=1)
        assert [int(counts[r]) for r, _ in TG.special_rows(n)] == [17, 40, 16] and counts.max() == 40 == TG.longest_row(P)
        assert np.count_nonzero(P) < 12 * n


@pytest.mark.parametrize("name", NAMES)
def test_the_fp64_route_stays_within_a_quarter_of_the_tolerance(name):
    c = CASES[name]
    for sparse in routes(c):
        w = ratios(TG.numpy_fp64(c, sparse), c, sparse)
        print(f"tree-grad-reference {name}{' (sparse route)' if sparse else ''}: worst err/tol " + " ".join(f"{k} {r:.3g}" for k, (r, _) in w.items()))
        for k, (r, at) in w.items():
            assert r <= 0.25, (name, sparse, k, r, at)
    tol = TG.tolerances(c)
    ref = TG.reference(c)
    for k in TG.OUTPUTS:
        assert tol[k].shape == ref[k].shape and np.all(np.isfinite(tol[k])) and np.all(tol[k] >= 0)
    if "jac_tH" in c:                                                               # the derivatives of ln jacobianRootBranch in fp64
        T = TG.Tables(c["parent"])
        H, R, rr = c["H"], c["R"], T.root_right
        S = (H[:, 0] - H[:, 1]) * R[:, 1] + (H[:, 0] - H[:, rr]) * R[:, rr]
        jac = dict(jac_h0=-(R[:, 1] + R[:, rr]) / S, jac_hl=R[:, 1] / S, jac_hr=R[:, rr] / S, jac_rl=-(H[:, 0] - H[:, 1]) / S,
                   jac_rr=-(H[:, 0] - H[:, rr]) / S, jac_tH=-1.0 / c["tH"], jac_rMu=-1.0 / c["rMu"])
        for k in TG.JAC:
            assert np.all(np.abs(jac[k] - ref[k]) <= 0.25 * tol[k]), (name, k)


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_the_tolerances_have_teeth(mutation):
    applied = []
    for name in NAMES:
        c = CASES[name]
        for sparse in routes(c):
            out = TG.numpy_fp64(c, sparse, mutation=mutation)
            if out is None:
                continue
            w = ratios(out, c, sparse)
            applied.append(name)
            assert max(r for r, _ in w.values()) > 1.0, (mutation, name, sparse, w)
    print(f"tree-grad-reference {mutation}: caught on {len(applied)} cases")
    # how many cases each defect applies to: the trees with such a node, every tree (all but the three of 3 nodes, whose root children
    # are both leaves and whose only slot has no neighbour), the sparse matrices with the long row, the cases of family 1
    wanted = {"drop_last_child_of_3": 14, "drop_only_child": 14, "root_right_out_of_gd": len(NAMES), "exchange_root_children": len(NAMES) - 3,
              "neighbour_slot_parent": len(NAMES) - 3, "omit_17th_entry": 5, "scale_component_of_b": 9}
    assert len(set(applied)) == wanted[mutation], (mutation, sorted(set(applied)))


@pytest.mark.parametrize("name", NAMES)
def test_the_c_oracle_agrees(name):
    c = CASES[name]
    P, mu = TG.matrix(c)
    ll, lj = O.tree_loglik_full_batch(c["parent"], c["H"], c["R"], c["tH"], c["rMu"], mu, P, float(c["logdet"]))
    assert np.all(np.abs(ll - c["ll"]) <= 1e-9 * np.abs(c["ll"])) and np.all(np.abs(lj - c["logjac"]) <= 1e-9 * np.maximum(1.0, np.abs(c["logjac"])))
    for b in range(len(c["tH"])):
        gH, gR, gt, gm = O.tree_grad_full(c["parent"], c["H"][b], c["R"][b], c["tH"][b], c["rMu"][b], mu, P)
        sc = max(np.abs(c["gH"][b]).max(), np.abs(c["gR"][b]).max())
        assert np.max(np.abs(gH - c["gH"][b])) <= 1e-9 * sc and np.max(np.abs(gR - c["gR"][b])) <= 1e-9 * sc, (name, b)
        assert abs(gt - c["gtH"][b]) <= 1e-9 * abs(c["gtH"][b]) and abs(gm - c["grMu"][b]) <= 1e-9 * abs(c["grMu"][b]), (name, b)


def test_committed_fixture_is_what_the_generator_writes():
    pytest.importorskip("mpmath")
    path = os.path.join(TG.GOLDEN, "make_tree_grad_reference.py")
    spec = importlib.util.spec_from_file_location("make_tree_grad_reference", path)
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    only = {"d5mix": [0, 1, 2, 3, 4, 5], "s256": [2], "p_n3": [1]}
    new = G.generate(only=only)
    for name, idx in only.items():
        old = CASES[name]
        assert set(new[name]) == set(old)
        for k, a in new[name].items():
            want = old[k] if k in TG.SHARED else old[k][idx]
            assert a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes(), (name, k)
