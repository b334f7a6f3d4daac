"""The 50-digit reference of the prior gradient (tests/golden/prior_grad_reference*.npz) checked on the host: it loads, it is
finite, its VALUES are the ones of the pinned C oracle of the prior (oracle/prior_oracle.c) -- which ties the mpmath restatement
of tests/golden/make_prior_grad_reference.py to the reference's value function -- and, where mpmath is installed, the committed
arrays are what the generator produces today (a stale fixture would otherwise test yesterday's function)."""
import importlib.util
import os

import numpy as np
import pytest

import oracle as O
import prior_grad_reference as PG

CASES = {which: PG.load(which) for which in PG.FILES}
ALL = [(which, name) for which in CASES for name in CASES[which]]


def spec_of(c, model):
    cal = [(int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for r in c["cal"]]
    con = [(int(r[0]), int(r[1]), r[2]) for r in c["con"]]
    ptr = c["brace_ptr"]
    br = [([int(v) for v in c["brace_nodes"][ptr[i]:ptr[i + 1]]], float(sd)) for i, sd in enumerate(c["brace_sd"])]
    return O.PriorSpec(c["parent"], float(c["ht"]), PG.MODELS[model], cal, con, br)


def test_the_cases_are_all_there():
    names = {name for _, name in ALL}
    assert names == {"n3", "n63", "n65", "n127", "n129", "n255", "n257", "n2047", "n65near", "n257near", "n257tables", "fx12", "fx24", "fx24near"}
    for n in (3, 63, 65, 127, 129, 255, 257):
        c = CASES["main"][f"n{n}"]
        assert len(c["parent"]) == n and len(c["tH"]) == 4 and list(c["models"]) == [0, 1, 2, 3]
        assert np.sum(c["tH"] == 1.0) == 1 and not np.any(c["near"])
        assert np.all(np.abs(c["birth"] - c["death"]) >= 0.1 * np.maximum(c["birth"], c["death"]))
    big = CASES["more"]["n2047"]
    assert len(big["parent"]) == 2047 and list(big["models"]) == [2, 3]
    t = CASES["main"]["n257tables"]
    assert len(t["cal"]) == 70 and len(t["con"]) == 70 and len(t["brace_sd"]) == 5
    for name in ("n65near", "n257near", "fx24near"):
        c = CASES["more"][name]
        assert np.all(c["near"] == 1) and np.all(c["death"] == 1.0) and list(c["birth"]) == [1.0, 1.0 + 3e-7, 1.0 - 9.9e-7]
        assert np.all(np.abs(c["birth"] - c["death"]) < 1e-6)
    for which in PG.FILES:
        assert os.path.getsize(os.path.join(PG.GOLDEN, PG.FILES[which])) <= 512 * 1024


@pytest.mark.parametrize("which,name", ALL)
def test_reference_is_finite_and_its_tolerances_follow_the_rule(which, name):
    c = CASES[which][name]
    B, n = c["H"].shape
    for m in (int(x) for x in c["models"]):
        g, tol = PG.reference(c, m), PG.tolerances(c, m)
        for k in PG.SCALARS + ["H", "R"]:
            assert g[k].shape == tol[k].shape == ((B, n) if k in ("H", "R") else (B,))
            assert np.all(np.isfinite(g[k])) and np.all(np.isfinite(tol[k])) and np.all(tol[k] >= 0)
        for k in PG.SCALARS:                                         # the stored tolerances are the rule applied to the stored A and E53
            assert np.array_equal(c["tol_" + k][:, m], 64 * PG.U * c["A_" + k][:, m] + 8 * c["e53_" + k][:, m])
            assert np.all(c["A_" + k][:, m] >= np.abs(g[k]) * (1 - 1e-15))
        assert np.all(c["AH_" + PG.hkey(m)] >= np.abs(g["H"]) * (1 - 1e-15))
        assert np.all(g["R"][:, 0] == 0.0) and np.array_equal(g["rMu"], np.full(B, -float(c["ht"])))
        # the caps the generator holds the rule to (they come from the reference alone)
        for b in range(B):
            for k in PG.SCALARS + ["H", "R"]:
                cap = 1e-10 * max(1.0, np.abs(np.atleast_1d(g[k][b])).max())
                if c["near"][b]:
                    cap = 1e-5 * max(1.0, abs(g[k][b])) if k in ("birth", "death") else 1e3 * cap
                assert np.all(tol[k][b] <= cap), (name, m, b, k)
        assert np.all(np.isfinite(c["lp"][:, m]))
    missing = [m for m in range(4) if m not in c["models"]]
    assert all(np.all(np.isnan(c["lp"][:, m])) for m in missing)


def test_near_critical_chains_tell_the_old_arrangement_of_the_duals_from_the_new():
    """fp64 arithmetic (mpmath at 53 bits) in the arrangement the kernel's birth-death duals had before they used expm1 misses
    the stored tolerance of g_birth and g_death on every near-critical chain: the GPU test can tell the defect from its fix."""
    for name in ("n65near", "n257near", "fx24near"):
        c = CASES["more"][name]
        for m in range(4):
            for k in ("birth", "death"):
                assert np.all(np.abs(c["g53k_" + k][:, m] - c["g_" + k][:, m]) > c["tol_" + k][:, m]), (name, m, k)
                assert np.all(c["e53_" + k][:, m] < 0.125 * c["tol_" + k][:, m] + 1e-300)


@pytest.mark.parametrize("which,name", ALL)
def test_stored_values_are_the_oracles(which, name):
    """ln prior of every regular chain: mpmath restatement against the C oracle, the `close` rule of tests/test_gpu_prior.py."""
    c = CASES[which][name]
    for m in (int(x) for x in c["models"]):
        spec = spec_of(c, m)
        for b in np.flatnonzero(c["near"] == 0):
            lp, comp = O.prior(spec, c["birth"][b], c["death"][b], c["tH"][b], c["H"][b], c["rMu"][b], c["rVar"][b], c["R"][b])
            assert np.isfinite(lp) and abs(c["lp"][b, m] - lp) <= 1e-11 * max(1.0, abs(lp)), (name, m, b, c["lp"][b, m], lp)
            assert abs(c["node_prior"][b, m] - comp[0]) <= 1e-11 * max(1.0, abs(comp[0])), (name, m, b)


def test_committed_fixture_is_what_the_generator_writes():
    pytest.importorskip("mpmath")
    path = os.path.join(PG.GOLDEN, "make_prior_grad_reference.py")
    spec = importlib.util.spec_from_file_location("make_prior_grad_reference", path)
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    only = {"n3": [0, 1, 2, 3], "n65": [2]}
    new = G.generate("main", only=only)
    for name, idx in only.items():
        old = CASES["main"][name]
        assert set(new[name]) == set(old)
        for k, a in new[name].items():
            want = old[k] if k in PG.SHARED else old[k][idx]
            assert a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes(), (name, k)
