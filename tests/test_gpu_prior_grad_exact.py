"""k_prior_grad.hip against the 50-digit reference of tests/golden/prior_grad_reference*.npz (written on the host by
tests/golden/make_prior_grad_reference.py; nothing here needs mpmath, the reference tree or an oracle).

Every output component k is held to the tolerance the fixture carries,
    tol_k = 64 * 2^-53 * A_k + 8 * max(E53 over that chain's output array),
A_k = sum of the absolute addends of the component, E53 = error of the same formulas in correctly rounded fp64 arithmetic; it
is derived from the reference alone.  ln prior: the `close` rule of tests/test_gpu_prior.py (1e-11), regular chains only (a
near-critical chain's VALUE is the reference's first-order formula, its gradient the exact formulas at the regime's edge).
Each test prints its worst err / tol per output array before it asserts (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest

import mcmc_date_amd as M
import prior_grad_reference as PG
from mcmc_date_amd import _capi

pytestmark = pytest.mark.gpu

CASES = {name: c for which in PG.FILES for name, c in PG.load(which).items()}
CASE_MODEL = [(name, int(m)) for name, c in CASES.items() for m in c["models"]]
KEYS = {"birth": "time_birth_rate", "death": "time_death_rate", "tH": "time_height", "H": "heights", "rMu": "rate_mean",
        "rVar": "rate_variance", "R": "rates"}
OUT = ["birth", "death", "tH", "H", "rMu", "rVar", "R"]              # the order of the C ABI's gradient outputs


def prior_function(c, model):
    cal = [M.Calibration(f"c{i}", int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for i, r in enumerate(c["cal"])]
    con = [M.Constraint(f"k{i}", int(r[0]), int(r[1]), r[2]) for i, r in enumerate(c["con"])]
    ptr = c["brace_ptr"]
    br = [M.Brace(f"b{i}", [int(v) for v in c["brace_nodes"][ptr[i]:ptr[i + 1]]], float(s)) for i, s in enumerate(c["brace_sd"])]
    return M.PriorFunction(float(c["ht"]), PG.MODELS[model], cal, con, br, M.Topology(c["parent"]))


def batch_of(c, idx=slice(None)):
    return M.StateBatch(c["H"][idx], c["R"][idx], c["tH"][idx], c["rMu"][idx], c["birth"][idx], c["death"][idx], c["rVar"][idx])


def worst(label, dev, c, model):
    """Prints the worst err / tol of every output array of `dev` (name -> [B] or [B, n]); returns the misses."""
    ref, tol = PG.reference(c, model), PG.tolerances(c, model)
    bad = []
    for k in OUT:
        d = np.asarray(dev[k], float)
        assert d.shape == ref[k].shape, (label, k, d.shape)
        err = np.abs(d - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / tol[k])
        ratio = np.where(np.isfinite(d), ratio, np.inf)
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"prior-grad-exact {label} model {model} g_{k}: worst err/tol {ratio[at]:.3g} at {tuple(int(i) for i in at)} "
              f"(err {err[at]:.3e}, tol {tol[k][at]:.3e}, reference {ref[k][at]:.17g})")
        if not ratio[at] <= 1.0:
            bad.append((k, float(ratio[at]), tuple(int(i) for i in at)))
    return bad


def close(a, b, rtol=1e-11):
    return np.all(np.isfinite(a)) and np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("name,model", CASE_MODEL)
def test_every_case_and_model(gpu, name, model):
    c = CASES[name]
    pf = prior_function(c, model)
    s = batch_of(c)
    lp, g = pf.grad(s)
    assert np.array_equal(lp, pf.logprior(s))                               # the value kernel's bits
    regular = c["near"] == 0
    assert np.all(np.isfinite(lp)) and close(lp[regular], c["lp"][regular, model]), (lp, c["lp"][:, model])
    bad = worst(name, {k: g[KEYS[k]] for k in OUT}, c, model)
    assert not bad, (name, model, bad)


def grad_c_abi(pf, c, batch, pad=3):
    """mcd_prior_grad_batch on host arrays with ld_state = n_nodes + pad: the case's chains tiled to `batch`, the padding of the
    inputs NaN, the padding of the outputs a mark that has to survive."""
    B, n = c["H"].shape
    idx = np.arange(batch) % B
    ld = n + pad
    H, R = np.full((batch, ld), np.nan), np.full((batch, ld), np.nan)
    H[:, :n], R[:, :n] = c["H"][idx], c["R"][idx]
    sc = {k: np.ascontiguousarray(c[k][idx]) for k in PG.SCALARS}
    out = {k: np.full((batch, ld) if k in ("H", "R") else batch, 7.25) for k in ["lp"] + OUT}
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.check(_capi.lib().mcd_prior_grad_batch(pf._p, p(sc["birth"]), p(sc["death"]), p(sc["tH"]), p(H), p(sc["rMu"]), p(sc["rVar"]), p(R),
                                                 ld, batch, 0, None, p(out["lp"]), *[p(out[k]) for k in OUT]))
    for k in ("H", "R"):
        assert np.all(out[k][:, n:] == 7.25), k                             # nothing is written beyond a chain's n_nodes
        out[k] = out[k][:, :n]
    return out


def check_batches(name, models, batches):
    c = CASES[name]
    B = len(c["tH"])
    for model in models:
        pf = prior_function(c, model)
        first = None
        for batch in batches:
            out = grad_c_abi(pf, c, batch)
            for k in ["lp"] + OUT:                                          # every replica of a chain: the bits of its first copy
                for b in range(min(B, batch)):
                    rep = out[k][b::B]
                    assert np.array_equal(rep, np.broadcast_to(rep[:1], rep.shape)), (name, model, batch, k, b)
            head = {k: out[k][:min(B, batch)] for k in ["lp"] + OUT}
            if first is None:
                first = head
                assert len(head["lp"]) == B
                bad = worst(f"{name} x{batch}", head, c, model)
                assert not bad, (name, model, batch, bad)
            else:                                                           # ... and the same bits whatever the waves per chain
                for k in head:
                    assert np.array_equal(head[k], first[k][:len(head[k])]), (name, model, batch, k)


@pytest.mark.parametrize("name", ["n3", "n63", "n65", "n127", "n129", "n255", "n257"])
def test_every_wave_count(gpu, name):
    """The launcher gives a chain min(ceil(n / 64), 4, 2048 / batch) waves: batches of 8, 600, 700 and 1100 chains are 4, 3, 2 and 1
    waves on a tree of 193 nodes or more (3 waves: 192 threads at stride 192, which no other test reaches), fewer on smaller trees."""
    check_batches(name, range(4), (8, 600, 700, 1100))


def test_every_wave_count_at_2047_nodes(gpu):
    """kPriorGradMaxNodes - 1 nodes: more than 64 KiB of LDS per workgroup; one chain alone, then 3 waves and 1 wave per chain."""
    check_batches("n2047", (2, 3), (1, 600, 1100))


def test_large_tables(gpu):
    """70 calibrations, 70 constraints, 5 braces: prior_nodes_wave takes a second round of i += 64 and lane 0's serial loop is long."""
    name = "n257tables"
    c = CASES[name]
    assert len(c["cal"]) > 64 and len(c["con"]) > 64
    check_batches(name, range(4), (8, 1100))
    for model in (0, 3):
        pf = prior_function(c, model)
        lp, comp = pf.logprior(batch_of(c), want_components=True)
        assert close(comp[:, 0], c["node_prior"][:, model]), (comp[:, 0], c["node_prior"][:, model])
        assert close(lp, c["lp"][:, model])


@pytest.mark.parametrize("name", ["n65near", "n257near", "fx24near"])
def test_near_critical_chains(gpu, name):
    """birth = death = 1, birth = death + 3e-7, birth = death - 9.9e-7 on one state.  The first two take their gradient at the same
    la_d = fl(death + 1e-6): the same bits.  The third takes it at fl(death - 1e-6): the step of g_birth and g_death across
    birth = death is the reference's own step (the exact formulas 2e-6 apart) to within the two tolerances."""
    c = CASES[name]
    for model in range(4):
        pf = prior_function(c, model)
        lp, g = pf.grad(batch_of(c))
        bad = worst(name, {k: g[KEYS[k]] for k in OUT}, c, model)
        assert not bad, (name, model, bad)
        ref, tol = PG.reference(c, model), PG.tolerances(c, model)
        for k in ("birth", "death"):
            d = np.asarray(g[KEYS[k]])
            assert d[0] == d[1] and ref[k][0] == ref[k][1]
            step, step_ref = d[2] - d[0], ref[k][2] - ref[k][0]
            print(f"prior-grad-exact {name} model {model} g_{k}: step across birth = death {step:.6e} (reference {step_ref:.6e})")
            assert abs(step - step_ref) <= tol[k][2] + tol[k][0], (name, model, k, step, step_ref)
        assert np.array_equal(np.asarray(g["rates"])[0], np.asarray(g["rates"])[1])
