"""The gradient of the ln likelihood with respect to the tree state -- k_tree_grad.hip, k_split.hip, k_wide_grad.hip, k_wide_grad_mc.hip,
k_sparse_grad.hip -- and the Hamiltonian target in position layout (k_hmc.hip, k_nuts.hip) against the 50-digit reference of
tests/golden/tree_grad_reference*.npz (written on the host by tests/golden/make_tree_grad_reference.py; nothing here needs mpmath, an
oracle or the reference tree).

Every chain and every component of ll, logjac, gH, gR, gtH and grMu is held to the tolerance of tests/tree_grad_reference.py,
    tol_k = 64 * m * 2^-53 * A_k,
A_k = the component's formula with every addend replaced by its absolute value, m = n for a dense handle, the longest row for gR and
gH of the sparse handle; it is derived from the stored inputs alone.  The trees are the ones the kernels carry code for and no other GPU
test runs: inner nodes with 3 and 5 children, inner nodes with one child, a leaf as the root's left or right child, nodes 256 and 257 of
k_wide_grad's tail.  Each test prints its worst err / tol per output array and form before it asserts (pytest -s shows them).

Measured on an MI355X (worst err / tol over all cases, batches and chains; this file: 40 tests in 3.6 s):
    form                     ll        gH        gR        gtH       grMu      ll (value call)  logjac
    sweep                    0.0219    0.0548    0.0507    0.0561    0.0568    0.0219           0.0103
    row split                0.000588  0.00302   0.00299   0.000365  0.00035   0.000588         0.000107
    multiply                 0.0219    0.0548    0.0507    0.0421    0.0452    0.0219           0.0103
    sparse, 1 and 2 chains   0.0552    0.0599    0.0488    0.0534    0.0483    0.0552           0.0154
    position layout          value 0.00098, gradient 0.571 (dense and sparse handle alike: the rate variance of n65, the prior gradient alone)
The largest ratios of sweep, multiply and sparse belong to the 3-node trees (n = 1, where the factor 64 n is smallest); no form misses a
tolerance on any tree, multifurcations and one-child nodes included.  What these tests did find: on a chain whose ln likelihood is NaN
the four dense forms wrote 0 into the stem rate's entry gR[., 0] where the sparse form writes NaN; they write NaN now
(test_one_poisoned_chain).
"""
import ctypes as C

import numpy as np
import pytest

import mcmc_date_amd as M
import prior_grad_reference as PG
import tree_grad_reference as TG
from mcmc_date_amd import _capi

pytestmark = pytest.mark.gpu

CASES = TG.load_all()
DENSE = [n for n in CASES if n.startswith("d")]
SPARSE = [n for n in CASES if n.startswith("s")]
MARK = 7.25
GRAD = ["ll", "gH", "gR", "gtH", "grMu"]

_handles, _tolerances = {}, {}


def handle(name, sparse=None):
    """The bound tree of a case over a dense (MvnLikelihood) or sparse (SparseLikelihood) handle, made once."""
    c = CASES[name]
    sparse = TG.is_sparse(c) if sparse is None else sparse
    if (name, sparse) not in _handles:
        P, mu = TG.matrix(c)
        topo = M.Topology(c["parent"])
        if sparse:
            lik = M.SparseLikelihood(M.Sparse(mu, TG.assoc_of(P), float(c["logdet"])))
        else:
            lik = M.MvnLikelihood(M.Full(mu, P, float(c["logdet"])))
        _handles[(name, sparse)] = lik.bind_tree(topo)
    return _handles[(name, sparse)]


def tolerances(name, sparse=None):
    c = CASES[name]
    sparse = TG.is_sparse(c) if sparse is None else sparse
    if (name, sparse) not in _tolerances:
        _tolerances[(name, sparse)] = TG.tolerances(c, sparse)
    return _tolerances[(name, sparse)]


def evaluate(gpu, tl, c, batch, poison=None, pad=3):
    """The case's chains tiled to `batch` through <api>_grad_batch and <api>_loglik_batch on device arrays with ld = n_nodes + pad: the
    padding of the inputs NaN, the padding of the outputs a mark that has to survive.  poison = (chain, node): that height is NaN.
    Returns name -> array of ll, gH, gR, gtH, grMu (the gradient call) and ll_value, logjac (the value call)."""
    import torch

    B, nn = c["H"].shape
    idx = np.arange(batch) % B
    ld = nn + pad
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=gpu)
    H = torch.full((batch, ld), np.nan, dtype=torch.float64, device=gpu)
    R = torch.full((batch, ld), np.nan, dtype=torch.float64, device=gpu)
    H[:, :nn], R[:, :nn] = dev(c["H"][idx]), dev(c["R"][idx])
    if poison is not None:
        H[poison[0], poison[1]] = np.nan
    tH, rMu = dev(c["tH"][idx]), dev(c["rMu"][idx])
    out = {k: torch.full((batch, ld) if k in ("gH", "gR") else (batch,), MARK, dtype=torch.float64, device=gpu)
           for k in GRAD + ["ll_value", "logjac"]}
    p = lambda t: C.c_void_p(t.data_ptr())
    api = "mcd_sparse_tree" if tl.sparse else "mcd_tree"
    lib = _capi.lib()
    _capi.check(getattr(lib, api + "_grad_batch")(tl._t, p(H), p(R), ld, p(tH), p(rMu), batch, 1, None, *[p(out[k]) for k in GRAD]))
    _capi.check(getattr(lib, api + "_loglik_batch")(tl._t, p(H), p(R), ld, p(tH), p(rMu), batch, 1, None, p(out["ll_value"]), p(out["logjac"])))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("gH", "gR"):
        assert np.all(out[k][:, nn:] == MARK), k                              # nothing is written beyond a chain's n_nodes
        out[k] = out[k][:, :nn]
    return out


def worst(label, out, name, sparse=None, chains=None):
    """Prints the worst err / tol of every output array of `out` (row i: chain chains[i] of the case, the first chains by default);
    returns the misses."""
    ref, tol = TG.reference(CASES[name]), tolerances(name, sparse)
    bad, line = [], []
    for k in GRAD + ["ll_value", "logjac"]:
        rk = "ll" if k == "ll_value" else k
        d = np.asarray(out[k], float)
        rows = np.arange(len(d)) if chains is None else chains
        r, t = ref[rk][rows], tol[rk][rows]
        assert d.shape == r.shape, (label, k, d.shape)
        err = np.abs(d - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / t)
        ratio = np.where(np.isfinite(d), ratio, np.inf)
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        line.append(f"{k} {ratio[at]:.3g}")
        if not ratio[at] <= 1.0:
            bad.append((k, float(ratio[at]), tuple(int(i) for i in at), float(err[at]), float(t[at]), float(r[at])))
    print(f"tree-grad-exact {label}: worst err/tol " + " ".join(line))
    return bad


PIECE = 1024                                                                     # kSplitMaxBatch: a larger batch of the row split goes in pieces


def check_batches(gpu, name, label, batches, sparse=None):
    """Every replica of a chain carries the bits of its first copy; the first copies are held to the reference.  A batch above PIECE
    (the row split from n = 769) is several launches, and the row split's number of row groups -- its order of summation -- follows the
    launch's batch (tests/test_gpu_split.py:101): there the replicas of every piece carry the bits of the piece's first copy, and the
    first copies of every piece are held to the reference."""
    c = CASES[name]
    tl = handle(name, sparse)
    B = len(c["tH"])
    heads = {}
    for batch in batches:
        out = evaluate(gpu, tl, c, batch)
        pieces = label == "split" and batch > PIECE
        for lo in range(0, batch, PIECE if pieces else batch):
            hi = min(batch, lo + PIECE) if pieces else batch
            first = np.arange(lo, min(hi, lo + B))                                  # the piece's first copy of every chain it holds
            for k, a in out.items():
                for at in first:
                    rep = a[at:hi:B]
                    assert np.array_equal(rep, np.broadcast_to(rep[:1], rep.shape)), (name, label, batch, lo, k, at % B)
            head = {k: a[first] for k, a in out.items()}
            bad = worst(f"{name} {label} x{batch}" + (f" piece at {lo}" if lo else ""), head, name, sparse, first % B)
            assert not bad, (name, label, batch, lo, bad)
            if lo == 0:
                heads[batch] = head
    return heads


# ---------------------------------------------------------------------------------------------------------------------------------
# the dense handle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DENSE)
def test_dense_forms(gpu, knobs, name):
    """The column sweep (n <= 768), the row split (MCD_SPLIT = 1 for 128 < n <= 256, the automatic choice above; from n = 769 a batch of
    1100 goes in pieces of 1024) and the multiply form (k_wide_grad up to n = 256, k_wide_grad_mc above; 40 and 4100 chains: 16 and 32 chains
    per workgroup).  Batches of 1, 7, 130 and 600: ragged tails for every chains-per-workgroup of the sweeps, a partly empty last tile."""
    n = len(CASES[name]["parent"]) - 2
    mvn = handle(name).mvn
    seen = {}
    try:
        if n <= 768:
            mvn.set_form("sweep")
            seen["sweep"] = check_batches(gpu, name, "sweep", (1, 7, 130, 600))
        mvn.set_form("auto")
        if n > 128:
            if n <= 256:
                knobs.setenv("MCD_SPLIT", 1)
            seen["split"] = check_batches(gpu, name, "split", (1, 7, 130, 600) + ((1100,) if n >= 769 else ()))
            knobs.delenv("MCD_SPLIT")
        mvn.set_form("multiply")
        seen["multiply"] = check_batches(gpu, name, "multiply", (40, 4100))
    finally:
        mvn.set_form("auto")
    if n > 128 and n <= 768:                                                    # really three kernels
        a, b, m = seen["sweep"][7]["gH"], seen["split"][7]["gH"], seen["multiply"][40]["gH"]
        assert not np.array_equal(a, b) and not np.array_equal(a, m) and not np.array_equal(b, m)


# ---------------------------------------------------------------------------------------------------------------------------------
# the sparse handle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SPARSE)
def test_sparse_handle(gpu, knobs, name):
    """One and two chains per workgroup give the same bits; the odd batches leave the last workgroup of two one live chain; the value call
    (mcd_sparse_tree_loglik_batch: another order of summation) is held to the same ll."""
    heads = {}
    for chains in (1, 2):
        knobs.setenv("MCD_SPARSE_GRAD_CHAINS", chains)
        heads[chains] = check_batches(gpu, name, f"sparse C={chains}", (1, 5, 513))
    for batch in heads[1]:
        for k in GRAD:
            assert np.array_equal(heads[1][batch][k], heads[2][batch][k]), (name, batch, k)


# ---------------------------------------------------------------------------------------------------------------------------------
# one poisoned chain
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("d63", "sweep"), ("d257", "split"), ("d255", "multiply"), ("d390", "multiply"), ("s256", "sparse1"),
                                       ("s256", "sparse2")])
def test_one_poisoned_chain(gpu, knobs, name, form):
    """A NaN height in chain 3 of a batch of 7: every output of that chain's gradient call is NaN, every other chain keeps the bits it has
    in the clean batch."""
    c = CASES[name]
    tl = handle(name)
    T = TG.Tables(c["parent"])
    node = int(T.slot_node[(T.n_nodes - 2) // 2])
    assert node not in (1, T.root_right)
    try:
        if form.startswith("sparse"):
            knobs.setenv("MCD_SPARSE_GRAD_CHAINS", int(form[-1]))
        else:
            tl.mvn.set_form("auto" if form == "split" else form)
        clean = evaluate(gpu, tl, c, 7)
        dirty = evaluate(gpu, tl, c, 7, poison=(3, node))
    finally:
        if not form.startswith("sparse"):
            tl.mvn.set_form("auto")
    for k in GRAD + ["ll_value"]:
        assert np.all(np.isnan(dirty[k][3])), (name, form, k, dirty[k][3])
        assert np.array_equal(np.delete(dirty[k], 3, axis=0), np.delete(clean[k], 3, axis=0)), (name, form, k)
    assert np.array_equal(dirty["logjac"], clean["logjac"])                     # (the node is no child of the root)


# ---------------------------------------------------------------------------------------------------------------------------------
# the target in position layout
# ---------------------------------------------------------------------------------------------------------------------------------
PRIOR = PG.load("main")
KEYS = {"birth": "time_birth_rate", "death": "time_death_rate", "tH": "time_height", "H": "heights", "rMu": "rate_mean",
        "rVar": "rate_variance", "R": "rates"}


def prior_function(c, model):
    cal = [M.Calibration(f"c{i}", int(r[0]), r[2] if r[1] else None, r[3], r[5] if r[4] else None, r[6]) for i, r in enumerate(c["cal"])]
    con = [M.Constraint(f"k{i}", int(r[0]), int(r[1]), r[2]) for i, r in enumerate(c["con"])]
    ptr = c["brace_ptr"]
    br = [M.Brace(f"b{i}", [int(v) for v in c["brace_nodes"][ptr[i]:ptr[i + 1]]], float(s)) for i, s in enumerate(c["brace_sd"])]
    return M.PriorFunction(float(c["ht"]), PG.MODELS[model], cal, con, br, M.Topology(c["parent"]))


def state_of(pc):
    return M.StateBatch(pc["H"], pc["R"], pc["tH"], pc["rMu"], pc["birth"], pc["death"], pc["rVar"])


def position_reference(name, model, sparse, mask):
    """(value, its tolerance, gradient [B, dim], its tolerance) of ln [prior x likelihood x jacobianRootBranch] in position layout: prior
    reference + likelihood reference + Jacobian reference, the sum of their tolerances.  The value of the prior: the `close` rule of
    tests/test_gpu_prior_grad_exact.py (1e-11 x max(1, |ln prior|))."""
    pc, c = PRIOR[name], CASES["p_" + name]
    assert np.array_equal(pc["H"], c["H"]) and np.array_equal(pc["R"], c["R"]) and np.array_equal(pc["tH"], c["tH"]) and not np.any(pc["near"])
    pr, pt = PG.reference(pc, model), PG.tolerances(pc, model)
    lr, lt = TG.reference(c), tolerances("p_" + name, sparse)
    T = TG.Tables(c["parent"])
    B, nn = c["H"].shape
    rr = T.root_right

    def jac(src):
        jH, jR = np.zeros((B, nn)), np.zeros((B, nn))
        jH[:, 0], jH[:, 1], jH[:, rr], jR[:, 1], jR[:, rr] = (src[k] for k in ("jac_h0", "jac_hl", "jac_hr", "jac_rl", "jac_rr"))
        return jH, jR

    def full(p, l, j):
        jH, jR = jac(j)
        return np.concatenate([p["birth"][:, None], p["death"][:, None], (p["tH"] + l["gtH"] + j["jac_tH"])[:, None], p["H"] + l["gH"] + jH,
                               (p["rMu"] + l["grMu"] + j["jac_rMu"])[:, None], p["rVar"][:, None], p["R"] + l["gR"] + jR], axis=1)[:, mask][:, ::-1]

    lp = pc["lp"][:, model]
    return (lp + lr["ll"] + lr["logjac"], 1e-11 * np.maximum(1.0, np.abs(lp)) + lt["ll"] + lt["logjac"], full(pr, lr, lr), full(pt, lt, lt))


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("name", ["n3", "n65", "n257", "fx24"])
def test_target_in_position_layout(gpu, name, sparse):
    """Leapfrog(...).position(): value and gradient from k_hmc_collect and hmc_grad_entry for both masks (calibrations available or not),
    a dense and a sparse handle.  n257 has 388 positions: the 256-thread strides run twice."""
    pc = PRIOR[name]
    tl = handle("p_" + name, sparse)
    topo = tl.topo
    B = len(pc["tH"])
    for model in (0, 3):
        pf = prior_function(pc, model)
        for cal in (True, False):
            mask = M.get_mask(cal, topo)
            lf = M.Leapfrog(tl, pf, cal, B)
            lf.set_state(state_of(pc))
            q, v, g = lf.position()
            assert lf.dim == mask.sum() and (name != "n257" or lf.dim == 387 + cal)
            fold = np.concatenate([pc["birth"][:, None], pc["death"][:, None], pc["tH"][:, None], pc["H"], pc["rMu"][:, None], pc["rVar"][:, None],
                                   pc["R"]], axis=1)
            assert np.array_equal(q, fold[:, mask][:, ::-1])
            rv, tv, rg, tg = position_reference(name, model, sparse, mask)
            ev, eg = np.abs(v - rv), np.abs(g - rg)
            with np.errstate(divide="ignore", invalid="ignore"):
                wv, wg = np.where(ev == 0, 0.0, ev / tv), np.where(eg == 0, 0.0, eg / tg)
            wv, wg = np.where(np.isfinite(v), wv, np.inf), np.where(np.isfinite(g), wg, np.inf)
            at = np.unravel_index(np.argmax(wg), wg.shape)
            print(f"tree-grad-exact position {name} {'sparse' if sparse else 'dense'} model {model} cal {cal}: worst err/tol value {wv.max():.3g} "
                  f"gradient {wg[at]:.3g} at {tuple(int(i) for i in at)} (err {eg[at]:.3e}, tol {tg[at]:.3e}, reference {rg[at]:.17g})")
            assert wv.max() <= 1.0 and wg[at] <= 1.0, (name, sparse, model, cal, wv.max(), wg[at], at)


@pytest.mark.parametrize("sparse", [False, True])
def test_position_after_a_nuts_transition(gpu, sparse):
    """After one NUTS transition on n65 the handle's position, value and gradient are the bits a fresh set_state of the returned state
    gives."""
    pc = PRIOR["n65"]
    tl = handle("p_n65", sparse)
    B = len(pc["tH"])
    pf = prior_function(pc, 0)
    lf = M.Leapfrog(tl, pf, True, B)
    lf.set_state(state_of(pc))
    q0, _, g0 = lf.position()
    inv_mass = np.maximum((0.1 * np.abs(q0)).mean(axis=0) ** 2, 1e-12)
    eps = 1e-2 / np.maximum(1.0, (np.abs(g0) * np.sqrt(inv_mass)).max(axis=1))
    alpha, depth = lf.nuts(eps, inv_mass, max_depth=4, seed=65, transition=0)
    q1, v1, g1 = lf.position()
    assert depth.min() >= 1 and np.all(np.isfinite(v1)) and np.all(np.any(q1 != q0, axis=1)), (depth, alpha)
    fresh = M.Leapfrog(tl, pf, True, B)
    fresh.set_state(lf.state())
    q2, v2, g2 = fresh.position()
    assert np.array_equal(q1, q2) and np.array_equal(v1, v2) and np.array_equal(g1, g2)
