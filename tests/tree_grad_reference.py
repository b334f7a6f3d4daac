"""Reader of tests/golden/tree_grad_reference*.npz (written by tests/golden/make_tree_grad_reference.py): the gradient of the ln
likelihood with respect to the tree state at 50 digits, the matrices those files do not store, and the tolerance rule.  numpy only:
the tests that use it need neither mpmath nor an oracle.

The function (app/Probability.hs:195-207, 247-248, 393-410), per chain, for a tree of n_nodes nodes numbered in pre-order whose root
has the children l = 1 and rr (`root_right`), n = n_nodes - 2:
    t_v = h_parent(v) - h_v,   b_v = t_v r_v                          (heightTreeToLengthTree, x rates)
    x_0 = b_l + b_rr,  x_i = b_slot_node(i)                          (getBranches, sumFirstTwo)
    d = x tH rMu,  dx = d - mu,  y = 1/2 (P + P^T) dx,  g = -y
    ll = -n ln sqrt(2 pi) - 1/2 logdet - 1/2 dx . P dx,   logjac = -ln (tH rMu (b_l + b_rr))
    d ll / d r_v = s g_slot(v) t_v,  d ll / d h_v = sum_children e_c - e_v  (e_v = s g_slot(v) r_v, s = tH rMu, e_root = 0),
    d ll / d tH = g . d / tH,  d ll / d rMu = g . d / rMu.

Matrices.  A dense matrix of 1022^2 entries does not fit a committed file, so every matrix is rebuilt here from a formula: its entries
are small integers times a power of two, drawn by an integer recurrence (splitmix64 on a counter; no floating-point random numbers),
hence exactly representable and the same on every platform; each case stores the SHA-256 of P.tobytes(), which `matrix` asserts.
    family 0 ("a")  dense, every entry nonzero, symmetric, strictly diagonally dominant: off-diagonal +-m / 8, m = 1 .. 8
    family 1 ("b")  D K D with K of family 0 and D = diag(2^(k mod 12)): exact, 2^22 of dynamic range between the entries
    family 2 ("c")  sparse: a band of half-width 2 plus one scattered entry per row, symmetric, diagonally dominant; from n = 64 up a
                    row of exactly 17 entries (n // 5), one of 40 (n // 2: past the 16-wide record of ellT_*) and one of 16 (4 n // 5)
    family 3        the matrix of a committed fixture (tests/golden/<fixture>.npz: sigma_inv, mu), as it is

Tolerance of output component k (nothing in it knows a device result):   tol_k = 64 * m * 2^-53 * A_k
with A_k the component's formula with every addend replaced by its absolute value, propagated through the chain rule from
    A^g_i = sum_j (|W^T| |W|)_ij |dx_j|    dense handle: g goes through the factor W (lower triangular, W^T W = P; host_factor.cpp
                                           precision_factors: the Cholesky factor of P with rows and columns reversed, reversed back
                                           and transposed), recomputed here in fp64 -- it only scales a bound
    A^g_i = sum_j |P_ij| |dx_j|            sparse handle
    A_R_v = s A^g_slot(v) |t_v|,  A_H_v = sum_children s A^g_c |r_c| + s A^g_v |r_v|,  A_gd = sum_i A^g_i |d_i|,
    A_ll = n ln sqrt(2 pi) + 1/2 |logdet| + 1/2 sum_i |dx_i| A^g_i,  A_logjac = |logjac| + 1 (the logarithm's own rounding plus the
    relative error of its argument, whose condition number is 1)
and m = n for a dense handle (the convention of tests/test_gpu_parity.py:151 with A_k per component in the place of kappa x max);
for the sparse handle m = L, the longest row of the symmetric part, for gR and gH and m = n for ll, logjac, gtH and grMu.  The
derivatives of logjac (position-layout cases) have one addend each: 64 * 2^-53 * |value|."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {"small": "tree_grad_reference.npz", "large": "tree_grad_reference_large.npz", "sparse": "tree_grad_reference_sparse.npz",
         "sparse_large": "tree_grad_reference_sparse_large.npz", "position": "tree_grad_reference_position.npz"}
OUTPUTS = ["ll", "logjac", "gH", "gR", "gtH", "grMu"]
JAC = ["jac_h0", "jac_hl", "jac_hr", "jac_rl", "jac_rr", "jac_tH", "jac_rMu"]      # d logjac / d (h_root, h_l, h_rr, r_l, r_rr, tH, rMu)
SHARED = ["parent", "family", "seed", "logdet", "mu", "sha256", "fixture"]          # every other array: [chain, ...]
U = 2.0 ** -53
LN_SQRT_2PI = 0.9189385332046727417803297364056176
FIXTURES = ["24-leaves-braces"]                                                     # family 3: `seed` indexes this list


# ---------------------------------------------------------------------------------------------------------------------------------
# integer recurrence
# ---------------------------------------------------------------------------------------------------------------------------------
def mix(x):
    """splitmix64's output function on a uint64 array (wrapping arithmetic)."""
    x = np.atleast_1d(np.asarray(x, np.uint64)) + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def pair_hash(seed, i, j):
    """One uint64 per unordered index pair: the key (seed, min, max) mixed twice."""
    i, j = np.asarray(i, np.uint64), np.asarray(j, np.uint64)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    return mix(mix((np.uint64(seed) << np.uint64(24)) | (lo << np.uint64(12)) | hi))


def uniform(seed, count):
    """count numbers k / 2^53 in [0, 1), k from the recurrence: exact in fp64 (the generator draws the states from these)."""
    k = mix(mix(np.uint64(seed) * np.uint64(0x100000001B3) + np.arange(count, dtype=np.uint64)))
    return (k >> np.uint64(11)).astype(np.float64) / 2.0 ** 53


def _offdiag(seed, i, j):
    h = pair_hash(seed, i, j)
    m = (1 + (h & np.uint64(7)).astype(np.int64)).astype(np.float64) / 8.0
    return np.where((h >> np.uint64(3)) & np.uint64(1), -m, m)


def _close_diagonal(seed, K):
    n = len(K)
    k = np.arange(n)
    extra = 1.0 + (pair_hash(seed, k, k) & np.uint64(3)).astype(np.float64) / 4.0
    K[k, k] = np.abs(K).sum(axis=1) + extra                                        # multiples of 1/8 below 2^53: exact in any order
    return K


def dense_k(n, seed):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    K = _offdiag(seed, i, j).reshape(n, n)
    K[np.arange(n), np.arange(n)] = 0.0
    return _close_diagonal(seed, K)


SPECIAL_ROWS = ((5, 1, 17), (2, 1, 40), (5, 4, 16))                                 # (row = num n // den, entries with the diagonal)


def special_rows(n):
    return [(num * n // den, target) for den, num, target in SPECIAL_ROWS] if n >= 64 else []


def sparse_p(n, seed):
    pairs = set()
    for i in range(n):
        for d in (1, 2):
            if i + d < n:
                pairs.add((i, i + d))
    far = (mix(mix((np.uint64(seed) << np.uint64(24)) + np.arange(n, dtype=np.uint64))) % np.uint64(max(n, 1))).astype(np.int64)
    for i in range(n):
        j = int(far[i])
        if abs(i - j) > 2:
            pairs.add((min(i, j), max(i, j)))
    special = special_rows(n)
    rows = {r for r, _ in special}
    for r, target in special:
        count = 1 + sum(1 for p in pairs if r in p)
        assert count <= target, (n, r, count)
        k = 0
        while count < target:
            j = (r + 7 + 5 * k) % n
            k += 1
            p = (min(r, j), max(r, j))
            if j in rows or p in pairs:
                continue
            pairs.add(p)
            count += 1
    P = np.zeros((n, n))
    if pairs:
        ii, jj = (np.array(x) for x in zip(*sorted(pairs)))
        v = _offdiag(seed, ii, jj)
        P[ii, jj] = v
        P[jj, ii] = v
    P = _close_diagonal(seed, P)
    for r, target in special:
        assert np.count_nonzero(P[r]) == target
    return P


_matrices = {}


def matrix(case):
    """(P [n, n], mu [n]) of a case, rebuilt from its formula (or read from its fixture) and checked against the stored hash."""
    family, seed, n = int(case["family"]), int(case["seed"]), len(case["parent"]) - 2
    key = (family, seed, n)
    if key not in _matrices:
        if family == 0:
            P = dense_k(n, seed)
        elif family == 1:
            D = 2.0 ** (np.arange(n) % 12)
            P = dense_k(n, seed) * D[:, None] * D[None, :]
        elif family == 2:
            P = sparse_p(n, seed)
        else:
            with np.load(os.path.join(GOLDEN, FIXTURES[seed] + ".npz")) as fx:
                P = np.array(fx["sigma_inv"], np.float64)
        P = np.ascontiguousarray(P)
        assert P.shape == (n, n)
        digest = hashlib.sha256(P.tobytes()).hexdigest()
        assert digest == str(case["sha256"]), (key, digest)
        _matrices[key] = P
    return _matrices[key], np.asarray(case["mu"], np.float64)


def is_sparse(case):
    return int(case["family"]) == 2


def assoc_of(P):
    """The association list [((i, j), value)] of the nonzero entries, row by row."""
    ii, jj = np.nonzero(P)
    return [((int(i), int(j)), float(P[i, j])) for i, j in zip(ii, jj)]


def factor(P):
    """W lower triangular with W^T W = 1/2 (P + P^T), as host_factor.cpp's precision_factors arranges it, in numpy fp64."""
    A = 0.5 * (P + P.T)
    C = np.linalg.cholesky(A[::-1, ::-1])
    return np.ascontiguousarray(C.T[::-1, ::-1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the tree's tables, as mcd_tree_create builds them
# ---------------------------------------------------------------------------------------------------------------------------------
class Tables:
    def __init__(self, parent):
        parent = np.asarray(parent, np.int64)
        nn = len(parent)
        roots = np.flatnonzero(parent == 0)
        assert len(roots) == 2 and roots[0] == 1
        self.parent, self.n_nodes, self.root_right = parent, nn, int(roots[1])
        self.slot_node = np.array([1] + [v for v in range(2, nn) if v != self.root_right], np.int64)     # getBranches, sumFirstTwo
        self.slot_parent = parent[self.slot_node]
        self.slot = np.full(nn, -1, np.int64)
        self.slot[self.slot_node] = np.arange(nn - 2)
        self.slot[self.root_right] = 0
        self.children = [[] for _ in range(nn)]
        for v in range(1, nn):
            self.children[int(parent[v])].append(v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the route in plain fp64, and what the host test does to it
# ---------------------------------------------------------------------------------------------------------------------------------
def distances(T, H, R, tH, rMu, slot_parent=None):
    """d [B, n] of the states; slot_parent replaces the table's (a mutation of the host test)."""
    sp = T.slot_parent if slot_parent is None else slot_parent
    rr = T.root_right
    x = (H[:, sp] - H[:, T.slot_node]) * R[:, T.slot_node]
    x[:, 0] = x[:, 0] + (H[:, 0] - H[:, rr]) * R[:, rr]
    return x * (tH * rMu)[:, None]


def numpy_fp64(case, sparse=None, mutation=None):
    """name -> array of OUTPUTS, the same route in plain fp64: y = W^T (W dx) for a dense handle, P dx for the sparse one.
    mutation: one of the defects of tests/test_tree_grad_reference_host.py, or None; a mutation that does not apply to the case
    returns None."""
    sparse = is_sparse(case) if sparse is None else sparse
    P, mu = matrix(case)
    T = Tables(case["parent"])
    H, R, tH, rMu = (np.asarray(case[k], np.float64) for k in ("H", "R", "tH", "rMu"))
    B, nn = H.shape
    n, rr = nn - 2, T.root_right
    kids = [list(c) for c in T.children]
    slot_parent = None
    if mutation == "drop_last_child_of_3":
        wide = [v for v in range(1, nn) if len(kids[v]) >= 3]
        if not wide:
            return None
        for v in wide:
            kids[v].pop()
    elif mutation == "drop_only_child":
        single = [v for v in range(1, nn) if len(kids[v]) == 1]
        if not single:
            return None
        for v in single:
            kids[v].pop()
    elif mutation == "neighbour_slot_parent":
        slot_parent = np.roll(T.slot_parent, -1)
        if np.array_equal(slot_parent, T.slot_parent):
            return None
    elif mutation == "omit_17th_entry":
        rows = [r for r, target in special_rows(n) if target > 16] if is_sparse(case) else []
        if not rows:
            return None
        P = P.copy()
        for r in rows:
            P[r, np.flatnonzero(P[r])[16]] = 0.0                                   # (the row alone: the record that is 16 wide is the row's)
    elif mutation == "scale_component_of_b" and int(case["family"]) != 1:
        return None
    s = tH * rMu
    d = distances(T, H, R, tH, rMu, slot_parent)
    dx = d - mu
    if sparse:
        y = dx @ (0.5 * (P + P.T)).T
        q = np.einsum("bi,bi->b", dx, dx @ P.T)
    else:
        W = factor(P)
        z = dx @ W.T
        y = z @ W
        q = np.einsum("bi,bi->b", z, z)
    g = -y
    if mutation == "scale_component_of_b":
        quiet = np.arange(0, n, 12)                                                 # D_i = 1: the components a max-norm bound does not see
        Ag = abs_g(case, sparse)
        i = quiet[np.argmax(np.abs(g[0, quiet]) / Ag[0, quiet])]                    # (the least cancelled of them in chain 0)
        g = g.copy()
        g[:, i] *= 1.0 + 1e-9
    out = {"ll": -LN_SQRT_2PI * n - 0.5 * float(case["logdet"]) - 0.5 * q}
    bl, br = (H[:, 0] - H[:, 1]) * R[:, 1], (H[:, 0] - H[:, rr]) * R[:, rr]
    out["logjac"] = -np.log(s * (bl + br))
    t = H[:, np.maximum(T.parent, 0)] - H
    gs = np.zeros((B, nn))
    gs[:, 1:] = g[:, T.slot[1:]]                                                    # g of every node's slot
    gR = s[:, None] * gs * t
    if mutation == "exchange_root_children":
        if np.array_equal(t[:, 1], t[:, rr]):                                       # (both root children leaves: the same branch)
            return None
        gR[:, [1, rr]] = np.stack([s * gs[:, 1] * t[:, rr], s * gs[:, rr] * t[:, 1]], axis=1)
    gR[:, 0] = 0.0
    e = s[:, None] * gs * R
    e[:, 0] = 0.0
    gH = -e
    for v in range(nn):
        for c in kids[v]:
            gH[:, v] += e[:, c]
    dn = (t * R * s[:, None])                                                       # every node's own share of the distances
    gd = np.einsum("bv,bv->b", gs[:, 1:], dn[:, 1:])
    if mutation == "root_right_out_of_gd":
        gd = gd - gs[:, rr] * dn[:, rr]
    out.update(gH=gH, gR=gR, gtH=gd / tH, grMu=gd / rMu)
    return out


def abs_g(case, sparse=None):
    """A^g [B, n] of the rule above, from the stored inputs in fp64."""
    sparse = is_sparse(case) if sparse is None else sparse
    P, mu = matrix(case)
    T = Tables(case["parent"])
    H, R, tH, rMu = (np.asarray(case[k], np.float64) for k in ("H", "R", "tH", "rMu"))
    adx = np.abs(distances(T, H, R, tH, rMu) - mu)
    if sparse:
        return adx @ np.abs(0.5 * (P + P.T)).T
    W = np.abs(factor(P))
    return (adx @ W.T) @ W


def longest_row(P):
    return int(np.count_nonzero(0.5 * (P + P.T), axis=1).max())


def tolerances(case, sparse=None):
    """name -> tolerance array of OUTPUTS (and of JAC where the case stores them), shaped like `reference`."""
    sparse = is_sparse(case) if sparse is None else sparse
    P, mu = matrix(case)
    T = Tables(case["parent"])
    H, R, tH, rMu = (np.asarray(case[k], np.float64) for k in ("H", "R", "tH", "rMu"))
    B, nn = H.shape
    n = nn - 2
    s = tH * rMu
    d = distances(T, H, R, tH, rMu)
    Ag = abs_g(case, sparse)
    As = np.zeros((B, nn))
    As[:, 1:] = Ag[:, T.slot[1:]]
    t = np.abs(H[:, np.maximum(T.parent, 0)] - H)
    AR = s[:, None] * As * t
    AR[:, 0] = 0.0
    Ae = s[:, None] * As * np.abs(R)
    Ae[:, 0] = 0.0
    AH = Ae.copy()
    for v in range(nn):
        for c in T.children[v]:
            AH[:, v] += Ae[:, c]
    Agd = np.einsum("bi,bi->b", Ag, np.abs(d))
    A = {"ll": LN_SQRT_2PI * n + 0.5 * abs(float(case["logdet"])) + 0.5 * np.einsum("bi,bi->b", np.abs(d - mu), Ag),
         "logjac": np.abs(np.asarray(case["logjac"])) + 1.0, "gH": AH, "gR": AR, "gtH": Agd / np.abs(tH), "grMu": Agd / np.abs(rMu)}
    rows = longest_row(P) if sparse else n
    tol = {k: 64 * (rows if k in ("gH", "gR") else n) * U * A[k] for k in OUTPUTS}
    for k in JAC:
        if k in case:
            tol[k] = 64 * U * np.abs(np.asarray(case[k]))
    return tol


def reference(case):
    """name -> 50-digit value rounded to fp64 of OUTPUTS (and JAC where stored): [B] or [B, n_nodes]."""
    return {k: np.asarray(case[k]) for k in OUTPUTS + JAC if k in case}


def load(which):
    """{case name: {array name: array}} of one of the files."""
    out = {}
    with np.load(os.path.join(GOLDEN, FILES[which])) as z:
        for key in z.files:
            name, arr = key.split("/", 1)
            out.setdefault(name, {})[arr] = z[key]
    return out


def load_all(which=None):
    out = {}
    for w in (FILES if which is None else which):
        out.update(load(w))
    return out
