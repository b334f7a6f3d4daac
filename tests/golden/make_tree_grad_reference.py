#!/usr/bin/env python3
"""Build tests/golden/tree_grad_reference*.npz: ln likelihood, ln jacobianRootBranch and their gradient with respect to the tree
state at 50 digits (mp.dps = 50), from the fp64 inputs taken as exact.  tests/tree_grad_reference.py (the reader) states the
function, rebuilds the matrices and carries the tolerance rule; this file makes the trees, the states and the reference values.

Two independent differentiations, which must agree to 1e-35 relative or the generator aborts:
  (a) the closed chain rule: g = -1/2 (P + P^T) dx, d ll / d r_v = s g t_v, d ll / d h_v = sum_children e_c - e_v, g . d / tH,
      g . d / rMu, the second root branch folded into slot 0;
  (b) forward mode: a dual number over mpf with a sparse tangent (one entry per state coordinate it depends on) carried through
      state -> branches -> distances -> dx -> P dx (P as given, not symmetrised) -> ll, and through ln jacobianRootBranch.
On trees of at most 25 nodes the whole function is also differentiated coordinate by coordinate with mpmath.diff.

Trees (integer recurrence of the reader, no floating-point random numbers; `build_tree`): random binary trees, caterpillars, the
root's left or right child a leaf, inner nodes with 3 and with 5 children, inner nodes with one child -- each below 64 nodes and
above 256 -- and the trees of 257 and 258 nodes whose last nodes are the third child of an inner node (node 256), which in the larger
tree has one child itself (node 257).  States: valid height trees (h_v = (depth of v's subtree + u_v) / (depth of the tree + 1)),
rates, tH and rMu around 1; chain 1 has tH = 1.  mu: the distances of the state with every u_v = 1/2 and unit rates, times
0.5 .. 1.5 per component, so that dx is of the size of d; on trees of at most 9 nodes, where a component of g has few addends and
a dx that happens to cancel would leave the rounding of d alone in it, times 0.25 .. 0.5.

Files (each below 512 KiB): dense cases up to 259 nodes, dense cases above, sparse cases up to 259 nodes, sparse cases above, and the
cases of the position layout: the states tests/golden/prior_grad_reference.npz holds for n3, n65, n257 (a family 0 matrix) and
fx24 (the fixture's own matrix), with the seven derivatives of ln jacobianRootBranch.

Run:  python tests/golden/make_tree_grad_reference.py [--check]     (--check: regenerate and compare with the committed files)
"""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tree_grad_reference as TG  # noqa: E402  (tests/tree_grad_reference.py: the reader)

from mpmath import mp, mpf  # noqa: E402

DIGITS = 50
MAX_FILE = 512 * 1024


# ---------------------------------------------------------------------------------------------------------------------------------
# trees
# ---------------------------------------------------------------------------------------------------------------------------------
def build_tree(n_nodes, kind, seed, extras=()):
    """Parent array in pre-order.  kind: "random", "caterpillar" (right spine: the root's left child is a leaf), "caterpillar_left"
    (left spine: the root's right child is a leaf), "left_leaf", "right_leaf" (random below the root's other child).  extras, applied
    in order to the binary tree: ("multi", k) gives a bifurcating inner node k children, ("single",) gives a leaf one child;
    a third element "tail" takes the parent of the last node in pre-order (multi) or the last node itself (single)."""
    extra_nodes = sum(e[1] - 2 if e[0] == "multi" else 1 for e in extras)
    base = n_nodes - extra_nodes
    assert base >= 3 and base % 2 == 1, (n_nodes, extras)
    kids = {0: [1, 2], 1: [], 2: []}
    par = {1: 0, 2: 0}
    draws = iter(TG.mix(TG.mix(np.uint64(seed) * np.uint64(1000003) + np.arange(4 * n_nodes + 16, dtype=np.uint64))).tolist())
    protected = {"left_leaf": {1}, "caterpillar": {1}, "right_leaf": {2}, "caterpillar_left": {2}}.get(kind, set())

    def add_child(v):
        c = len(kids)
        kids[c] = []
        kids[v].append(c)
        par[c] = v
        return c

    spine = 2 if kind == "caterpillar" else 1
    while len(kids) < base:
        if kind.startswith("caterpillar"):
            v = spine
        else:
            leaves = [v for v in kids if v and not kids[v] and v not in protected]
            v = leaves[next(draws) % len(leaves)]
        a, b = add_child(v), add_child(v)
        spine = b if kind == "caterpillar" else a

    def last_node():
        v = 0
        while kids[v]:
            v = kids[v][-1]
        return v

    pinned = set()
    for e in extras:
        tail = e[-1] == "tail"
        if e[0] == "multi":
            if tail:
                v = par[last_node()]
            else:
                cand = [v for v in kids if v and len(kids[v]) == 2 and v not in pinned]
                v = cand[next(draws) % len(cand)]
            assert v != 0 and len(kids[v]) == 2
            for _ in range(e[1] - 2):
                add_child(v)
            pinned |= {v} | set(kids[v])
        else:
            if tail:
                v = last_node()
            else:
                cand = [v for v in kids if v and not kids[v] and v not in protected and v not in pinned]
                v = cand[next(draws) % len(cand)]
            pinned |= {v, add_child(v)}
    parent = []

    def number(v, p):
        stack = [(v, p)]
        while stack:
            v, p = stack.pop()
            me = len(parent)
            parent.append(p)
            for c in reversed(kids[v]):
                stack.append((c, me))

    number(0, -1)
    parent = np.asarray(parent, np.int32)
    assert len(parent) == n_nodes and np.all(parent[1:] < np.arange(1, n_nodes))
    return parent


def children_of(parent):
    kids = [[] for _ in parent]
    for v in range(1, len(parent)):
        kids[int(parent[v])].append(v)
    return kids


def features(parent):
    kids = children_of(parent)
    nn = len(parent)
    rr = kids[0][1]
    deg = [len(k) for k in kids]
    return dict(root_right=rr, left_leaf=deg[1] == 0, right_leaf=deg[rr] == 0, three=3 in deg[1:], five=5 in deg[1:], single=1 in deg[1:],
                binary=all(d in (0, 2) for d in deg), caterpillar=all(d in (0, 2) for d in deg) and sum(1 for d in deg if d) == (nn - 1) // 2
                and max(sum(1 for c in k if kids[c]) for k in kids) <= 1)


# name -> (n_nodes, family of the matrix, tree kind, extras)
M3, M5, S1 = ("multi", 3), ("multi", 5), ("single",)
DENSE = {
    "d1": (3, 0, "random", ()),
    "d5bin": (7, 0, "random", ()),
    "d5cat": (7, 1, "caterpillar_left", ()),
    "d5mix": (7, 1, "left_leaf", (S1, M3)),
    "d20": (22, 1, "random", (M5, M3, S1)),
    "d63": (65, 0, "random", ()),
    "d64": (66, 1, "random", (M5, M3, S1)),
    "d65": (67, 0, "caterpillar", ()),
    "d129": (131, 1, "right_leaf", ()),
    "d200": (202, 0, "left_leaf", (S1,)),
    "d255": (257, 1, "random", (M3 + ("tail",), S1)),
    "d256": (258, 0, "random", (M3 + ("tail",), S1 + ("tail",), M3)),
    "d257": (259, 1, "random", ()),
    "d390": (392, 0, "caterpillar_left", (M5,)),
    "d513": (515, 1, "right_leaf", (M3, S1)),
    "d769": (771, 0, "left_leaf", (M5, S1)),
    "d1022": (1024, 1, "random", (M3, S1, M3)),
}
SPARSE = {
    "s1": (3, 2, "random", ()),
    "s20": (22, 2, "left_leaf", (M5, M3, S1)),
    "s255": (257, 2, "random", (M3 + ("tail",), S1)),
    "s256": (258, 2, "random", (M3 + ("tail",), S1 + ("tail",), M3)),
    "s257": (259, 2, "caterpillar", ()),
    "s1022": (1024, 2, "right_leaf", (M3, S1, M3)),
    "s2046": (2048, 2, "random", (M5, S1, M3)),
}


def file_of(name, n_nodes):
    if name.startswith("p_"):
        return "position"
    big = n_nodes > 259
    return ("sparse_large" if big else "sparse") if name.startswith("s") else ("large" if big else "small")


# ---------------------------------------------------------------------------------------------------------------------------------
# states
# ---------------------------------------------------------------------------------------------------------------------------------
def subtree_depth(parent):
    kids = children_of(parent)
    depth = np.zeros(len(parent), int)
    for v in range(len(parent) - 1, -1, -1):
        if kids[v]:
            depth[v] = 1 + max(depth[c] for c in kids[v])
    return depth, kids


def make_states(parent, batch, seed):
    nn = len(parent)
    depth, kids = subtree_depth(parent)
    inner = np.array([bool(k) for k in kids])
    u = TG.uniform(seed, batch * (2 * nn + 2)).reshape(batch, 2 * nn + 2)
    H = np.where(inner[None, :], (depth[None, :] + 0.05 + 0.9 * u[:, :nn]) / (depth[0] + 1.0), 0.0)
    H[:, 0] = 1.0
    R = 0.6 + 0.8 * u[:, nn:2 * nn]
    tH, rMu = 0.8 + 0.4 * u[:, 2 * nn], 0.8 + 0.4 * u[:, 2 * nn + 1]
    if batch > 1:
        tH[1] = 1.0
    assert np.all(H[:, parent[1:]] > H[:, 1:])
    return dict(H=H, R=R, tH=tH, rMu=rMu)


def make_mu(parent, seed):
    nn = len(parent)
    depth, kids = subtree_depth(parent)
    inner = np.array([bool(k) for k in kids])
    H = np.where(inner, (depth + 0.5) / (depth[0] + 1.0), 0.0)[None, :]
    H[:, 0] = 1.0
    d0 = TG.distances(TG.Tables(parent), H, np.ones((1, nn)), np.ones(1), np.ones(1))[0]
    u = TG.uniform(seed + 77, nn - 2)
    return d0 * (0.25 + 0.25 * u if nn <= 9 else 0.5 + u)


def build_cases(only=None):
    cases = {}
    for k, (name, (nn, family, kind, extras)) in enumerate(list(DENSE.items()) + list(SPARSE.items())):
        if only is not None and name not in only:
            continue
        seed = 100 + k
        parent = build_tree(nn, kind, seed, extras)
        c = dict(parent=parent, family=np.int32(family), seed=np.int32(seed), logdet=np.float64(3.25), mu=make_mu(parent, seed),
                 fixture=np.str_(""), **make_states(parent, 6 if nn <= 257 else 4, seed))
        cases[name] = c
    import prior_grad_reference as PG
    prior = PG.load("main")
    for k, name in enumerate(("n3", "n65", "n257", "fx24")):
        if only is not None and "p_" + name not in only:
            continue
        pc = prior[name]
        parent = np.asarray(pc["parent"], np.int32)
        c = dict(parent=parent, H=np.array(pc["H"], float), R=np.array(pc["R"], float), tH=np.array(pc["tH"], float), rMu=np.array(pc["rMu"], float))
        if name == "fx24":
            fx = np.load(os.path.join(HERE, TG.FIXTURES[0] + ".npz"))
            c.update(family=np.int32(3), seed=np.int32(0), logdet=np.float64(fx["logdet"]), mu=np.array(fx["mu"], float), fixture=np.str_(TG.FIXTURES[0]))
        else:
            c.update(family=np.int32(0), seed=np.int32(200 + k), logdet=np.float64(3.25), mu=make_mu(parent, 200 + k), fixture=np.str_(""))
        cases["p_" + name] = c
    for name, c in cases.items():
        c["sha256"] = np.str_(hashlib.sha256(raw_matrix(c).tobytes()).hexdigest())
    return cases


def raw_matrix(c):
    """The matrix by the reader's formulas, before there is a hash to check."""
    family, seed, n = int(c["family"]), int(c["seed"]), len(c["parent"]) - 2
    if family == 3:
        with np.load(os.path.join(HERE, TG.FIXTURES[seed] + ".npz")) as fx:
            return np.ascontiguousarray(np.array(fx["sigma_inv"], np.float64))
    if family == 2:
        return np.ascontiguousarray(TG.sparse_p(n, seed))
    K = TG.dense_k(n, seed)
    if family == 1:
        D = 2.0 ** (np.arange(n) % 12)
        K = K * D[:, None] * D[None, :]
    return np.ascontiguousarray(K)


# ---------------------------------------------------------------------------------------------------------------------------------
# forward mode over mpf, sparse tangents
# ---------------------------------------------------------------------------------------------------------------------------------
class Dual:
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = v, d

    def __add__(self, o):
        if not isinstance(o, Dual):
            return Dual(self.v + o, self.d)
        d = dict(self.d)
        for k, x in o.d.items():
            d[k] = d[k] + x if k in d else x
        return Dual(self.v + o.v, d)

    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.v, {k: -x for k, x in self.d.items()})

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, Dual):
            return Dual(self.v * o, {k: x * o for k, x in self.d.items()})
        d = {k: x * o.v for k, x in self.d.items()}
        for k, x in o.d.items():
            d[k] = d[k] + self.v * x if k in d else self.v * x
        return Dual(self.v * o.v, d)

    __rmul__ = __mul__


def d_log(x):
    if isinstance(x, Dual):
        return Dual(mp.log(x.v), {k: a / x.v for k, a in x.d.items()})
    return mp.log(x)


def state_to_values(T, H, R, tH, rMu, P_rows, mu, logdet, lin):
    """(ll, logjac) of one state in whatever number type H, R, tH, rMu carry.  lin(row, xs): sum_j row[j] xs[j] (row: fp64 entries)."""
    n = T.n_nodes - 2
    rr = T.root_right
    s = tH * rMu
    b = lambda v: (H[int(T.parent[v])] - H[v]) * R[v]
    root = b(1) + b(rr)
    x = [root] + [b(int(v)) for v in T.slot_node[1:]]
    dx = [xi * s - mpf(m) for xi, m in zip(x, mu)]
    q = mpf(0)
    for i in range(n):
        q = q + dx[i] * lin(P_rows[i], dx)                   # y_i is folded into the sum at once (a row's tangent is long)
    ll = q * mpf(-0.5) + (-mpf(n) * mp.log(mp.sqrt(2 * mp.pi)) - mpf(logdet) / 2)
    return ll, -d_log(s * root)


def lin_plain(row, xs):
    cols, vals = row
    return mp.fdot(vals, [xs[j] for j in cols])


def lin_dual(row, xs):
    cols, vals = row
    v = mpf(0)
    acc = {}
    for j, p in zip(cols, vals):
        xj = xs[j]
        v += p * xj.v
        for k, a in xj.d.items():
            acc[k] = acc[k] + p * a if k in acc else p * a
    return Dual(v, acc)


def sparse_rows(P):
    """Every row as (columns, mpf values) of its nonzero entries."""
    out = []
    for i in range(len(P)):
        cols = np.flatnonzero(P[i])
        out.append(([int(j) for j in cols], [mpf(float(P[i, j])) for j in cols]))
    return out


def agree(a, b, what):
    scale = max(abs(a), abs(b))
    if abs(a - b) > mpf(10) ** -35 * scale + mpf(10) ** -60:
        raise SystemExit(f"differentiations disagree: {what}: {mp.nstr(a, 45)} vs {mp.nstr(b, 45)}")


_rows = {}


def chain_reference(args):
    """Everything stored for one chain: name -> float / array."""
    name, c, bidx = args
    mp.dps = DIGITS
    P = raw_matrix(c)
    key = (int(c["family"]), int(c["seed"]), len(P))
    if key not in _rows:
        _rows.clear()
        _rows[key] = (sparse_rows(P), sparse_rows(np.ascontiguousarray(P.T)))
    rows, rows_t = _rows[key]
    T = TG.Tables(c["parent"])
    nn, n, rr = T.n_nodes, T.n_nodes - 2, T.root_right
    H = [mpf(float(x)) for x in c["H"][bidx]]
    R = [mpf(float(x)) for x in c["R"][bidx]]
    tH, rMu = mpf(float(c["tH"][bidx])), mpf(float(c["rMu"][bidx]))
    mu, logdet = [float(x) for x in c["mu"]], float(c["logdet"])
    # (a) the closed chain rule
    s = tH * rMu
    t = [mpf(0)] + [H[int(T.parent[v])] - H[v] for v in range(1, nn)]
    bn = [t[v] * R[v] for v in range(nn)]
    x = [bn[1] + bn[rr]] + [bn[int(v)] for v in T.slot_node[1:]]
    d = [xi * s for xi in x]
    dx = [di - mpf(m) for di, m in zip(d, mu)]
    Pdx = [lin_plain(rows[i], dx) for i in range(n)]
    Ptdx = Pdx if np.array_equal(P, P.T) else [lin_plain(rows_t[i], dx) for i in range(n)]
    g = [-(a + b) / 2 for a, b in zip(Pdx, Ptdx)]
    ll = -mpf(n) * mp.log(mp.sqrt(2 * mp.pi)) - mpf(logdet) / 2 - mp.fdot(dx, Pdx) / 2
    root = bn[1] + bn[rr]
    logjac = -mp.log(s * root)
    gs = [mpf(0)] + [g[int(T.slot[v])] for v in range(1, nn)]
    gR = [s * gs[v] * t[v] for v in range(nn)]
    e = [s * gs[v] * R[v] for v in range(nn)]
    gH = [sum((e[ch] for ch in T.children[v]), mpf(0)) - e[v] for v in range(nn)]
    gd = mp.fdot(g, d)
    out = dict(ll=ll, logjac=logjac, gH=gH, gR=gR, gtH=gd / tH, grMu=gd / rMu)
    jac = dict(jac_h0=-(R[1] + R[rr]) / root, jac_hl=R[1] / root, jac_hr=R[rr] / root, jac_rl=-t[1] / root, jac_rr=-t[rr] / root,
               jac_tH=-1 / tH, jac_rMu=-1 / rMu)
    # (b) forward mode: coordinates H_v -> v, R_v -> nn + v, tH -> 2 nn, rMu -> 2 nn + 1
    one = mpf(1)
    Hd = [Dual(h, {v: one}) for v, h in enumerate(H)]
    Rd = [Dual(r, {nn + v: one}) for v, r in enumerate(R)]
    ll_d, lj_d = state_to_values(T, Hd, Rd, Dual(tH, {2 * nn: one}), Dual(rMu, {2 * nn + 1: one}), rows, mu, logdet, lin_dual)
    agree(ll_d.v, ll, f"{name} chain {bidx} ll")
    agree(lj_d.v, logjac, f"{name} chain {bidx} logjac")
    zero = mpf(0)
    for v in range(nn):
        agree(ll_d.d.get(v, zero), gH[v], f"{name} chain {bidx} gH[{v}]")
        agree(ll_d.d.get(nn + v, zero), gR[v], f"{name} chain {bidx} gR[{v}]")
    agree(ll_d.d[2 * nn], out["gtH"], f"{name} chain {bidx} gtH")
    agree(ll_d.d[2 * nn + 1], out["grMu"], f"{name} chain {bidx} grMu")
    for k, coord in (("jac_h0", 0), ("jac_hl", 1), ("jac_hr", rr), ("jac_rl", nn + 1), ("jac_rr", nn + rr), ("jac_tH", 2 * nn), ("jac_rMu", 2 * nn + 1)):
        agree(lj_d.d[coord], jac[k], f"{name} chain {bidx} {k}")
    assert set(lj_d.d) == {0, 1, rr, nn + 1, nn + rr, 2 * nn, 2 * nn + 1}
    # (c) small trees: the whole function, coordinate by coordinate
    if nn <= 25:
        x0 = H + R + [tH, rMu]
        flat = gH + gR + [out["gtH"], out["grMu"]]
        jflat = {0: jac["jac_h0"], 1: jac["jac_hl"], rr: jac["jac_hr"], nn + 1: jac["jac_rl"], nn + rr: jac["jac_rr"], 2 * nn: jac["jac_tH"],
                 2 * nn + 1: jac["jac_rMu"]}

        def at(i, z, w):
            xs = x0[:i] + [z] + x0[i + 1:]
            return state_to_values(T, xs[:nn], xs[nn:2 * nn], xs[2 * nn], xs[2 * nn + 1], rows, mu, logdet, lin_plain)[w]

        for i in range(len(x0)):
            for w, want in ((0, flat[i]), (1, jflat.get(i, zero))):
                got = mp.diff(lambda z: at(i, z, w), x0[i])
                if abs(got - want) > mpf(10) ** -35 * max(abs(got), abs(want)) + mpf(10) ** -40:
                    raise SystemExit(f"{name} chain {bidx}: mpmath.diff disagrees at coordinate {i} of output {w}: {mp.nstr(got, 40)} vs {mp.nstr(want, 40)}")
    res = {k: (np.array([float(a) for a in v]) if isinstance(v, list) else float(v)) for k, v in out.items()}
    if name.startswith("p_"):
        res.update({k: float(v) for k, v in jac.items()})
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------------------------------
INPUTS = ["parent", "family", "seed", "logdet", "mu", "sha256", "fixture", "H", "R", "tH", "rMu"]


def savez_bytes(arrays):
    """np.savez_compressed into memory with fixed time stamps, so that the same arrays give the same file."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), a.getvalue(), zipfile.ZIP_DEFLATED)
    return buf.getvalue()


def generate(only=None, pool=None):
    """{case: arrays}; only = {case name: [chain indices]} restricts the work (the host test's stale-fixture check)."""
    cases = build_cases(None if only is None else set(only))
    jobs = [(name, b) for name, c in cases.items() for b in range(len(c["tH"])) if only is None or b in only[name]]
    jobs.sort(key=lambda j: -len(cases[j[0]]["parent"]))                            # the long ones first
    run = (lambda f, a: pool.imap(f, a, chunksize=1)) if pool is not None else map
    res = dict(zip(jobs, run(chain_reference, [(name, cases[name], b) for name, b in jobs])))
    out = {}
    for name, c in cases.items():
        idx = [b for b in range(len(c["tH"])) if (name, b) in res]
        arrays = {k: (np.asarray(c[k]) if k in TG.SHARED else np.asarray(c[k])[idx]) for k in INPUTS}
        chains = [res[(name, b)] for b in idx]
        for k in chains[0]:
            arrays[k] = np.array([ch[k] for ch in chains])
        out[name] = arrays
    return out


def check_features(cases):
    """What the trees are there for."""
    f = {name: features(c["parent"]) for name, c in cases.items()}
    small = [n for n, c in cases.items() if len(c["parent"]) < 64]
    large = [n for n, c in cases.items() if len(c["parent"]) > 256]
    for group in (small, large):
        for key in ("binary", "caterpillar", "left_leaf", "right_leaf", "three", "five", "single"):
            assert any(f[n][key] for n in group), (key, group)
    assert any(f[n]["root_right"] == 2 for n in cases) and any(f[n]["root_right"] == len(cases[n]["parent"]) - 1 for n in cases)
    for name in ("d255", "s255"):
        p = cases[name]["parent"]
        assert len(p) == 257 and int(np.sum(p == p[256])) == 3
    for name in ("d256", "s256"):
        p = cases[name]["parent"]
        assert len(p) == 258 and p[257] == 256 and int(np.sum(p == p[256])) == 3 and int(np.sum(p == 256)) == 1
    for name, c in cases.items():
        if int(c["family"]) == 2 and len(c["parent"]) - 2 >= 64:
            P = TG.matrix(c)[0]
            counts = np.count_nonzero(P, axis=1)
            assert {16, 17, 40} <= set(counts.tolist()) and counts.max() == 40 and np.array_equal(P, P.T)
        if int(c["family"]) < 3:
            P = TG.matrix(c)[0]
            off = np.abs(P).sum(axis=1) - np.abs(np.diag(P))
            if int(c["family"]) == 1:
                D = 2.0 ** (np.arange(len(P)) % 12)
                K = P / D[:, None] / D[None, :]
                off = np.abs(K).sum(axis=1) - np.abs(np.diag(K))
                assert np.all(np.diag(K) > off)
            else:
                assert np.all(np.diag(P) > off)
            if int(c["family"]) < 2:
                assert np.all(P != 0)


def main():
    import multiprocessing as mpc

    check_only = "--check" in sys.argv
    with mpc.get_context("fork").Pool(min(16, os.cpu_count() or 1)) as pool:
        cases = generate(pool=pool)
    check_features(cases)
    for which, fname in TG.FILES.items():
        mine = {name: c for name, c in cases.items() if file_of(name, len(c["parent"])) == which}
        blob = savez_bytes({f"{name}/{k}": v for name, c in mine.items() for k, v in c.items()})
        print(f"{fname}: {sorted(mine)}: {len(blob)} bytes")
        if len(blob) > MAX_FILE:
            raise SystemExit(f"{fname} is larger than {MAX_FILE} bytes")
        path = os.path.join(HERE, fname)
        if check_only:
            if open(path, "rb").read() != blob:
                raise SystemExit(f"{fname} differs from the committed file")
            print("  identical to the committed file")
        else:
            with open(path, "wb") as f:
                f.write(blob)


if __name__ == "__main__":
    main()
