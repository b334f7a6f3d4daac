#!/usr/bin/env python3
"""Build tests/golden/prior_grad_reference.npz (and prior_grad_reference_more.npz): the gradient of the log prior at 50 digits.

The function differentiated is `priorFunction` as the value kernel defines it (csrc/prior_device.hpp, csrc/k_prior.hip), restated
in mpmath at 50 digits: soft node priors with the 1/tH transform of the calibration bounds, the birth-death terms with rho = 1
plus the two `exponential 1` densities, the four clock models plus `exponential ht` on rMu and `gamma(3/2, 1/6)` on rVar.  For a
near-critical chain (|birth - death| < 1e-6) it is what the header of csrc/k_prior_grad.hip defines: the exact formulas at
la_d = fl(death +- 1e-6), la_d formed in fp64 as the kernel forms it and then taken as exact.

Two independent differentiations, which must agree to 1e-35 relative or the generator aborts:
  (a) mpmath.diff of every per-node term in its local variables (the birth-death term in the kernel's own arrangement),
  (b) a forward-mode dual class over mpf (the birth-death term in the `expm1` arrangement).
The contributions are assembled by the tree structure; on trees of at most 25 nodes the whole function is also differentiated
coordinate by coordinate (mpmath.diff on the full sum), which checks the assembly itself.

fp64 yardstick: the dual class run at mp.prec = 53 (IEEE double arithmetic with correctly rounded elementary functions).  Its
error against the 50-digit values is E53; it is measured for the `expm1` arrangement (the yardstick of the tolerance) and for the
arrangement the kernel's duals had before the near-critical fix (printed, and stored as e53k_*).

Tolerance of component k of an output array:   tol_k = 64 * 2^-53 * A_k + 8 * max(E53 over that chain's output array)
with A_k the sum of the absolute values of the addends of that component (per-node tangents, child contributions, soft-bound
terms).  64 is the project's convention (tests/test_gpu_parity.py); 8 = 4 (device exp / log / lgamma at up to 2 ulp against
mpmath's 0.5 ulp) x 2 (another association order).  Nothing here knows a device result.

What is stored.  The cases below do not fit one 512 KiB file with g, A and tol as fp64 arrays per node, model and chain
(the gradients and the inputs alone are about 530 KB), so nothing is stored twice:
  * per chain scalars (birth, death, tH, rMu, rVar): g_*, A_*, tol_* for every model, in full;
  * heights: gH_<m>, AH_<m> per node for m in {bd, 2, 3}: the models UncorrelatedGamma (0) and UncorrelatedLogNormal (1) have no
    clock term that depends on a height, so their g_H and A_H are one array ("bd"); e53_H[chain, model];
  * rates: gR_<model> per node; a rate's gradient has ONE addend, so A_R = |g_R| and is not stored; e53_R[chain, model];
  * tol_H and tol_R are the rule above applied to these stored arrays by `tolerances()` of tests/prior_grad_reference.py (numpy only);
  * the near-critical chains and the 2047-node tree (kPriorGradMaxNodes - 1, the large-LDS path) are a second file; the 2047-node
    tree has ONE chain and TWO clock models (UncorrelatedWhiteNoise, AutocorrelatedLogNormal), the reduction foreseen for it.
Each file stays below 512 KiB.

Run:  python tests/golden/make_prior_grad_reference.py [--check]     (--check: regenerate and compare with the committed files)
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(HERE))
from prior_grad_reference import FILES, SCALARS, U, hkey, tolerances  # noqa: E402  (tests/prior_grad_reference.py: the reader)

SQRT_2_OVER_PI = 0.7978845608028654            # the kernel's constant, taken as exact
LN_SQRT_2PI = 0.9189385332046727417803297364056176
DIGITS = 50
MAX_FILE = 512 * 1024


# ---------------------------------------------------------------------------------------------------------------------------------
# numbers: mpf or Dual over mpf
# ---------------------------------------------------------------------------------------------------------------------------------
from mpmath import mp, mpf  # noqa: E402


class Dual:
    """Forward-mode dual number over mpf with a tuple of tangents; the rules are written as the kernel's D4 writes them."""
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = v, d

    def _c(self, o):
        return o if isinstance(o, Dual) else Dual(mpf(o), (mpf(0),) * len(self.d))

    def __add__(self, o):
        o = self._c(o)
        return Dual(self.v + o.v, tuple(a + b for a, b in zip(self.d, o.d)))

    __radd__ = __add__

    def __sub__(self, o):
        o = self._c(o)
        return Dual(self.v - o.v, tuple(a - b for a, b in zip(self.d, o.d)))

    def __rsub__(self, o):
        return self._c(o) - self

    def __neg__(self):
        return Dual(-self.v, tuple(-a for a in self.d))

    def __mul__(self, o):
        o = self._c(o)
        return Dual(self.v * o.v, tuple(a * o.v + self.v * b for a, b in zip(self.d, o.d)))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._c(o)
        q = self.v / o.v
        return Dual(q, tuple((a - q * b) / o.v for a, b in zip(self.d, o.d)))

    def __rtruediv__(self, o):
        return self._c(o) / self


def seed(values):
    n = len(values)
    return [Dual(mpf(x), tuple(mpf(1) if i == k else mpf(0) for i in range(n))) for k, x in enumerate(values)]


def val(x):
    return x.v if isinstance(x, Dual) else x


_LG = {}


def _loggamma(x):                                   # (a chain evaluates lgamma(1 / rVar) once per node otherwise)
    key = (mp.prec, x)
    if key not in _LG:
        if len(_LG) > 4096:
            _LG.clear()
        _LG[key] = mp.loggamma(x)
    return _LG[key]


def f_exp(x):
    if isinstance(x, Dual):
        e = mp.exp(x.v)
        return Dual(e, tuple(e * a for a in x.d))
    return mp.exp(x)


def f_expm1(x):
    if isinstance(x, Dual):
        e = mp.exp(x.v)
        return Dual(mp.expm1(x.v), tuple(e * a for a in x.d))
    return mp.expm1(x)


def f_log(x):
    if isinstance(x, Dual):
        return Dual(mp.log(x.v), tuple(a / x.v for a in x.d))
    return mp.log(x)


def f_sqrt(x):
    if isinstance(x, Dual):
        s = mp.sqrt(x.v)
        return Dual(s, tuple(mpf(0.5) * a / s for a in x.d))
    return mp.sqrt(x)


def f_lgamma(x):
    if isinstance(x, Dual):
        psi = mp.digamma(x.v)
        return Dual(_loggamma(x.v), tuple(psi * a for a in x.d))
    return _loggamma(x)


# ---------------------------------------------------------------------------------------------------------------------------------
# the terms of priorFunction (prior_device.hpp), generic in the number type
# ---------------------------------------------------------------------------------------------------------------------------------
def bd_term(la, mu, hv, hp, nc, form):
    """ln [D of node v's branch (x la for a bifurcating node)], rho = 1.  form "kernel": the arrangement of prior_bd_term /
    compute_de; form "expm1": the same function with 1 - exp(-d h) = -expm1(-d h), la - mu xx = d - mu expm1(-d h) and the
    denominator -d - expm1(-d br) (e0 la - mu)."""
    br = hp - hv
    d = la - mu
    e0 = 0
    if form == "kernel":
        if nc > 0:
            xx = f_exp(-(la - mu) * hv)
            e0 = mu * (1 - xx) / (la - mu * xx)
        x = f_exp(-d * br)
        y = (mu - e0 * la) * x
        c1 = e0 - 1
        denom = la * c1 + y
    else:
        if nc > 0:
            m1 = f_expm1(-d * hv)
            e0 = mu * (-m1) / (d - mu * m1)
        x = f_exp(-d * br)
        denom = -d - f_expm1(-d * br) * (e0 * la - mu)
    pd = d * d * x / denom / denom
    return f_log(pd * la if nc == 2 else pd)


def ln_gamma_pdf(k, t, x):
    return f_log(x) * (k - 1) - (x / t) - f_lgamma(k) - f_log(t) * k


def ln_lognormal_prime(v, x):
    t = -(mpf(LN_SQRT_2PI) + f_log(x * f_sqrt(v)))
    a = 1 / (2 * v)
    b = f_log(x) + mpf(0.5) * v
    return t + (-(a * b * b))


def ck_term(r, va, hv, hp, model):
    if model == 0:
        return ln_gamma_pdf(1 / va, va, r)
    if model == 1:
        return ln_lognormal_prime(va, r)
    br = hp - hv
    if model == 2:
        v2 = va / br
        return ln_gamma_pdf(1 / v2, v2, r)
    return ln_lognormal_prime(va * br, r)


def normal_ratio(s, x):
    q = x / s
    return mpf(-0.5) * q * q


def cal_term(th, hv, row):
    """One calibration (node, has_lo, lo, lo_p, has_hi, hi, hi_p) as a function of (tH, h_node)."""
    x = 1 / th
    t = 0 * th
    if row[1]:
        a = x * mpf(row[2])
        if val(hv) < val(a):
            t = t + normal_ratio(mpf(SQRT_2_OVER_PI) * mpf(row[3]), a - hv)
    if row[4]:
        b = x * mpf(row[5])
        if val(hv) > val(b):
            t = t + normal_ratio(mpf(SQRT_2_OVER_PI) * mpf(row[6]), hv - b)
    return t


def con_term(hy, ho, p):
    if val(hy) < val(ho):
        return 0 * hy
    return normal_ratio(mpf(SQRT_2_OVER_PI) * mpf(p), hy - ho)


def brace_term(hs, sd):
    if all(val(h) == val(hs[0]) for h in hs):
        return 0 * hs[0]
    s = hs[0]
    for h in hs[1:]:
        s = s + h
    mean = s / len(hs)
    t = 0 * hs[0]
    for h in hs:
        t = t + normal_ratio(mpf(sd), h - mean)
    return t


def scalar_terms(la, mu, rm, va, ht):
    """exponential 1 la, exponential 1 mu, exponential ht rMu, gamma(3/2, 1/6) rVar."""
    hyper = f_log(va) * mpf(0.5) - va * 6 - _loggamma(mpf(1.5)) - mp.log(mpf(1) / 6) * mpf(1.5)
    return (-la) + (-mu) + (mp.log(mpf(ht)) - mpf(ht) * rm) + hyper


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def children_of(parent):
    n = len(parent)
    kids = [[] for _ in range(n)]
    for v in range(1, n):
        kids[int(parent[v])].append(v)
    return kids


def heights(parent, batch, rng, short=True):
    """Ultrametric relative heights, root 1, leaves 0: h_v = (D(v) + u_v) / (D(root) + 1) with D the depth of v's subtree in
    edges and u_v uniform in (0.05, 0.95), so branches do not shrink geometrically with the depth; every eighth internal
    node whose parent is not shortened sits a log-uniform 1e-4 .. 1e-2 below its parent."""
    n = len(parent)
    kids = children_of(parent)
    depth = np.zeros(n, int)
    for v in range(n - 1, -1, -1):
        if kids[v]:
            depth[v] = 1 + max(depth[c] for c in kids[v])
    dr = depth[0] + 1.0
    H = np.zeros((batch, n))
    for b in range(batch):
        shortened = np.zeros(n, bool)
        for v in range(n):
            if v == 0:
                H[b, 0] = 1.0
            elif kids[v]:
                H[b, v] = (depth[v] + rng.uniform(0.05, 0.95)) / dr
                p = int(parent[v])
                if short and p != 0 and depth[v] == depth[p] - 1 and not shortened[p] and rng.random() < 0.125:
                    H[b, v] = H[b, p] - np.exp(rng.uniform(np.log(1e-4), np.log(min(1e-2, 0.4 / dr))))
                    shortened[v] = True
    return H


def regular_rates(rng, batch):
    lo, hi = np.log(0.3), np.log(3.0)
    birth, death = np.empty(batch), np.empty(batch)
    for b in range(batch):
        while True:
            x, y = np.exp(rng.uniform(lo, hi, 2))
            if abs(x - y) >= 0.1 * max(x, y):
                birth[b], death[b] = x, y
                break
    return birth, death


def states(parent, batch, rng, H=None, R=None, tH=None, rMu=None, th_one=0):
    n = len(parent)
    st = {}
    st["H"] = heights(parent, batch, rng) if H is None else np.array(H, float)
    if R is None:
        R = np.exp(0.2 * rng.standard_normal((batch, n)))
        R[:, 0] = 0.0
    st["R"] = np.array(R, float)
    st["tH"] = np.exp(0.05 * rng.standard_normal(batch)) if tH is None else np.array(tH, float)
    st["tH"][th_one] = 1.0
    st["rMu"] = np.exp(0.05 * rng.standard_normal(batch)) if rMu is None else np.array(rMu, float)
    st["birth"], st["death"] = regular_rates(rng, batch)
    st["rVar"] = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), batch))
    return st


def make_near(st):
    """Three chains with chain 0's state: birth = death = 1; birth = death + 3e-7; birth = death - 9.9e-7."""
    out = {k: np.repeat(v[:1], 3, axis=0) for k, v in st.items()}
    out["death"] = np.ones(3)
    out["birth"] = np.array([1.0, 1.0 + 3e-7, 1.0 - 9.9e-7])
    out["tH"] = np.array([1.0, st["tH"][0], st["tH"][0]])
    assert st["tH"][0] != 1.0
    return out


def tables(parent, H, tH, rng, n_cal, n_con, n_brace):
    """Soft-bound tables on a synthetic tree.  Bounds are placed relative to chain 0 (absolute time = tH x relative height)."""
    n = len(parent)
    kids = children_of(parent)
    inner = [v for v in range(1, n) if kids[v]]
    leaves = [v for v in range(1, n) if not kids[v]]
    h0, t0 = H[0], float(tH[0])
    cal, con = [], []

    def one(v, kind, f_lo, f_hi):
        base = t0 * (h0[v] if h0[v] > 0 else 0.2)
        p = lambda: float(np.round(rng.uniform(0.025, 0.5), 4))
        return [v, int(kind != "hi"), base * f_lo if kind != "hi" else 0.0, p() if kind != "hi" else 0.0,
                int(kind != "lo"), base * f_hi if kind != "lo" else 0.0, p() if kind != "lo" else 0.0]

    if n_cal >= 1:
        cal.append(one(0, "both", 1.03, 1.2))                       # root: lower bound active for tH <~ 1.03 t0
    if n_cal >= 2 and inner:
        cal.append(one(inner[len(inner) // 2], "lo", 2.5, 0))
    if n_cal >= 3:
        cal.append(one(leaves[len(leaves) // 3], "lo", 0.5, 0))     # a leaf: h = 0 is below the bound, whatever the chain
    if n_cal > 3:
        cal.append(one(cal[1][0], "hi", 0, 0.4))                    # two on the same node
        cal.append(one(0, "hi", 0, 0.97))                           # root again, upper only, active
        cal.append(one(0, "lo", 0.8, 0))                            # root, lower only, mostly idle
        while len(cal) < n_cal:
            i = len(cal)
            if i % 5 == 0:
                cal.append(one(int(rng.choice(leaves)), "lo", rng.uniform(0.2, 1.5), 0))
            else:
                v = int(rng.choice(inner))
                kind = ("lo", "hi", "both")[i % 3]
                far = rng.random() < 0.7
                cal.append(one(v, kind, rng.choice([2.5, 1.1]) if far else 0.9, rng.choice([0.4, 0.9]) if far and kind != "both" else 3.0))
    # constraints: (young, old) with young an ancestor of old are violated in every chain; the rest are random pairs
    for i in range(n_con):
        if i % 3 != 2 and len(inner) > 2:
            o = int(rng.choice(inner))
            y = int(parent[o])
            con.append([y, o, float(np.round(rng.uniform(0.025, 0.5), 4))])
        else:
            y, o = (int(x) for x in rng.choice(inner if len(inner) > 2 else np.arange(n), 2, replace=False))
            con.append([y, o, float(np.round(rng.uniform(0.025, 0.5), 4))])
    braces = []
    if n_brace >= 1 and len(inner) >= 4:
        a = [int(x) for x in rng.choice(inner, 3, replace=False)]
        braces.append((a, 0.05))
        if n_brace >= 2:
            braces.append(([a[0], int(rng.choice([v for v in inner if v not in a]))], 0.2))      # shares a node with the first
            braces.append(([int(x) for x in leaves[:3]], 0.01))                                  # all heights equal (0): no term
            while len(braces) < n_brace:
                k = int(rng.integers(2, 5))
                braces.append(([int(x) for x in rng.choice(inner, k, replace=False)], float(np.round(rng.uniform(0.05, 0.3), 3))))
    ptr = np.concatenate([[0], np.cumsum([len(b[0]) for b in braces])]).astype(np.int32)
    return (np.array(cal, float).reshape(-1, 7), np.array(con, float).reshape(-1, 3), ptr,
            np.array([v for b in braces for v in b[0]], np.int32), np.array([b[1] for b in braces], float))


def build_cases(which):
    from mcmc_date_amd import synthetic as S

    cases = {}
    if which == "more":
        rng = np.random.default_rng(2047)
        parent = np.asarray(S.random_topology(1024, seed=11).parent, np.int32)
        st = states(parent, 1, rng)
        st["tH"][0] = 1.0371                                       # (one chain: tH != 1; there is no calibration to transform)
        st["rVar"][0] = 0.37
        cases["n2047"] = dict(parent=parent, ht=np.float64(0.75), models=np.array([2, 3], np.int32), near=np.zeros(1, np.int32),
                              cal=np.zeros((0, 7)), con=np.zeros((0, 3)), brace_ptr=np.zeros(1, np.int32),
                              brace_nodes=np.zeros(0, np.int32), brace_sd=np.zeros(0), **st)
    all_models = np.arange(4, dtype=np.int32)
    for leaves in (2, 32, 33, 64, 65, 128, 129):
        n = 2 * leaves - 1
        rng = np.random.default_rng(1000 + n)
        parent = np.asarray(S.random_topology(leaves, seed=n).parent, np.int32)
        st = states(parent, 4, rng, th_one=1)
        tb = tables(parent, st["H"], st["tH"], rng, 1 if n == 3 else 3, 0 if n == 3 else 2, 0 if n == 3 else 1)
        cases[f"n{n}"] = dict(parent=parent, ht=np.float64(0.75), models=all_models, near=np.zeros(4, np.int32), cal=tb[0], con=tb[1],
                              brace_ptr=tb[2], brace_nodes=tb[3], brace_sd=tb[4], **st)
        if n in (65, 257):
            cases[f"n{n}near"] = dict(cases[f"n{n}"], near=np.ones(3, np.int32), **make_near(st))
        if n == 257:
            rng = np.random.default_rng(70705)
            st2 = states(parent, 2, rng, th_one=1)
            tb = tables(parent, st2["H"], st2["tH"], rng, 70, 70, 5)
            cases["n257tables"] = dict(parent=parent, ht=np.float64(0.75), models=all_models, near=np.zeros(2, np.int32), cal=tb[0], con=tb[1],
                                       brace_ptr=tb[2], brace_nodes=tb[3], brace_sd=tb[4], **st2)
    for name in ("12-leaves-variable-rate", "24-leaves-braces"):
        fx = np.load(os.path.join(HERE, name + ".npz"))
        rng = np.random.default_rng(500 + len(fx["parent"]))
        pick = [0, 2, 3]
        st = states(fx["parent"], 3, rng, H=fx["H"][pick], R=fx["R"][pick], tH=fx["prior_tH"][pick], rMu=fx["rMu"][pick], th_one=2)
        st["tH"][0] = 1.25 * fx["cal"][1, 5] / st["H"][0, int(fx["cal"][1, 0])]           # an upper bound active away from tH = 1
        key = "fx" + name[:2]
        cases[key] = dict(parent=np.asarray(fx["parent"], np.int32), ht=np.float64(fx["prior_ht"]), models=all_models, near=np.zeros(3, np.int32),
                          cal=np.array(fx["cal"], float), con=np.array(fx["con"], float), brace_ptr=np.asarray(fx["brace_ptr"], np.int32),
                          brace_nodes=np.asarray(fx["brace_nodes"], np.int32), brace_sd=np.array(fx["brace_sd"], float), **st)
        if name.startswith("24"):
            cases[key + "near"] = dict(cases[key], near=np.ones(3, np.int32), **make_near(st))
    return {k: c for k, c in cases.items() if (which == "more") == (k.endswith("near") or k == "n2047")}


# ---------------------------------------------------------------------------------------------------------------------------------
# one chain
# ---------------------------------------------------------------------------------------------------------------------------------
def agree(a, b, what):
    scale = max(abs(a), abs(b))
    if abs(a - b) > mpf(10) ** -35 * scale + mpf(10) ** -60:
        raise SystemExit(f"differentiations (a) and (b) disagree: {what}: {mp.nstr(a, 45)} vs {mp.nstr(b, 45)}")


def la_dual(birth, death, near):
    """The birth rate the duals are taken at: line `la_d = near ? mu + (la >= mu ? 1e-6 : -1e-6) : la` of the kernel, in fp64."""
    if not near:
        return float(birth)
    return float(np.float64(death) + (np.float64(1e-6) if birth >= death else np.float64(-1e-6)))


def soft_terms(case, b):
    """[(nodes, value, d/d tH, [d/d h_node ...])] of every soft bound of chain b at the working precision, by duals; at 50
    digits every derivative is also taken with mpmath.diff."""
    H, th = case["H"][b], float(case["tH"][b])
    check = mp.prec > 60
    out = []
    for row in case["cal"]:
        v = int(row[0])
        dth, dh = seed([th, H[v]])
        t = cal_term(dth, dh, row)
        if not isinstance(t, Dual):
            t = dth._c(t)
        if check:
            f = lambda a, c: cal_term(a, c, row)
            agree(mp.diff(f, (mpf(th), mpf(H[v])), (1, 0)), t.d[0], "calibration d/d tH")
            agree(mp.diff(f, (mpf(th), mpf(H[v])), (0, 1)), t.d[1], "calibration d/d h")
            for bound, on in ((row[2], row[1]), (row[5], row[4])):
                if on and abs(H[v] - bound / th) <= 1e-9 * max(1.0, bound / th):
                    raise SystemExit("a calibration bound sits on a node's height: change the inputs")
        out.append(([v], t.v, t.d[0], [t.d[1]]))
    for y, o, p in case["con"]:
        y, o = int(y), int(o)
        dy, do = seed([H[y], H[o]])
        t = con_term(dy, do, p)
        if check:
            f = lambda a, c: con_term(a, c, p)
            agree(mp.diff(f, (mpf(H[y]), mpf(H[o])), (1, 0)), t.d[0], "constraint d/d h_young")
            agree(mp.diff(f, (mpf(H[y]), mpf(H[o])), (0, 1)), t.d[1], "constraint d/d h_old")
            if y != o and H[y] == H[o]:
                raise SystemExit("a constraint sits on its edge: change the inputs")
        out.append(([y, o], t.v, mpf(0), list(t.d)))
    ptr = case["brace_ptr"]
    for i, sd in enumerate(case["brace_sd"]):
        nodes = [int(x) for x in case["brace_nodes"][ptr[i]:ptr[i + 1]]]
        hs = seed([H[v] for v in nodes])
        t = brace_term(hs, sd)
        if check:
            for j in range(len(nodes)):
                order = tuple(int(k == j) for k in range(len(nodes)))
                agree(mp.diff(lambda *a: brace_term(list(a), sd), tuple(mpf(H[v]) for v in nodes), order), t.d[j], "brace d/d h")
        out.append((nodes, t.v, mpf(0), list(t.d)))
    return out


def evaluate(case, b, model, form, check=False, check_bd=False):
    """lp and the gradient of chain b at the working precision (duals, arrangement `form`), with the sums of absolute addends.
    check: every per-node derivative is also taken with mpmath.diff of the OTHER arrangement and compared."""
    parent, H, R = case["parent"], case["H"][b], case["R"][b]
    n = len(parent)
    kids = children_of(parent)
    mu, va, rm = (float(case[k][b]) for k in ("death", "rVar", "rMu"))
    ht = float(case["ht"])
    la = la_dual(case["birth"][b], mu, case["near"][b])
    z = mpf(0)
    g = dict(birth=mpf(-1), death=mpf(-1), tH=z, rMu=-mpf(ht), rVar=mpf(0.5) / mpf(va) - 6, H=[z] * n, R=[z] * n)
    A = dict(birth=mpf(1), death=mpf(1), tH=z, rMu=mpf(ht), rVar=mpf(0.5) / mpf(va) + 6, H=[z] * n, R=[z] * n)
    lp = scalar_terms(mpf(la), mpf(mu), mpf(rm), mpf(va), ht)
    for v in range(1, n):
        p, nc = int(parent[v]), len(kids[v])
        x = [la, mu, H[v], H[p]]
        t = bd_term(*seed(x), nc, form)
        if check and check_bd:
            other = "kernel" if form == "expm1" else "expm1"
            for k in range(4):
                order = tuple(int(i == k) for i in range(4))
                agree(mp.diff(lambda *a: bd_term(*a, nc, other), tuple(mpf(q) for q in x), order), t.d[k], f"birth-death node {v} d[{k}]")
        y = [R[v], va, H[v], H[p]]
        c = ck_term(*seed(y), model)
        if check:
            for k in range(2 if model < 2 else 4):
                order = tuple(int(i == k) for i in range(4))
                agree(mp.diff(lambda *a: ck_term(*a, model), tuple(mpf(q) for q in y), order), c.d[k], f"clock {model} node {v} d[{k}]")
        lp = lp + t.v + c.v
        for key, d in (("birth", t.d[0]), ("death", t.d[1]), ("rVar", c.d[1])):
            g[key] += d
            A[key] += abs(d)
        g["R"][v], A["R"][v] = c.d[0], abs(c.d[0])
        for node, k in ((v, 2), (p, 3)):
            g["H"][node] += t.d[k] + c.d[k]
            A["H"][node] += abs(t.d[k]) + abs(c.d[k])
    node_prior = z
    for nodes, value, dth, dhs in soft_terms(case, b):
        node_prior += value
        g["tH"] += dth
        A["tH"] += abs(dth)
        for node, d in zip(nodes, dhs):
            g["H"][node] += d
            A["H"][node] += abs(d)
    return lp + node_prior, node_prior, g, A


def full_value(case, b, model, vec):
    """The whole log prior as a function of the flat coordinate vector (birth, death, tH, H.., rMu, rVar, R..)."""
    parent = case["parent"]
    n = len(parent)
    kids = children_of(parent)
    la, mu, th = vec[0], vec[1], vec[2]
    H, rm, va, R = vec[3:3 + n], vec[3 + n], vec[4 + n], vec[5 + n:]
    lp = scalar_terms(la, mu, rm, va, float(case["ht"]))
    for v in range(1, n):
        p = int(parent[v])
        lp += bd_term(la, mu, H[v], H[p], len(kids[v]), "kernel") + ck_term(R[v], va, H[v], H[p], model)
    for row in case["cal"]:
        lp += cal_term(th, H[int(row[0])], row)
    for y, o, p in case["con"]:
        lp += con_term(H[int(y)], H[int(o)], p)
    ptr = case["brace_ptr"]
    for i, sd in enumerate(case["brace_sd"]):
        lp += brace_term([H[int(x)] for x in case["brace_nodes"][ptr[i]:ptr[i + 1]]], sd)
    return lp


def check_assembly(case, b, model, g):
    n = len(case["parent"])
    la = la_dual(case["birth"][b], case["death"][b], case["near"][b])
    x0 = [mpf(la), mpf(float(case["death"][b])), mpf(float(case["tH"][b]))] + [mpf(float(h)) for h in case["H"][b]] + \
         [mpf(float(case["rMu"][b])), mpf(float(case["rVar"][b]))] + [mpf(float(r)) for r in case["R"][b]]
    flat = [g["birth"], g["death"], g["tH"]] + g["H"] + [g["rMu"], g["rVar"]] + g["R"]
    for i in range(len(x0)):
        if i == 5 + n:
            continue                                                # the root's rate is no argument of the prior
        d = mp.diff(lambda t: full_value(case, b, model, x0[:i] + [t] + x0[i + 1:]), x0[i])
        if abs(d - flat[i]) > mpf(10) ** -35 * max(abs(d), abs(flat[i])) + mpf(10) ** -40:
            raise SystemExit(f"assembly check failed at coordinate {i}: {mp.nstr(d, 40)} vs {mp.nstr(flat[i], 40)}")


def chain_reference(args):
    """Everything stored for one chain: dict name -> float / array, per model."""
    case, b = args
    n = len(case["parent"])
    out = {}
    for model in (int(m) for m in case["models"]):
        mp.dps = DIGITS
        lp, node_prior, g, A = evaluate(case, b, model, "expm1", check=True, check_bd=(model == int(case["models"][0])))
        if n <= 25:
            check_assembly(case, b, model, g)
        r = {"lp": float(lp), "node_prior": float(node_prior)}
        flat = lambda d, k: np.array([float(x) for x in d[k]]) if k in ("H", "R") else float(d[k])
        for k in SCALARS + ["H", "R"]:
            r["g_" + k], r["A_" + k] = flat(g, k), flat(A, k)
        for form, tag in (("expm1", "e53_"), ("kernel", "e53k_")):
            mp.prec = 53
            _, _, g53, _ = evaluate(case, b, model, form)
            mp.dps = DIGITS
            for k in SCALARS:
                r[tag + k] = float(abs(g53[k] - g[k]))
            for k in ("H", "R"):
                r[tag + k] = float(max(abs(x - y) for x, y in zip(g53[k], g[k])))
            if form == "kernel":
                r["g53k_birth"], r["g53k_death"] = float(g53["birth"]), float(g53["death"])
        out[model] = r
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------------------------------
INPUTS = ["parent", "ht", "models", "near", "cal", "con", "brace_ptr", "brace_nodes", "brace_sd", "H", "R", "tH", "rMu", "birth", "death", "rVar"]


def assemble(case, chains):
    """The arrays of one case from its chains' results; asserts the caps of the tolerance rule."""
    B, models = len(chains), [int(m) for m in case["models"]]
    out = {k: np.asarray(case[k]) for k in INPUTS}
    per = ["lp", "node_prior", "g53k_birth", "g53k_death", "e53_H", "e53_R", "e53k_H", "e53k_R"] + \
          [p + s for p in ("g_", "A_", "e53_", "e53k_") for s in SCALARS]
    for k in per + ["tol_" + s for s in SCALARS]:
        out[k] = np.full((B, 4), np.nan)                            # [chain, model]; NaN for a model the case does not carry
    for m in models:
        for k in per:
            out[k][:, m] = [c[m][k] for c in chains]
        for s in SCALARS:
            out["tol_" + s][:, m] = 64 * U * out["A_" + s][:, m] + 8 * out["e53_" + s][:, m]
        out[f"gR_{m}"] = np.array([c[m]["g_R"] for c in chains])
        assert all(np.array_equal(np.abs(c[m]["g_R"]), c[m]["A_R"]) for c in chains)         # one addend: A_R = |g_R|
        hk = hkey(m)
        gh, ah = np.array([c[m]["g_H"] for c in chains]), np.array([c[m]["A_H"] for c in chains])
        if "gH_" + hk in out:
            assert np.array_equal(out["gH_" + hk], gh) and np.array_equal(out["AH_" + hk], ah)    # models 0 and 1: the same bits
        out["gH_" + hk], out["AH_" + hk] = gh, ah
    return out


def check_caps(name, c):
    """The conditions of the tolerance rule; the sensitivity of the near-critical chains.  Returns True if the arrangement of
    the duals before the fix, in fp64, violates tol in g_birth or g_death on some near-critical chain."""
    sensitive = False
    for m in (int(x) for x in c["models"]):
        tol = tolerances(c, m)
        ref = dict(H=c["gH_" + hkey(m)], R=c[f"gR_{m}"], **{s: c["g_" + s][:, m] for s in SCALARS})
        for b in range(len(c["tH"])):
            near = bool(c["near"][b])
            for k in SCALARS + ["H", "R"]:
                t, g = np.atleast_1d(tol[k][b]), np.atleast_1d(ref[k][b])
                cap = 1e-10 * max(1.0, np.abs(g).max())
                if near:
                    cap = 1e-5 * max(1.0, np.abs(g).max()) if k in ("birth", "death") else cap * 1e3
                if not np.all(t <= cap):
                    raise SystemExit(f"{name} chain {b} model {m} {k}: tolerance {t.max():.3e} above its cap {cap:.3e}: change the inputs")
            if near:
                for k in ("birth", "death"):
                    if abs(c["g53k_" + k][b, m] - ref[k][b]) > tol[k][b]:
                        sensitive = True
    return sensitive


def count_active(c, b):
    H, th = c["H"][b], c["tH"][b]
    n_cal = sum(1 for r in c["cal"] if (r[1] and H[int(r[0])] < r[2] / th) or (r[4] and H[int(r[0])] > r[5] / th))
    n_con = sum(1 for y, o, _ in c["con"] if not H[int(y)] < H[int(o)])
    return n_cal, n_con


def savez_bytes(arrays):
    """np.savez_compressed into memory with fixed time stamps, so that the same arrays give the same file."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), a.getvalue(), zipfile.ZIP_DEFLATED)
    return buf.getvalue()


def generate(which, only=None, pool=None):
    """{case: arrays} of one file; only = {case name: [chain indices]} restricts the work (the host test's stale-fixture check)."""
    cases = build_cases(which)
    jobs = [(name, b) for name, c in cases.items() for b in range(len(c["tH"])) if only is None or b in only.get(name, [])]
    run = pool.map if pool is not None else map
    res = list(run(chain_reference, [(cases[name], b) for name, b in jobs]))
    out = {}
    for name, c in cases.items():
        chains = [r for (nm, _), r in zip(jobs, res) if nm == name]
        if not chains:
            continue
        if only is not None:
            idx = only[name]
            c = dict(c, **{k: c[k][idx] for k in ("H", "R", "tH", "rMu", "birth", "death", "rVar", "near")})
        out[name] = assemble(c, chains)
    return out


def report(name, c):
    for m in (int(x) for x in c["models"]):
        for k in SCALARS + ["H", "R"]:
            print(f"  E53 {name:12s} model {m} {k:6s} expm1 {np.nanmax(c['e53_' + k][:, m]):.3e}   kernel {np.nanmax(c['e53k_' + k][:, m]):.3e}")


def main():
    import multiprocessing as mpc

    check_only = "--check" in sys.argv
    with mpc.get_context("fork").Pool(min(16, os.cpu_count() or 1)) as pool:
        for which in ("main", "more"):
            cases = generate(which, pool=pool)
            sensitive = False
            for name, c in cases.items():
                report(name, c)
                sensitive = check_caps(name, c) or sensitive
                hmin = min((c["H"][b, int(c["parent"][v])] - c["H"][b, v]) for b in range(len(c["tH"])) for v in range(1, len(c["parent"])))
                print(f"{name}: {len(c['parent'])} nodes, {len(c['tH'])} chains, shortest branch {hmin:.2e}, active (cal, con) per chain "
                      f"{[count_active(c, b) for b in range(len(c['tH']))]}")
            if which == "more" and not sensitive:
                raise SystemExit("no near-critical chain tells the old arrangement of the duals from the expm1 one: change the inputs")
            if which == "main":
                t = cases["n257tables"]
                assert len(t["cal"]) == 70 and len(t["con"]) == 70 and len(t["brace_sd"]) == 5
                for b in range(len(t["tH"])):
                    a = count_active(t, b)
                    assert a[0] >= 40 and a[1] >= 40, a
            blob = savez_bytes({f"{name}/{k}": v for name, c in cases.items() for k, v in c.items()})
            path = os.path.join(HERE, FILES[which])
            print(f"{FILES[which]}: {len(blob)} bytes")
            if len(blob) > MAX_FILE:
                raise SystemExit(f"{FILES[which]} is larger than {MAX_FILE} bytes")
            if check_only:
                if open(path, "rb").read() != blob:
                    raise SystemExit(f"{FILES[which]} differs from the committed file")
                print("  identical to the committed file")
            else:
                with open(path, "wb") as f:
                    f.write(blob)


if __name__ == "__main__":
    main()
