"""Reader of tests/golden/prior_grad_reference*.npz (written by tests/golden/make_prior_grad_reference.py, which explains the
layout) and the tolerance rule those files carry.  numpy only: the tests that use it need neither mpmath nor an oracle."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = ["UncorrelatedGamma", "UncorrelatedLogNormal", "UncorrelatedWhiteNoise", "AutocorrelatedLogNormal"]
FILES = {"main": "prior_grad_reference.npz", "more": "prior_grad_reference_more.npz"}
SCALARS = ["birth", "death", "tH", "rMu", "rVar"]
SHARED = ["parent", "ht", "models", "cal", "con", "brace_ptr", "brace_nodes", "brace_sd"]   # every other array: [chain, ...]
U = 2.0 ** -53


def hkey(model):
    """The g_H / A_H array of a clock model: UncorrelatedGamma (0) and UncorrelatedLogNormal (1) have no clock term that
    depends on a height, so they share the birth-death + soft-bound array "bd"."""
    return "bd" if model < 2 else str(model)


def reference(case, model):
    """name -> 50-digit gradient rounded to fp64, shaped like the kernel's output ([B] or [B, n_nodes])."""
    g = {k: case["g_" + k][:, model] for k in SCALARS}
    g["H"], g["R"] = case["gH_" + hkey(model)], case[f"gR_{model}"]
    return g


def tolerances(case, model):
    """tol_k = 64 * 2^-53 * A_k + 8 * max(E53 over that chain's output array): stored for the scalars, applied here to the
    stored A_H, |g_R| (a rate's gradient has one addend: A_R = |g_R|) and E53 for the per-node arrays."""
    t = {k: case["tol_" + k][:, model] for k in SCALARS}
    t["H"] = 64 * U * case["AH_" + hkey(model)] + 8 * case["e53_H"][:, model][:, None]
    t["R"] = 64 * U * np.abs(case[f"gR_{model}"]) + 8 * case["e53_R"][:, model][:, None]
    return t


def load(which="main"):
    """{case name: {array name: array}} of one of the two files."""
    out = {}
    with np.load(os.path.join(GOLDEN, FILES[which])) as z:
        for key in z.files:
            name, arr = key.split("/", 1)
            out.setdefault(name, {})[arr] = z[key]
    return out
