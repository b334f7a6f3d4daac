#!/usr/bin/env python3
"""Tree state -> ln likelihood + state gradient over the sparse precision matrix (mcd_sparse_tree_grad_batch, csrc/k_sparse_grad.hip) next to
the only route there was before it, mcd_tree_grad_batch on the densified matrix: microseconds per call, device-resident states, both sides
in ONE process, the median (and minimum) of interleaved repeats; a repeat is `calls` back-to-back calls of the C ABI on one stream between
two synchronisations (wall clock: a kernel shorter than the host's launch path shows that path).  Sizes: 1025 nodes x 512 chains for both; 2013 x 512 and 13 x 128 for the
sparse kernel alone (no dense handle beyond 1024 dimensions; the small one shows the launch floor).  Matrix: synthetic.banded_precision.
Usage: python tools/bench_sparse_grad.py [--repeats 5] [--calls 200] [--budget-s 240]      (one JSON line per size)
The wall-clock budget is the tool's own: a size that would start after it is skipped and reported as such."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, calls, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / calls


def grad_call(tl, st, torch):
    """The C ABI call itself on preallocated device outputs (no allocation, no Python mirror in the timed loop)."""
    import ctypes as C

    from mcmc_date_amd import _capi
    from mcmc_date_amd.likelihood import SparseTreeLikelihood, _stream_ptr

    L = _capi.lib()
    fn = L.mcd_sparse_tree_grad_batch if isinstance(tl, SparseTreeLikelihood) else L.mcd_tree_grad_batch
    B = st.heights.shape[0]
    out = [torch.empty(B, dtype=torch.float64, device=st.heights.device), torch.empty_like(st.heights), torch.empty_like(st.rates),
           torch.empty_like(st.time_height), torch.empty_like(st.rate_mean)]
    args = [tl._t] + [C.c_void_p(t.data_ptr()) for t in (st.heights, st.rates)] + [st.heights.stride(0)] + \
           [C.c_void_p(t.data_ptr()) for t in (st.time_height, st.rate_mean)] + [B, 1, _stream_ptr(st.heights.device.index or 0)] + \
           [C.c_void_p(t.data_ptr()) for t in out]

    def call():
        _capi.check(fn(*args))

    call.out = out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--budget-s", type=float, default=240.0)
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error("at least three interleaved repeats")
    import torch

    import mcmc_date_amd as M
    from mcmc_date_amd import synthetic as S

    t_start = time.perf_counter()
    dev = torch.device("cuda:0")
    for n_leaves, B, with_dense in ((513, 512, True), (1007, 512, False), (7, 128, False)):
        topo = S.random_topology(n_leaves, seed=3)
        n = topo.n_nodes - 2
        rec = {"metric": "tree ll + state gradient, us per call", "n_nodes": topo.n_nodes, "chains": B, "calls": a.calls, "repeats": a.repeats}
        if time.perf_counter() - t_start > a.budget_s:
            rec["skipped"] = "wall-clock budget"
            print(json.dumps(rec), flush=True)
            continue
        P, assoc = S.banded_precision(n, seed=3)
        mu = np.random.default_rng(3).uniform(0.01, 0.2, n)
        st = S.random_states(topo, B, seed=4).to(dev)
        sides = {"sparse": M.SparseLikelihood(M.Sparse(mu, assoc, 0.0)).bind_tree(topo)}
        rec["nnz"] = int(P.nnz)
        if with_dense:
            sides["dense"] = M.MvnLikelihood(M.Full(mu, P.toarray(), 0.0)).bind_tree(topo)
        calls = {k: grad_call(tl, st, torch) for k, tl in sides.items()}
        for c in calls.values():                        # warm-up: first launches, per-device attributes
            for _ in range(10):
                c()
        us = {k: [] for k in sides}
        for _ in range(a.repeats):                      # interleaved: sparse, dense, sparse, dense, ...
            for k, c in calls.items():
                us[k].append(timed(c, a.calls, torch))
        for k, v in us.items():
            rec[k + "_us_median"] = float(np.median(v))
            rec[k + "_us_min"] = float(np.min(v))
            rec[k + "_us_all"] = [round(x, 2) for x in v]
        if with_dense:
            ls, ld = calls["sparse"].out[0], calls["dense"].out[0]
            rec["max_rel_ll_difference"] = float(torch.max(torch.abs(ls - ld) / torch.abs(ld)))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
