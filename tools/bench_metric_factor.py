#!/usr/bin/env python3
"""Wall time of the dense metric's factorisation, hmc.factor_metric (mcd_metric_factor): the host's long double loops next to the device
kernels (csrc/k_metric_factor.hip) on what the warm-up hands them -- the shrunk covariance of a rank-deficient window, n = dim // 2
positions.  One JSON line per size.  Usage: python tools/bench_metric_factor.py [--dims 387,1539,3072,4098] [--repeat 5] [--host-max 3072]
The call is timed as a caller sees it: upload of C, pre-pass, factor, inverse, the status word, download of sym, U and U^-1 (the handle's
path, Leapfrog.set_metric_factor("device"), keeps all of that on the device: tools/bench_nuts.py --metric-factor times it).  A small
matrix is factored first so that loading the library and creating the context are not in the figure; the device figure is the median of
--repeat calls, the host figure one call (seconds to minutes), skipped above --host-max.  Every size runs in a child process of its own
under a time limit sized to it; after a child that fails or runs out of time nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(dim):
    import mcmc_date_amd as M

    rng = np.random.default_rng(dim)
    n = dim // 2
    Q = rng.standard_normal((n, dim)) * (0.05 * np.exp(rng.standard_normal(dim)))
    C = M.shrunk_covariance(Q)
    return 0.5 * (C + C.T), n


def one(dim, host, repeat):
    import mcmc_date_amd as M

    C, n = problem(dim)
    out = {"dim": dim, "positions": n}
    M.factor_metric(problem(16)[0], where="device")                    # library, context
    runs = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        sym, U, W = M.factor_metric(C, where="device")
        runs.append(time.perf_counter() - t0)
    out.update({"device_s_runs": runs, "device_s": statistics.median(runs)})
    scale = np.sqrt(np.outer(np.diag(sym), np.diag(sym)))
    out["device_residual"] = float(np.max(np.abs(U @ U.T - sym) / scale))           # in double: an order of magnitude, not a test
    out["device_inverse_residual"] = float(np.max(np.abs(U @ W - np.eye(dim))))
    if host:
        t0 = time.perf_counter()
        sym_h, U_h, W_h = M.factor_metric(C, where="host")
        out["host_s"] = time.perf_counter() - t0
        out["host_over_device"] = out["host_s"] / out["device_s"]
        out["equal_sym"] = bool(np.array_equal(sym, sym_h))
        out["max_rel_dU"] = float(np.max(np.abs(U - U_h) / np.sqrt(np.outer(np.diag(U_h), np.diag(U_h)))))
    print(json.dumps(out), flush=True)


def limit(dim, host):
    return int(60 + (dim / 4098.0) ** 2 * 120 + (3 * (dim / 1024.0) ** 3 if host else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="387,1539,3072,4098")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=3072)
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--host", type=int, default=0)
    args = ap.parse_args()
    if args.one:
        one(args.one, bool(args.host), args.repeat)
        return 0
    for dim in [int(x) for x in args.dims.split(",") if x]:
        host = int(dim <= args.host_max)
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(dim), "--host", str(host), "--repeat", str(args.repeat)]
        try:
            rc = subprocess.run(cmd, timeout=limit(dim, host)).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"dim": dim, "error": f"time limit of {limit(dim, host)} s"}), flush=True)
            return 124
        if rc != 0:
            print(json.dumps({"dim": dim, "error": f"exit status {rc}"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
