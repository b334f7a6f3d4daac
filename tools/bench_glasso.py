#!/usr/bin/env python3
"""Wall time of the graphical lasso of `prepare`'s sparse specification: the host solver (prepare.graphical_lasso) next to the device
solver (prepare.graphical_lasso_device, csrc/k_glasso.hip) on synthetic AR(1)-correlated data (a = 0.6, 2 p samples, at least 200),
rho = 0.1, tol = 1e-10.  One JSON line per size.  Usage: python tools/bench_glasso.py [--both 48,96,192] [--device 512,1024,2011]
  --both    sizes solved by host and device (the difference of the two results is reported)
  --device  sizes solved by the device alone; at the largest the optimality residuals of tests/test_gpu_glasso.py are reported too
Every size runs in a child process of its own under a time limit sized to it; after a child that fails or runs out of time nothing more
is started.  The device call is timed as a user sees it (screening, upload, passes, Theta, download); a small problem is solved first so
that loading the library and creating the context are not in the figure."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RHO = 0.1


def problem(p):
    from glasso_inputs import ar

    n = max(200, 2 * p)
    return np.corrcoef(ar(np.random.default_rng(p), p, n), rowvar=False), n


def one(p, host, residuals):
    import mcmc_date_amd as M
    from glasso_inputs import optimality_violations

    S, n = problem(p)
    out = {"p": p, "samples": n, "rho": RHO, "tol": 1e-10}
    M.graphical_lasso_device(problem(16)[0], RHO)                       # library, context
    runs = []
    for _ in range(1 if residuals else 2):
        t0 = time.perf_counter()
        W, T, info = M.graphical_lasso_device(S, RHO, return_info=True)
        runs.append(time.perf_counter() - t0)
    out.update({"device_s_runs": runs, "device_s": min(runs), **info, "theta_nonzeros": int((T != 0).sum())})
    out["component_sizes_largest5"] = sorted(np.bincount(M.glasso_components(S, RHO)).tolist(), reverse=True)[:5]
    if host:
        t0 = time.perf_counter()
        Wh, Th = M.graphical_lasso(S, RHO)
        out["host_s"] = time.perf_counter() - t0
        out["host_over_device"] = out["host_s"] / out["device_s"]
        out["max_abs_dW"] = float(np.abs(W - Wh).max())
        out["max_abs_dTheta"] = float(np.abs(T - Th).max())
        out["equal_zero_pattern"] = bool(np.array_equal(T != 0, Th != 0))
    if residuals:
        inv, diag, active, inactive, lam = optimality_violations(S, W, T, RHO, True)
        out["residuals"] = {"W_Theta_minus_I": float(inv), "diagonal": float(diag), "active_set": float(active),
                            "inactive_minus_rho": float(inactive), "min_eigenvalue_Theta": float(lam)}
    print(json.dumps(out), flush=True)


def limit(p, host):
    return int(60 + (p / 192.0) ** 3 * 60 * (1 if host else 0) + (p / 2048.0) ** 2 * 840)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--both", default="48,96,192")
    ap.add_argument("--device", default="512,1024,2011")
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--host", type=int, default=0)
    ap.add_argument("--residuals", type=int, default=0)
    args = ap.parse_args()
    if args.one:
        one(args.one, bool(args.host), bool(args.residuals))
        return 0
    both = [int(x) for x in args.both.split(",") if x]
    dev = [int(x) for x in args.device.split(",") if x]
    for p, host in [(p, 1) for p in both] + [(p, 0) for p in dev]:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(p), "--host", str(host), "--residuals", str(int(bool(dev) and p == max(dev) and not host))]
        try:
            rc = subprocess.run(cmd, timeout=limit(p, host)).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"p": p, "error": f"time limit of {limit(p, host)} s"}), flush=True)
            return 124
        if rc != 0:
            print(json.dumps({"p": p, "error": f"exit status {rc}"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
