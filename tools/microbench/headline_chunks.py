"""Per-chunk times of the headline launch's column phase (N = 256, 512 chains by default), from the stamp behind every chunk's barrier
on compute wave 0 of workgroup 0 (library: `make -C mcmc-date_amd/csrc stamp_headline_chunks` -> tools/microbench/libheadlinechunks.so).
The harness is headline_phases.py's: graphs of 100 launches alternating two input batches, replayed back to back; the last 64 launches
are kept.  Chunk ci's time is barrier(ci) - barrier(ci - 1), chunk 0's counts from the first barrier.  Units per chunk (1 KiB each)
are printed beside it: a chunk bound by the CU's ingest costs about units x 1024 / 28 ticks.

usage: python tools/microbench/headline_chunks.py [N [chains]]      (MCD_FSTREAM=2 in the environment: the substitution stream)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
os.environ["MCD_LIB_PATH"] = os.path.join(HERE, "libheadlinechunks.so")
import mcmc_date_amd as M  # noqa: E402
from mcmc_date_amd import synthetic as S  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
B = int(sys.argv[2]) if len(sys.argv) > 2 else 512
dev = torch.device("cuda", 0)
mu, sigma = S.random_spd_problem(n, seed=n)
lik = M.MvnLikelihood.from_covariance(mu, sigma, device=0)
X = [torch.as_tensor(S.sample_chains(mu, sigma, B, seed=n + 500 * i), device=dev) for i in range(2)]
ll = [torch.empty(B, dtype=torch.float64, device=dev) for _ in range(2)]
st = torch.cuda.Stream(device=dev)
with torch.cuda.stream(st):
    lik.logpdf_into(X[0], ll[0])
st.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g, stream=st):
    for i in range(100):
        lik.logpdf_into(X[i & 1], ll[i & 1])
for _ in range(50):
    g.replay()
torch.cuda.synchronize()

L = M._capi.lib()
hist = np.zeros((64, 8, 8), np.uint64)
span = np.zeros((64, 64, 2), np.uint64)
chunk = np.zeros((64, 16), np.uint64)
nl = C.c_uint(0)
L.mcd_debug_hist.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint)]
L.mcd_debug_chunks.argtypes = [C.c_void_p]
assert L.mcd_debug_hist(hist.ctypes.data, span.ctypes.data, C.byref(nl)) == 0 and L.mcd_debug_chunks(chunk.ctypes.data) == 0
hist, chunk = hist.astype(np.int64), chunk.astype(np.int64)
R = (n + 63) // 64
nchunk = (n + 15) // 16
diag = (7, 5, 3, 1)
units = [diag[ci % 4] + 8 * (R - 1 - ci // 4) for ci in range(nchunk)]
block = [ci // 4 for ci in range(nchunk)]
fs = int(os.environ.get("MCD_FSTREAM", "3" if (240 < n <= 256 and 128 < B <= 512) else "2"))
t = np.concatenate([hist[:, 0, 2:3], chunk[:, :nchunk]], axis=1)             # first barrier, then the barrier behind every chunk
d = np.diff(t, axis=1)
ok = (d > 0).all(axis=1) & (d < 100000).all(axis=1)                           # a launch whose slots hold one launch's stamps
d = d[ok]
print(f"N = {n}, {B} chains, stream {fs}: {len(d)} launches; ticks per chunk, median (min .. max), units, units x 1024 / 28")
for ci in range(nchunk):
    print(f"  chunk {ci:2d} (block {block[ci]}): {np.median(d[:, ci]):7.0f} ({d[:, ci].min():6d} .. {d[:, ci].max():6d})   {units[ci]:2d} units  {units[ci] * 1024 / 28:6.0f}")
for jb in range(R):
    cs = [c for c in range(nchunk) if block[c] == jb]
    print(f"  block {jb}: {np.median(d[:, cs].sum(axis=1)):7.0f} ticks, {sum(units[c] for c in cs)} units")
print(f"  column phase (first barrier -> last): {np.median(d.sum(axis=1)):7.0f} ticks; sweep milestone {np.median(hist[ok, 0, 3] - hist[ok, 0, 2]):7.0f}")
