"""Per-wave times of the headline launch's stripe kernel (k_logpdf_stripe: N = 256, 512 chains by default), from the s_memtime stamps
every stripe wave of workgroup 0 keeps per launch (library: `make -C mcmc-date_amd/csrc stamp_headline` ->
tools/microbench/libheadlinestamp.so; STAMPLIB names another file beside it, such as a build with another number of stripe waves).
The harness is headline_phases.py's: graphs of 100 launches alternating two input batches, replayed back to back; the last 64
launches are kept.  Milestones of a wave: 0 entry, 1 its loads of x / mu / 1/diag landed (behind the issue of the prologue's LDS-DMAs),
5 exchange barrier passed and r read (the shared prologue only; MCD_STRIPE_PROLOGUE=0 in the environment: the private one), 2 first
unit landed, 3 last unit applied, and on wave 0: 4 ll stored.  Under the per-chain finish (MCD_STRIPE_FINISH unset or 1) both
finishing waves stamp 6 hand-over barrier passed, 7 hand-over read and 4 ll stored; a stamp the second finishing wave takes after wave 0
has closed the launch's slot lands in the next slot and is dropped here (counted in "of").  A wave's stream rate is its units x 1024 bytes over 2 -> 3; the CU's is the
whole stream over (first wave's 2) -> (last wave's 3), and over entry -> (last wave's 3).

usage: python tools/microbench/headline_stripes.py [N [chains [waves]]]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
os.environ["MCD_LIB_PATH"] = os.path.join(HERE, os.environ.get("STAMPLIB", "libheadlinestamp.so"))
import mcmc_date_amd as M  # noqa: E402
from mcmc_date_amd import synthetic as S  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
B = int(sys.argv[2]) if len(sys.argv) > 2 else 512
NW = int(sys.argv[3]) if len(sys.argv) > 3 else 4
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
nl = C.c_uint(0)
L.mcd_debug_hist.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint)]
assert L.mcd_debug_hist(hist.ctypes.data, span.ctypes.data, C.byref(nl)) == 0
H = hist.astype(np.int64)[:, :NW, :]
R = (n + 63) // 64
total = {3: 144, 4: 256}[R]
e = H[:, 0:1, 0]
t = H - e[:, :, None]                                                          # ticks since wave 0's entry
ok = (t[:, :, 1:4] > 0).all(axis=(1, 2)) & (t[:, :, 1:4] < 100000).all(axis=(1, 2)) & (np.diff(t[:, :, 0:4], axis=2) >= 0).all(axis=(1, 2))
t = t[ok]
shared = bool((H[ok][:, :, 5] != 0).all())                                     # milestone 5 is stamped by the shared prologue only
print(f"N = {n}, {B} chains, {NW} stripe waves: {len(t)} launches; ticks after wave 0's entry, median (min .. max)")
for w in range(NW):
    def m(i):
        return f"{np.median(t[:, w, i]):6.0f} ({t[:, w, i].min():6d} .. {t[:, w, i].max():6d})"
    print(f"  wave {w}: entry {m(0)}  loads landed {m(1)}  " + (f"barrier passed, r read {m(5)}  " if shared else "") +
          f"first unit landed {m(2)}  last unit applied {m(3)}  first -> last {np.median(t[:, w, 3] - t[:, w, 2]):6.0f}")
for w in range(NW):                                                            # the finishing waves (milestone 6: the per-chain finish only)
    good = (t[:, w, 6] > t[:, w, 3]) & (t[:, w, 7] >= t[:, w, 6]) & (t[:, w, 4] >= t[:, w, 7]) & (t[:, w, 4] < 100000)
    if good.any():
        f = t[good]
        print(f"  wave {w} finishes ({good.sum()} of {len(t)}): barrier passed {np.median(f[:, w, 6]):6.0f}  hand-over read {np.median(f[:, w, 7]):6.0f}  "
              f"ll stored {np.median(f[:, w, 4]):6.0f}  last unit applied -> ll stored {np.median(f[:, w, 4] - f[:, w, 3]):6.0f}  "
              f"workgroup's last unit -> ll stored {np.median(f[:, w, 4] - f[:, :, 3].max(axis=1)):6.0f}")
first, last = t[:, :, 2].min(axis=1), t[:, :, 3].max(axis=1)
print(f"  workgroup: first unit landed {np.median(first):6.0f}, last unit applied {np.median(last):6.0f}, ll stored {np.median(t[:, 0, 4]):6.0f}")
print(f"  stream: {total} units; {total * 1024 / np.median(last - first):5.1f} B/clk first landed -> last applied, "
      f"{total * 1024 / np.median(last):5.1f} B/clk entry -> last applied")
