"""The checkpoint blob of the device sampler (mcd_mh_save / mcd_mh_load, include/mcmcdate_mvn.h; csrc/ckpt_format.hpp) restated in numpy,
and the host trailer that `Sampler.save` appends behind it.

Replaces: what `mcmc` writes with `Settings ... Save` and reloads for `continue` (app/Main.hs:494-509), as far as the host holds it.  The C
blob carries everything the device handle is between two runs; the host side of a `Sampler` adds the generator that shuffles the proposal
cycle and the iteration count, as length-prefixed JSON: TRAILER_MAGIC, a uint64 length, then {"version", "iterations_done", "sched_rng"}.

    parse(blob)      -> {"info": header fields, "meta": the handle's host counters, section name: array}
    checksum(words)  the checksum of 8-byte words, sum_i mix(w_i ^ (i + 1) golden) mod 2^64 with the splitmix64 finaliser
    build(...)       a blob from plain arrays (tests; the library writes its own with the kernels of csrc/k_checkpoint.hip)
"""
from __future__ import annotations

import json
import struct
from typing import Dict, Optional

import numpy as np

MAGIC = 0x0054504B4344434D            # "MCDCKPT\0"
VERSION = 1
FIXED_WORDS = 16
META_WORDS = 48
MAX_SECTIONS = 24
FULL, STATE_TUNING = 0, 1
FLAG_DENSE, FLAG_MC3, FLAG_HAMILTONIAN, FLAG_INV_MASS, FLAG_RECORDER, FLAG_POWER = 1, 2, 4, 8, 16, 32
SECTIONS = {1: "meta", 2: "sc", 3: "heights", 4: "rates", 5: "post", 6: "pcomp", 7: "beta", 8: "tune", 9: "accepted", 10: "tried", 11: "age_sum",
            12: "age_sq", 13: "mc3_rank", 14: "mc3_tried", 15: "mc3_accepted", 16: "ham_sums", 17: "ham_eps", 18: "ham_inv_mass"}
SECTION_IDS = {v: k for k, v in SECTIONS.items()}
# fixed header words and the words of the meta section (csrc/ckpt_format.hpp: CKPT_W_*, CKPT_M_*)
W_MAGIC, W_VERSION_HBYTES, W_TOTAL, W_NSEC_FLAGS, W_NODES_PROPS, W_BATCH, W_DIM_DENSE, W_SEED, W_CHAIN0, W_TOPOLOGY, W_TABLE, W_FINGERPRINT, W_STEP = range(13)
META_FIELDS = ("step", "n_samples", "lik_only", "rec_period", "rec_iter", "rec_fetched", "mc3_chains", "mc3_total", "mc3_seed", "mc3_phase")
M_MC3_LADDER, M_HAM = 10, 26
HAM_FIELDS = ("ham", "ham_depth", "ham_seed", "ham_next", "ham_counted", "ham_inv_mass", "ham_dim")
TRAILER_MAGIC = b"MCDHOST\0"
TRAILER_VERSION = 1

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def _mix(z: np.ndarray) -> np.ndarray:
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def words_of(data) -> np.ndarray:
    """bytes (a multiple of 8) or an array as little-endian uint64 words."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), dtype="<u8")
    return np.ascontiguousarray(data).view(np.uint8).reshape(-1).view("<u8")


def checksum(words) -> int:
    w = words_of(words).astype(np.uint64)
    if w.size == 0:
        return 0
    with np.errstate(over="ignore"):
        i = np.arange(1, w.size + 1, dtype=np.uint64)
        return int(np.sum(_mix(w ^ (i * _GOLDEN)), dtype=np.uint64))


def topology_hash(parent) -> int:
    p = np.asarray(parent, np.int32)
    return checksum(np.concatenate([[p.size], p.view(np.uint32)]).astype(np.uint64))


def table_hash(table: dict) -> int:
    """table: the arrays of sampler.table_arrays."""
    n = len(table["kind"])
    w = np.empty((n, 8), np.uint64)
    for j, f in enumerate(("kind", "node", "n1", "n2", "jac_root", "dim")):
        w[:, j] = np.asarray(table[f], np.int32).view(np.uint32)
    w[:, 6] = np.asarray(table["p0"], np.float64).view(np.uint64)
    w[:, 7] = np.asarray(table["p1"], np.float64).view(np.uint64)
    return checksum(np.concatenate([[np.uint64(n)], w.reshape(-1)]).astype(np.uint64))


def c_bytes(blob: bytes) -> int:
    """Length of the C blob at the start of `blob` (the header's total bytes), whatever follows it."""
    if len(blob) < 8 * (FIXED_WORDS + 1):
        raise ValueError("checkpoint: truncated")
    return int(np.frombuffer(blob[:8 * FIXED_WORDS], "<u8")[W_TOTAL])


def _meta(m: np.ndarray) -> dict:
    meta = {k: int(m[i]) for i, k in enumerate(META_FIELDS)}
    meta["mc3_ladder"] = np.array(m[M_MC3_LADDER:M_MC3_LADDER + 16]).view(np.float64)[:meta["mc3_chains"]]
    meta.update({k: int(m[M_HAM + i]) for i, k in enumerate(HAM_FIELDS)})
    return meta


def meta_of(blob: bytes) -> dict:
    """The "meta" of `parse` alone, for a blob the library has accepted: nothing else is read or summed."""
    at = int(np.frombuffer(blob[8 * (FIXED_WORDS + 1):8 * (FIXED_WORDS + 2)], "<u8")[0])
    return _meta(np.frombuffer(blob[at:at + 8 * META_WORDS], "<u8"))


def parse(blob: bytes) -> Dict[str, object]:
    """The C blob (a host trailer behind it is ignored) as arrays in the shapes of the Sampler's accessors: sc [5, B], heights / rates /
    age_sum / age_sq [B, n_nodes], post [B, 3] (transposed from the blob's [3][B], as Sampler.posterior returns it), pcomp [B, 3], beta [B],
    tune / accepted / tried [B, P], the MC3 and attachment sections where present; "info" and "meta" hold the header's and the meta section's
    fields, "sections" the table as (id, offset, bytes, checksum).  Raises ValueError on a bad header or checksum."""
    blob = bytes(blob)
    total = c_bytes(blob)
    if total > len(blob) or total % 8:
        raise ValueError("checkpoint: truncated")
    w = np.frombuffer(blob[:total], "<u8")
    if int(w[W_MAGIC]) != MAGIC:
        raise ValueError("checkpoint: bad magic")
    version, hbytes = int(w[W_VERSION_HBYTES]) & 0xFFFFFFFF, int(w[W_VERSION_HBYTES]) >> 32
    nsec, flags = int(w[W_NSEC_FLAGS]) & 0xFFFFFFFF, int(w[W_NSEC_FLAGS]) >> 32
    if version != VERSION:
        raise ValueError(f"checkpoint: unknown version {version}")
    hw = FIXED_WORDS + 4 * nsec + 1
    if not 1 <= nsec <= MAX_SECTIONS or hbytes != 8 * hw or total < 8 * hw:
        raise ValueError("checkpoint: bad header")
    if checksum(w[:hw - 1]) != int(w[hw - 1]):
        raise ValueError("checkpoint: the header's checksum does not match")
    n_nodes, n_prop = int(w[W_NODES_PROPS]) & 0xFFFFFFFF, int(w[W_NODES_PROPS]) >> 32
    B = int(w[W_BATCH])
    info = dict(version=version, header_bytes=hbytes, total_bytes=total, n_sections=nsec, flags=flags, n_nodes=n_nodes, n_prop=n_prop, batch=B,
                dim=int(w[W_DIM_DENSE]) & 0xFFFFFFFF, dense=int(w[W_DIM_DENSE]) >> 32, seed=int(w[W_SEED]), chain0=int(w[W_CHAIN0]),
                topology=int(w[W_TOPOLOGY]), table=int(w[W_TABLE]), fingerprint=int(w[W_FINGERPRINT]), step=int(w[W_STEP]))
    out: Dict[str, object] = {"info": info, "sections": []}
    at = 8 * hw
    for s in range(nsec):
        sid, off, nbytes, csum = (int(x) for x in w[FIXED_WORDS + 4 * s:FIXED_WORDS + 4 * s + 4])
        if off != at or nbytes % 8 or off + nbytes > total:
            raise ValueError(f"checkpoint: section {s} leaves the blob")
        at += nbytes
        sec = w[off // 8:(off + nbytes) // 8]
        if checksum(sec) != csum:
            raise ValueError(f"checkpoint: section {s} (id {sid}): checksum mismatch")
        out["sections"].append((sid, off, nbytes, csum))
        out[SECTIONS.get(sid, f"section_{sid}")] = sec
    if at != total:
        raise ValueError("checkpoint: the sections do not fill the blob")
    f64 = lambda a: np.array(a).view(np.float64)
    i32 = lambda a, n: np.array(a).view(np.int32)[:n]
    meta = out["meta"] = _meta(out["meta"])
    out["sc"] = f64(out["sc"]).reshape(5, B)
    for k in ("heights", "rates", "age_sum", "age_sq"):
        out[k] = f64(out[k]).reshape(B, n_nodes)
    out["post"] = f64(out["post"]).reshape(3, B).T.copy()
    out["pcomp"] = f64(out["pcomp"]).reshape(B, 3)
    out["beta"] = f64(out["beta"])
    out["tune"] = f64(out["tune"]).reshape(B, n_prop)
    for k in ("accepted", "tried"):
        out[k] = i32(out[k], B * n_prop).reshape(B, n_prop)
    if "mc3_rank" in out:
        out["mc3_rank"] = i32(out["mc3_rank"], meta["mc3_total"])
        out["mc3_tried"] = np.array(out["mc3_tried"]).view(np.int64)
        out["mc3_accepted"] = np.array(out["mc3_accepted"]).view(np.int64)
    if "ham_sums" in out:
        out["ham_sums"] = np.array(out["ham_sums"]).reshape(4, B)
        out["ham_eps"] = f64(out["ham_eps"])
    if "ham_inv_mass" in out:
        out["ham_inv_mass"] = f64(out["ham_inv_mass"])
    return out


def _pad_i32(a) -> np.ndarray:
    a = np.asarray(a, np.int32).reshape(-1)
    return words_of(np.concatenate([a, np.zeros(a.size % 2, np.int32)]))


def build(parent, table: dict, sc, heights, rates, post, pcomp, beta, tune, accepted, tried, age_sum, age_sq, *, dim: int, dense: bool = True,
          seed: int = 0, chain0: int = 0, step: int = 0, n_samples: int = 0, lik_only: int = 0, recorder: Optional[tuple] = None) -> bytes:
    """A blob as mcd_mh_save writes it for a handle without MC3 and without an attachment, from arrays in the shapes `parse` returns
    (post [B, 3]); recorder = (period, iter, fetched) or None."""
    sc = np.asarray(sc, np.float64)
    B = sc.shape[1]
    n_nodes, n_prop = len(parent), len(table["kind"])
    meta = np.zeros(META_WORDS, np.uint64)
    meta[:3] = (step, n_samples, lik_only)
    if recorder is not None:
        meta[3:6] = recorder
    f = lambda a, shape: words_of(np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape)))
    secs = [(1, meta), (2, f(sc, (5, B))), (3, f(heights, (B, n_nodes))), (4, f(rates, (B, n_nodes))), (5, f(np.asarray(post).T, (3, B))),
            (6, f(pcomp, (B, 3))), (7, f(beta, (B,))), (8, f(tune, (B, n_prop))), (9, _pad_i32(accepted)), (10, _pad_i32(tried)),
            (11, f(age_sum, (B, n_nodes))), (12, f(age_sq, (B, n_nodes)))]
    hw = FIXED_WORDS + 4 * len(secs) + 1
    h = np.zeros(hw, np.uint64)
    flags = (FLAG_DENSE if dense else 0) | (FLAG_RECORDER if recorder is not None else 0) | (FLAG_POWER if lik_only else 0)
    h[W_MAGIC] = MAGIC
    h[W_VERSION_HBYTES] = VERSION | (8 * hw) << 32
    h[W_NSEC_FLAGS] = len(secs) | flags << 32
    h[W_NODES_PROPS] = n_nodes | n_prop << 32
    h[W_BATCH] = B
    h[W_DIM_DENSE] = dim | (1 if dense else 0) << 32
    h[W_SEED], h[W_CHAIN0], h[W_STEP] = seed, chain0, step
    h[W_TOPOLOGY], h[W_TABLE] = topology_hash(parent), table_hash(table)
    h[W_FINGERPRINT] = checksum(h[W_NODES_PROPS:W_FINGERPRINT])
    at = hw
    for s, (sid, w) in enumerate(secs):
        h[FIXED_WORDS + 4 * s:FIXED_WORDS + 4 * s + 4] = (sid, 8 * at, 8 * w.size, checksum(w))
        at += w.size
    h[W_TOTAL] = 8 * at
    h[hw - 1] = checksum(h[:hw - 1])
    return b"".join([h.astype("<u8").tobytes()] + [np.asarray(w, "<u8").tobytes() for _, w in secs])


def save_size(B: int, n_nodes: int, P: int) -> int:
    """Bytes of the blob of a handle without MC3 and without an attachment: 12 sections."""
    return 8 * (FIXED_WORDS + 4 * 12 + 1) + 8 * META_WORDS + 8 * (12 * B + 4 * B * n_nodes + B * P + 2 * ((B * P + 1) // 2))


# ---- the host trailer ----------------------------------------------------------------------------------------------------------------
def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, np.ndarray):
        return {"__ndarray__": x.tolist(), "dtype": str(x.dtype)}
    if isinstance(x, (np.integer,)):
        return int(x)
    return x


def _unplain(x):
    if isinstance(x, dict):
        if "__ndarray__" in x:
            return np.array(x["__ndarray__"], dtype=x["dtype"])
        return {k: _unplain(v) for k, v in x.items()}
    return x


def trailer(rng: np.random.Generator, iterations_done: int) -> bytes:
    body = json.dumps({"version": TRAILER_VERSION, "iterations_done": int(iterations_done), "sched_rng": _plain(rng.bit_generator.state)}).encode()
    return TRAILER_MAGIC + struct.pack("<Q", len(body)) + body


def read_trailer(data: bytes) -> dict:
    """{"iterations_done", "sched_rng" (a bit generator state as numpy takes it)} of the bytes behind the C blob."""
    if len(data) < 16 or data[:8] != TRAILER_MAGIC:
        raise ValueError("checkpoint: no host trailer behind the device blob")
    (n,) = struct.unpack("<Q", data[8:16])
    if len(data) != 16 + n:
        raise ValueError("checkpoint: the host trailer is truncated")
    t = json.loads(data[16:].decode())
    if t.get("version") != TRAILER_VERSION:
        raise ValueError(f"checkpoint: unknown host trailer version {t.get('version')}")
    return {"iterations_done": int(t["iterations_done"]), "sched_rng": _unplain(t["sched_rng"])}
