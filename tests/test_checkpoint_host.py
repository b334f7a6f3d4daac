"""CPU tests of the checkpoint format: the pure-host entry points mcd_ckpt_inspect and mcd_ckpt_checksum through ctypes (the library loads
without a device), against the numpy restatement mcmc_date_amd.checkpoint, and the host trailer of Sampler.save."""
import ctypes as C

import numpy as np
import pytest

import mcmc_date_amd as M
from mcmc_date_amd import _capi, checkpoint as K, synthetic as S

INVALID = _capi.MCD_ERR_INVALID_ARG


def c_checksum(words: np.ndarray) -> int:
    w = np.ascontiguousarray(words, "<u8")
    return int(_capi.lib().mcd_ckpt_checksum(w.ctypes.data_as(C.c_void_p), w.size))


def a_blob(B=3, leaves=6, seed=1, odd_counters=True):
    """A blob of checkpoint.build over random arrays: (blob, the arguments it was built from)."""
    rng = np.random.default_rng(seed)
    topo = S.random_topology(leaves, seed=seed)
    n = topo.n_nodes
    ps, _ = M.proposals(topo, [], calibrations_available=True)
    if odd_counters and (B * len(ps)) % 2 == 0:
        ps = ps[:-1]                                                     # (an odd number of int32 counters: the padded half word)
    tab = M.table_arrays(ps)
    Pn = len(ps)
    a = dict(sc=rng.random((5, B)), heights=rng.random((B, n)), rates=rng.random((B, n)), post=rng.standard_normal((B, 3)), pcomp=rng.standard_normal((B, 3)),
             beta=rng.random(B), tune=rng.random((B, Pn)) + 0.5, accepted=rng.integers(0, 1 << 30, (B, Pn), dtype=np.int32),
             tried=rng.integers(0, 1 << 31, (B, Pn), dtype=np.int32, endpoint=False), age_sum=rng.random((B, n)), age_sq=rng.random((B, n)))
    kw = dict(dim=n - 2, dense=True, seed=(1 << 63) + 12345, chain0=7, step=(1 << 40) + 3, n_samples=17, lik_only=1, recorder=(3, 10, 3))
    return K.build(topo.parent, tab, **a, **kw), dict(parent=topo.parent, table=tab, **a, **kw)


def test_checksum_agrees_with_numpy():
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 63, 64, 65, 2048, 5000):
        w = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        assert c_checksum(w) == K.checksum(w), n
    assert c_checksum(np.zeros(0, np.uint64)) == 0
    one = np.array([0x0123456789ABCDEF], np.uint64)
    z = int(one[0]) ^ 0x9E3779B97F4A7C15                                 # the definition, on Python integers
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    assert c_checksum(one) == z ^ (z >> 31)
    w = rng.integers(0, 1 << 64, 100, dtype=np.uint64)                   # position matters: a swap of two words changes the sum
    v = w.copy()
    v[[3, 4]] = v[[4, 3]]
    assert c_checksum(w) != c_checksum(v)


def test_inspect_reads_what_build_wrote():
    blob, a = a_blob()
    info = _capi.ckpt_inspect(blob)
    B, n, Pn = a["sc"].shape[1], len(a["parent"]), len(a["table"]["kind"])
    assert (info.version, info.n_sections, info.total_bytes, info.header_bytes) == (K.VERSION, 12, len(blob), 8 * (K.FIXED_WORDS + 4 * 12 + 1))
    assert len(blob) == K.save_size(B, n, Pn) and (B * Pn) % 2 == 1
    assert (info.n_nodes, info.n_prop, info.batch, info.dim, info.dense, info.seed, info.chain0, info.step) == (n, Pn, B, n - 2, 1, a["seed"], 7, a["step"])
    assert info.flags == K.FLAG_DENSE | K.FLAG_RECORDER | K.FLAG_POWER
    assert info.topology == K.topology_hash(a["parent"]) and info.table == K.table_hash(a["table"])
    words = np.frombuffer(blob, "<u8")
    at = info.header_bytes
    for s in range(info.n_sections):
        assert info.section_id[s] == s + 1 and info.section_offset[s] == at and info.section_bytes[s] % 8 == 0
        sec = words[at // 8:(at + info.section_bytes[s]) // 8]
        assert info.section_checksum[s] == K.checksum(sec) == c_checksum(sec)
        at += info.section_bytes[s]
    assert at == len(blob)
    p = K.parse(blob + b"anything behind the blob")
    for k in ("sc", "heights", "rates", "post", "pcomp", "beta", "tune", "accepted", "tried", "age_sum", "age_sq"):
        assert np.array_equal(p[k], a[k]), k
    m = p["meta"]
    assert (m["step"], m["n_samples"], m["lik_only"], m["rec_period"], m["rec_iter"], m["rec_fetched"], m["mc3_chains"], m["ham"]) == (a["step"], 17, 1, 3, 10, 3, 0, 0)
    # a changed configuration changes its hash and the fingerprint
    other, _ = a_blob(seed=2)
    assert _capi.ckpt_inspect(other).topology != info.topology and _capi.ckpt_inspect(other).fingerprint != info.fingerprint


def _refused(blob, match):
    with pytest.raises(M.McdError, match=match) as e:
        _capi.ckpt_inspect(blob)
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        K.parse(blob)


def test_inspect_refuses_damaged_blobs():
    blob, _ = a_blob()
    info = _capi.ckpt_inspect(blob)
    _refused(blob[:-8], "truncated")
    _refused(blob[:100], "truncated")
    _refused(blob[:0] + b"", "truncated")
    x = bytearray(blob)
    x[0] ^= 1
    _refused(bytes(x), "bad magic")
    x = bytearray(blob)
    x[8:12] = (K.VERSION + 1).to_bytes(4, "little")
    _refused(bytes(x), "unknown version 2")
    for byte in (8 * K.W_SEED, 8 * K.W_BATCH + 1, 8 * K.FIXED_WORDS + 8, info.header_bytes - 1):      # fixed words, the table, the header's own sum
        x = bytearray(blob)
        x[byte] ^= 0x10
        _refused(bytes(x), "header's checksum")
    for s in (0, 3, 11):                                                  # a bit in the counters, in a payload section, in the last byte
        x = bytearray(blob)
        x[info.section_offset[s] + info.section_bytes[s] - 1] ^= 0x80
        _refused(bytes(x), "checksum does not match its bytes")
    with pytest.raises(M.McdError, match="truncated"):
        _capi.ckpt_inspect(blob + b"\0" * 8)                              # len must be the blob's total bytes exactly


def test_trailer_round_trips_the_schedule_generator():
    topo = S.random_topology(6, seed=1)
    ps, _ = M.proposals(topo, [])
    rng = np.random.default_rng([13, 0x5EED])
    M.cycle_schedule(ps, 3, rng)                                          # (a generator in mid-stream)
    t = K.trailer(rng, 41)
    back = K.read_trailer(t)
    assert back["iterations_done"] == 41
    other = np.random.default_rng(0)
    other.bit_generator.state = back["sched_rng"]
    assert np.array_equal(M.cycle_schedule(ps, 4, other), M.cycle_schedule(ps, 4, rng))
    for bad in (t[:-1], b"x" + t[1:], t + b"0", b""):
        with pytest.raises(ValueError):
            K.read_trailer(bad)
