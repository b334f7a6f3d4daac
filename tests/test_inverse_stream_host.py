"""The inverse factor stream Fw of the column sweep (csrc/host_factor.cpp: pack_inverse_forward) is host code: the strictly lower
triangle of W = L^-1 in the compact layout of csrc/fc_layout.hpp, unscaled, zeros on and above the diagonal.  Here the library packs
a random lower-triangular W and the test finds every entry where the layout's arithmetic -- written out again below -- puts the
matching entry of the substitution stream Fc.  Also the device-free choice of stream (sweep_launch.cpp) at the edges of the window in
which the inverse stream is the default.  No GPU involved."""
import ctypes as C

import numpy as np
import pytest

import mcmc_date_amd as M

CP, CPB = 8, 4                                   # fc_layout.hpp at R = 3, 4: column pairs per chunk, chunks per 64-column block


def diag_start(lc, p):
    return p * (64 - 2 * lc * CP - p)


def diag_units(lc):
    return (diag_start(lc, CP) + 63) // 64


def chunk_units(R, ci):
    return diag_units(ci % CPB) + CP * (R - 1 - ci // CPB)


def chunk_base(R, ci):
    return sum(chunk_units(R, c) for c in range(ci))


def position(R, i, j):
    """index (in doubles) of element (row i, column j), j < i, in a compact stream"""
    k, lane, JB, pl, h = i // 64, i % 64, j // 64, (j % 64) // 2, j & 1
    lc, p = pl // CP, pl % CP
    base = chunk_base(R, JB * CPB + lc)
    if k == JB:
        assert lane > 2 * pl
        return 2 * (64 * base + diag_start(lc, p) - (2 * pl + 1) + lane) + h
    return 2 * (64 * (base + diag_units(lc) + p * (R - 1 - JB) + (k - JB - 1)) + lane) + h


def library():
    L = C.CDLL(M._capi.LIB_PATH)
    L.mcd_inverse_stream_pack_.restype = C.c_int
    L.mcd_inverse_stream_pack_.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mcd_stream_selftest_.restype = C.c_int
    L.mcd_stream_selftest_.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64]
    return L


@pytest.mark.parametrize("n", [129, 200, 256])
def test_inverse_stream_layout(n):
    L = library()
    R = (n + 63) // 64
    total = chunk_base(R, R * CPB)
    assert total == {3: 144, 4: 256}[R]                    # 16 diagonal units per block + 32 per block pair below
    rng = np.random.default_rng(n)
    W = np.tril(rng.uniform(0.5, 1.5, (n, n)) * rng.choice([-1.0, 1.0], (n, n)))       # no entry of the triangle is zero
    Fw = np.full(total * 128 + 7, np.nan)                                              # (a guard behind the stream)
    Fc = np.full(total * 128 + 7, np.nan)
    got = L.mcd_inverse_stream_pack_(n, W.ctypes.data, Fw.ctypes.data, Fc.ctypes.data)
    assert got == total                                                                 # fc_total_units(R)
    assert np.isnan(Fw[total * 128:]).all() and np.isnan(Fc[total * 128:]).all()
    Fw, Fc = Fw[: total * 128], Fc[: total * 128]
    # the same bytes as pack_compact_forward makes of a padded stream built from the same matrix
    assert np.array_equal(Fw, Fc)
    ii, jj = np.tril_indices(n, -1)
    pos = np.array([position(R, i, j) for i, j in zip(ii, jj)])
    assert len(np.unique(pos)) == len(pos) and pos.max() < Fw.size
    assert np.array_equal(Fw[pos], W[ii, jj])                                           # unscaled
    rest = np.ones(Fw.size, dtype=bool)
    rest[pos] = False
    assert not Fw[rest].any()                                                           # the diagonal, everything above it, the padding


def test_inverse_stream_refused_elsewhere():
    L = library()
    W = np.eye(64)
    out = np.zeros(8)
    assert L.mcd_inverse_stream_pack_(64, W.ctypes.data, out.ctypes.data, out.ctypes.data) < 0       # R = 1: no compact stream
    W = np.eye(300)
    assert L.mcd_inverse_stream_pack_(300, W.ctypes.data, out.ctypes.data, out.ctypes.data) < 0      # R = 6


def test_stream_choice(knobs):
    """mcd_stream_selftest_(n, R, form, split tables exist, multiply tiles exist, batch): the forward stream a raw-x log-density
    call takes, -1 where the column sweep does not serve it"""
    f = library().mcd_stream_selftest_
    AUTO, SWEEP, MULT = 0, 1, 2

    def auto(n, batch):
        return f(n, (n + 63) // 64, AUTO, 1, 1, batch)

    # the window: 240 < N <= 256, 128 < batch <= 512, form auto
    assert [auto(n, 512) for n in (240, 241, 255, 256)] == [2, 3, 3, 3]
    assert [auto(256, b) for b in (128, 129, 130, 256, 512, 513)] == [-1, 3, 3, 3, 3, 0]       # (up to 128 chains: the row split)
    assert [auto(241, b) for b in (128, 129, 512, 513)] == [-1, 3, 3, 0]
    assert auto(257, 512) == -1 and auto(200, 256) == 2 and auto(129, 512) == 2 and auto(128, 512) == 0
    assert auto(256, 2048) == -1                                                               # the multiply form
    # a handle without the row-split tables keeps the sweep below the window, on the substitution stream
    assert f(256, 4, AUTO, 0, 1, 128) == 2 and f(256, 4, AUTO, 0, 1, 129) == 3
    # form "sweep" keeps substitution everywhere; "multiply" is no sweep where its tiles exist
    assert [f(256, 4, SWEEP, 1, 1, b) for b in (1, 128, 129, 512, 513)] == [2, 2, 2, 2, 0]
    assert f(256, 4, MULT, 1, 1, 512) == -1 and f(256, 4, MULT, 1, 0, 512) == 2
    # MCD_SPLIT = 1 wins over the new stream; MCD_SPLIT = 0 leaves the window as it is
    knobs.setenv("MCD_SPLIT", "1")
    assert auto(256, 512) == -1 and auto(241, 129) == -1
    knobs.setenv("MCD_SPLIT", "0")
    assert auto(256, 512) == 3 and auto(256, 128) == 2
    knobs.delenv("MCD_SPLIT")
    # the knob: 3 selects the stream in the two-compute-wave geometry at R = 3, 4 under any form, elsewhere that geometry's default
    knobs.setenv("MCD_FSTREAM", "3")
    assert [f(n, (n + 63) // 64, SWEEP, 1, 1, 5) for n in (129, 140, 200, 241, 255, 256)] == [3] * 6
    assert f(256, 4, SWEEP, 1, 1, 513) == 0 and f(200, 4, AUTO, 1, 1, 600) == 0                # four compute waves
    assert f(128, 2, SWEEP, 1, 1, 5) == 0 and f(300, 6, SWEEP, 1, 1, 5) == 0                   # no compact stream at this R
    assert auto(256, 128) == -1                                                                # (the row split still takes its batches)
    for fs in (0, 1, 2):
        knobs.setenv("MCD_FSTREAM", str(fs))
        assert auto(256, 512) == fs and f(256, 4, SWEEP, 1, 1, 512) == fs
    knobs.delenv("MCD_FSTREAM")
    assert auto(256, 512) == 3
