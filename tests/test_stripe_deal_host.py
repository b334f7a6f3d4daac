"""The deal of the inverse stream Fw to the stripe waves of the raw-x log-density kernel (csrc/stripe_deal.hpp) is constexpr arithmetic
shared by the host and the device.  mcd_stripe_deal_selftest_ returns a wave's list of pieces; here it is checked against the layout
of csrc/fc_layout.hpp, written out again below: every unit has one owner, pieces are whole, the shares are even, a list is in
ascending column order, and a sweep that stops early keeps exactly the chunks in front of the cut.  No GPU involved."""
import ctypes as C

import numpy as np
import pytest

import mcmc_date_amd as M

CP, CPB = 8, 4                                   # fc_layout.hpp at R = 3, 4: column pairs per chunk, chunks per 64-column block


def diag_units(lc):
    return (CP * (64 - 2 * lc * CP - CP) + 63) // 64


def chunk_units(R, ci):
    return diag_units(ci % CPB) + CP * (R - 1 - ci // CPB)


def chunk_base(R, ci):
    return sum(chunk_units(R, c) for c in range(ci))


def pieces(R, S, w, ncols):
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_deal_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    out = np.full((160, 5), -7, dtype=np.int32)
    n = f(R, S, w, ncols, out.ctypes.data, len(out))
    assert 0 <= n <= len(out)
    assert (out[n:] == -7).all()
    return [tuple(int(v) for v in row) for row in out[:n]]


@pytest.mark.parametrize("R,S", [(3, 4), (3, 8), (4, 4), (4, 8)])
def test_stripe_deal(R, S):
    total = chunk_base(R, R * CPB)
    assert total == {3: 144, 4: 256}[R]
    owner = np.full(total, -1)
    counts = []
    for w in range(S):
        ps = pieces(R, S, w, 64 * R)
        pos = 0
        cols = []
        for ci, p, first, units, at in ps:
            JB, lc = ci // CPB, ci % CPB
            base = chunk_base(R, ci)
            if p < 0:                                                    # the chunk's diagonal part, whole
                assert (first, units) == (base, diag_units(lc))
                cols.append(16 * ci)
            else:                                                        # the off-diagonal units of one column pair, whole
                assert 0 <= p < CP and units == R - 1 - JB and units > 0
                assert first == base + diag_units(lc) + p * units
                assert (ci * CP + p) % S == w
                cols.append(16 * ci + 2 * p)
            assert at == pos                                             # the list is packed: unit u of the list is ring slot u mod D
            assert (owner[first:first + units] == -1).all()
            owner[first:first + units] = w
            pos += units
        # ascending column order, a chunk's diagonal part in front of its pairs
        keys = [(c, 0 if p < 0 else 1) for c, (_, p, _, _, _) in zip(cols, ps)]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        counts.append(pos)
    assert (owner >= 0).all()                                            # every unit owned, exactly once (asserted above)
    assert sum(counts) == total
    if R == 4:
        assert counts == [256 // S] * S
    else:
        mean = total / S
        assert max(counts) - min(counts) <= mean / 4, counts
    # the bad arguments
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_deal_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    buf = np.zeros((4, 5), dtype=np.int32)
    assert f(R, S, S, 64 * R, buf.ctypes.data, 4) == -1 and f(2, S, 0, 128, buf.ctypes.data, 4) == -1
    assert f(R, 5, 0, 64 * R, buf.ctypes.data, 4) == -1 and f(R, S, 0, 64 * R, buf.ctypes.data, 4) == -2


@pytest.mark.parametrize("R,S,ncols", [(R, S, nc) for R in (3, 4) for S in (4, 8) for nc in (129, 144, 192, 241, 256) if nc <= 64 * R])
def test_stripe_deal_early_stop(R, S, ncols):
    kept = set()
    for w in range(S):
        full = pieces(R, S, w, 64 * R)
        cut = pieces(R, S, w, ncols)
        assert cut == full[:len(cut)]                                    # a suffix of the wave's list goes
        assert all(16 * ci < ncols for ci, *_ in cut) and all(16 * ci >= ncols for ci, *_ in full[len(cut):])
        for ci, p, first, units, at in cut:
            kept.update(range(first, first + units))
    nchunk = sum(1 for ci in range(R * CPB) if 16 * ci < ncols)
    assert kept == set(range(chunk_base(R, nchunk)))                     # exactly the units of the chunks with 16 CI < ncols
