"""The compact forward factor stream of the column sweep (csrc/fc_layout.hpp, host_factor.cpp: pack_compact_forward) is host
code: the library packs a random factor both ways, unpacks the compact stream chunk by chunk as the sweep reads it and compares
every element with the padded stream and the dense scaled factor.  No GPU involved."""
import ctypes as C

import mcmc_date_amd as M


def expected_units(n):
    """Units (1 KiB: 64 lanes x 2 columns) of the compact stream, from the layout's definition."""
    R = next(a for a in (1, 2, 3, 4, 6, 8, 12, 16) if (n + 63) // 64 <= a)
    CP = {1: 32, 2: 16, 3: 8, 4: 8, 6: 4, 8: 4}.get(R, 4)
    total = 0
    for jb in range(R):
        for lc in range(32 // CP):
            diag = sum(63 - 2 * (lc * CP + p) for p in range(CP))        # nonzero lanes of the chunk's diagonal units
            total += -(-diag // 64) + CP * (R - 1 - jb)
    return total


def test_compact_stream_round_trip():
    L = C.CDLL(M._capi.LIB_PATH)
    f = L.mcd_compact_stream_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_uint]
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 192, 255, 256, 320, 512):
        got = f(n, 11 * n + 1)
        assert got == expected_units(n), (n, got, expected_units(n))
    assert expected_units(256) == 256                                      # the triangle: 320 units padded
