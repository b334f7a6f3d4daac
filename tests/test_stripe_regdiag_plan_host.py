"""The plan of a stripe wave of k_logpdf_stripe_reg (csrc/stripe_plan.hpp: stripe_reg_plan, MCD_STRIPE_DIAG = 1), where the diagonal
parts of the inverse stream arrive by register load too: a list position is a request, a part contributes eight, one per column pair,
whose lanes above the pair's threshold read the part with a lane shift folded into the address and whose other lanes read a unit of
zeros behind the stream.  mcd_stripe_regplan_selftest_ returns a wave's plan, every lane's vector offset and the verdict of the library's
own replay; here the plan is replayed once more with a queue that retires in issue order, and every diagonal request's lanes are set
against the layout computed here from its definition (csrc/fc_layout.hpp), not from the plan.  Then the host's choice of kernel
(stripe_diag, the function the launcher calls) under every value of the four stripe options.  tests/cpp/test_stripe_plan_reg.cpp, the
same header without the library, is compiled and run too.  No GPU involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mcmc_date_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTAL = {3: 144, 4: 256}                         # units of the stream
LOOKAHEADS = (10, 11, 12, 13, 14, 15, 16)
CP = 8                                           # column pairs per chunk at R = 3, 4; four chunks per 64-column block


def diag_start(lc, p):
    """16-byte lanes of a chunk's diagonal part in front of pair p: pair q keeps lanes 2 (8 lc + q) + 1 .. 63"""
    return sum(63 - 2 * (8 * lc + q) for q in range(p))


def diag_units(lc):
    return (diag_start(lc, CP) + 63) // 64


def layout(R):
    """chunk -> (first unit, units of its diagonal part, row blocks below the diagonal), in stream order"""
    out, at = [], 0
    for ci in range(4 * R):
        du, nko = diag_units(ci % 4), R - 1 - ci // 4
        out.append((at, du, nko))
        at += du + CP * nko
    assert at == TOTAL[R]
    return out


def plan(R, S, w, A):
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_regplan_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    head = np.full(7, -7, dtype=np.int32)
    pos = np.full((96, 8), -7, dtype=np.int32)
    grp = np.full((32, 7), -7, dtype=np.int32)
    lanes = np.zeros((96, 64), dtype=np.uint32)
    verdict = f(R, S, w, A, head.ctypes.data, pos.ctypes.data, len(pos), grp.ctypes.data, len(grp), lanes.ctypes.data)
    n, ng = int(head[0]), int(head[1])
    assert 0 < n <= len(pos) and 0 < ng <= len(grp)
    assert (pos[n:] == -7).all() and (grp[ng:] == -7).all()
    return verdict, [int(v) for v in head], pos[:n].tolist(), grp[:ng].tolist(), lanes[:n].astype(np.int64)


def replay(head, pos, grp):
    """the wave's requests in its order of events; returns the most operations outstanding"""
    n, ng, lead, pro, slots = head[:5]
    queue = [-1] * lead                                                  # -1: a leading load of the prologue
    landed, applied, reg = set(), set(), {}
    issued, most = 0, lead

    def issue(upto):
        nonlocal issued, most
        assert issued <= upto <= n
        for u in range(issued, upto):
            slot, base, imm = pos[u][:3]
            assert 0 <= slot < slots and -4096 <= imm <= 4095 and base >= 0
            assert slot not in reg or pos[reg[slot]][7] in applied, ("register slot taken before its group was multiplied", u)
            reg[slot] = u
            queue.append(u)
            most = max(most, len(queue))
        issued = upto

    def wait(count):
        while len(queue) > count:
            landed.add(queue.pop(0))

    issue(pro)
    wait(pro)
    assert -1 not in queue                                               # the prologue's loads have returned
    at = 0
    for g, (ci, diag, beg, end, pre, vmcnt, post) in enumerate(grp):
        assert beg == at and end > beg and end - beg <= slots            # the groups tile the list in order; a group fits the ring
        assert all(pos[u][7] == g for u in range(beg, end))
        at = end
        if g:
            applied.add(g - 1)                                           # the multiply-adds of the group before, then ...
        issue(pre)
        wait(vmcnt)
        assert all(u in landed for u in range(beg, end)), ("a request used before it landed", g)
        assert len(queue) == vmcnt and (not queue or queue[0] == end), ("the wait covers more than the group", g)
        issue(post)
    assert at == n == issued
    return most


@pytest.mark.parametrize("R,S", [(3, 4), (3, 8), (4, 4), (4, 8)])
@pytest.mark.parametrize("A", LOOKAHEADS)
def test_regdiag_plan(R, S, A):
    chunks = layout(R)
    zero = 1024 * TOTAL[R]
    units = np.zeros(TOTAL[R], dtype=int)
    pairs = np.zeros((4 * R, CP), dtype=int)
    for w in range(S):
        verdict, head, pos, grp, lanes = plan(R, S, w, A)
        assert verdict == 0, (w, verdict)
        assert head[5] == A and head[3] == min(A, head[0]) and head[6] == zero
        assert replay(head, pos, grp) < 64, w
        lane = np.arange(64)
        for u, (slot, base, imm, thr, zoff, unit, pair, g) in enumerate(pos):
            ci, diag = grp[g][0], grp[g][1]
            at = base + imm + lanes[u]                                   # the bytes of Fw each lane reads, 16 from there on
            if not diag:
                assert thr == -1 and pair == -1
                assert np.array_equal(at, 1024 * unit + 16 * lane), (w, u)
                first, du, nko = chunks[ci]
                assert first + du <= unit < first + du + CP * nko         # an off-diagonal unit of the group's chunk
                units[unit] += 1
                continue
            first, du, _ = chunks[ci]
            lc, pl = ci % 4, 8 * (ci % 4) + pair
            assert unit == first and thr == 2 * pl and pair == u - grp[g][2]
            pairs[ci, pair] += 1
            valid = lane > 2 * pl
            # lane l > 2 pl of the pair's diagonal unit is lane diag_start + l - (2 pl + 1) of the part
            want = 1024 * first + 16 * (diag_start(lc, pair) + lane - (2 * pl + 1))
            assert np.array_equal(at[valid], want[valid]), (w, u)
            assert (at[valid] >= 1024 * first).all() and (at[valid] + 16 <= 1024 * (first + du)).all()
            assert (at[~valid] == zero).all(), (w, u)                    # zeros from memory: the zero unit's first 16 bytes
            assert (lanes[u] >= 0).all() and zoff >= 0
    for ci, (first, du, nko) in enumerate(chunks):
        assert (units[first:first + du] == 0).all() and (units[first + du:first + du + CP * nko] == 1).all()
    assert (pairs == 1).all()                                            # every (part, pair) exactly once across the waves


def test_regdiag_plan_refuses():
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_regplan_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    head = np.zeros(7, dtype=np.int32)
    pos = np.zeros((96, 8), dtype=np.int32)
    grp = np.zeros((32, 7), dtype=np.int32)
    args = (head.ctypes.data, pos.ctypes.data, 96, grp.ctypes.data, 32, None)
    assert f(2, 4, 0, 12, *args) == -1 and f(4, 5, 0, 12, *args) == -1 and f(4, 4, 4, 12, *args) == -1 and f(4, 4, 0, -1, *args) == -1
    assert f(4, 4, 0, 12, head.ctypes.data, pos.ctypes.data, 8, grp.ctypes.data, 32, None) == -2
    assert f(4, 4, 0, 0, *args) == 0 and 10 <= head[5] <= 16              # A = 0: the lookahead the library is built with
    # a lookahead the register ring cannot hold behind a part's eight requests is refused by the library's replay and by this one
    verdict, h, p, g, _ = plan(4, 4, 0, 28)
    assert verdict == 6
    with pytest.raises(AssertionError, match="register slot"):
        replay(h, p, g)


def hook(name, R, ncols):
    f = getattr(C.CDLL(M._capi.LIB_PATH), name)
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int]
    return f(R, ncols)


def diag_at(R, ncols, batch):
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_diag_batch_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_longlong]
    return f(R, ncols, batch)


def test_stripe_diag_choice():
    names = ("MCD_STRIPE_SCHED", "MCD_STRIPE_PROLOGUE", "MCD_STRIPE_FINISH", "MCD_STRIPE_DIAG")
    before = {k: M.get_option(k) for k in names}
    try:
        for k in names:
            M.set_option(k, None)
        default = hook("mcd_stripe_diag_selftest_", 4, 256)              # the library's default at the headline batch, 512 chains
        assert default in (0, 1) and default == diag_at(4, 256, 512)
        by_batch = [diag_at(4, 256, b) for b in range(1, 513)]           # unset, the batch decides: the ring below one threshold
        assert all(v in (0, 1) for v in by_batch) and by_batch == sorted(by_batch)
        for n in range(129, 257):
            R, ncols = (n + 63) // 64, 16 * ((n + 15) // 16)
            whole = ncols == 64 * R                                      # N = 177 .. 192 and 241 .. 256: schedule 2 runs there
            for sched in (None, 0, 1, 2):
                for prologue in (None, 0, 1):
                    for fin in (None, 0, 1):
                        reports = set()
                        for diag in (None, 0, 1, 2):
                            for k, v in zip(names, (sched, prologue, fin, diag)):
                                M.set_option(k, v)
                            perchain = whole and sched in (None, 2) and prologue != 0 and fin != 0
                            on = default if diag is None else int(diag != 0)
                            assert hook("mcd_stripe_diag_selftest_", R, ncols) == (on if perchain else 0), (n, sched, prologue, fin, diag)
                            if diag is not None:                         # a value set holds at every batch
                                assert {diag_at(R, ncols, b) for b in (1, 129, 256, 512)} == {on if perchain else 0}
                            # ... and the two older reports do not know the option
                            assert hook("mcd_stripe_finish_selftest_", R, ncols) == (1 if perchain else 0), (n, sched, prologue, fin, diag)
                            reports.add((hook("mcd_stripe_finish_selftest_", R, ncols), hook("mcd_stripe_schedule_selftest_", R, ncols)))
                        assert len(reports) == 1, (n, sched, prologue, fin)
                        want = -1 if prologue == 0 else (2 if whole else 1) if sched in (None, 2) else sched
                        assert reports.pop()[1] == want, (n, sched, prologue, fin)
        for k in names:
            M.set_option(k, None)
        assert hook("mcd_stripe_diag_selftest_", 2, 128) == -2 and hook("mcd_stripe_diag_selftest_", 5, 320) == -2
    finally:
        for k in names:
            M.set_option(k, before[k])


def test_regdiag_plan_standalone(tmp_path):
    exe = tmp_path / "test_stripe_plan_reg"
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "test_stripe_plan_reg.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("ok:"), out
