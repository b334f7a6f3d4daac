"""The issue plan of a stripe wave under the register-load schedule of the raw-x log-density kernel (csrc/stripe_plan.hpp,
MCD_STRIPE_SCHED = 2) is constexpr arithmetic shared by the host and the device.  mcd_stripe_plan_selftest_ returns a wave's plan and the
verdict of the library's own replay; here the plan is replayed once more, operation by operation, with a queue that retires in issue
order: every wait leaves exactly the operations issued behind the group's last unit, fewer than 64 operations are ever outstanding
(the prologue's loads included), no register slot and no ring slot is requested again before the group that reads it is done with it,
every immediate fits the instruction's 13 signed bits, and the waves together request every unit of the stream exactly once.
tests/cpp/test_stripe_plan.cpp, the same header without the library, is compiled and run too.  No GPU involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mcmc_date_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTAL = {3: 144, 4: 256}                         # units of the stream (fc_layout.hpp)
LOOKAHEADS = (10, 12, 14, 16)                    # the ones that are measured; 12 ships


def plan(R, S, w, A):
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_plan_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    head = np.full(6, -7, dtype=np.int32)
    pos = np.full((80, 6), -7, dtype=np.int32)
    grp = np.full((32, 7), -7, dtype=np.int32)
    verdict = f(R, S, w, A, head.ctypes.data, pos.ctypes.data, len(pos), grp.ctypes.data, len(grp))
    n, ng = int(head[0]), int(head[1])
    assert 0 < n <= len(pos) and 0 < ng <= len(grp)
    assert (pos[n:] == -7).all() and (grp[ng:] == -7).all()
    return verdict, [int(v) for v in head], pos[:n].tolist(), grp[:ng].tolist()


def replay(head, pos, grp):
    """the wave's operations in its order of events; returns the units it requested and the most operations outstanding"""
    n, ng, lead, pro, D, slots = head
    queue = [-1] * lead                                                  # -1: a leading load of the prologue
    landed, applied, read = set(), set(), set()
    reg, ring = {}, {}
    requested, issued, most = [], 0, lead

    def issue(upto):
        nonlocal issued, most
        assert issued <= upto <= n
        for u in range(issued, upto):
            kind, slot, base, imm, unit, g = pos[u]
            if kind == 1:
                assert 0 <= slot < slots and -4096 <= imm <= 4095 and base >= 0 and base + imm == 1024 * unit
                assert slot not in reg or pos[reg[slot]][5] in applied, ("register slot taken before its group was multiplied", u)
                reg[slot] = u
            else:
                assert slot == u % D
                assert slot not in ring or pos[ring[slot]][5] in read, ("ring slot taken before its group was read", u)
                ring[slot] = u
            requested.append(unit)
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
        assert beg == at and end > beg                                   # the groups tile the list in order
        assert all(pos[u][5] == g and pos[u][0] == (0 if diag else 1) for u in range(beg, end))
        at = end
        issue(pre)
        wait(vmcnt)
        assert all(u in landed for u in range(beg, end)), ("a unit read before it landed", g)
        assert len(queue) == vmcnt and (not queue or queue[0] == end), ("the wait covers more than the group", g)
        read.add(g)                                                      # its ring reads go out in front of ...
        if g:
            applied.add(g - 1)                                           # ... the multiply-adds of the group before
        issue(post)
    assert at == n == issued
    return requested, most


@pytest.mark.parametrize("R,S", [(3, 4), (3, 8), (4, 4), (4, 8)])
@pytest.mark.parametrize("A", LOOKAHEADS)
def test_stripe_plan(R, S, A):
    seen = np.zeros(TOTAL[R], dtype=int)
    for w in range(S):
        verdict, head, pos, grp = plan(R, S, w, A)
        assert verdict == 0, (w, verdict)
        assert head[3] == min(A, head[4], head[0]) and head[4] == 128 // S
        requested, most = replay(head, pos, grp)
        assert most < 64, (w, most)
        np.add.at(seen, requested, 1)
        assert any(p[0] == 0 for p in pos) and any(p[0] == 1 for p in pos)   # both kinds in every wave
    assert (seen == 1).all()                                             # every unit of the stream, exactly once


def test_stripe_plan_refuses():
    """a lookahead the register ring cannot hold is refused by the library's replay and by this one; so are the bad arguments"""
    verdict, head, pos, grp = plan(4, 4, 0, 32)
    assert verdict == 6
    with pytest.raises(AssertionError, match="register slot"):
        replay(head, pos, grp)
    f = C.CDLL(M._capi.LIB_PATH).mcd_stripe_plan_selftest_
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    head = np.zeros(6, dtype=np.int32)
    pos = np.zeros((80, 6), dtype=np.int32)
    grp = np.zeros((32, 7), dtype=np.int32)
    args = (head.ctypes.data, pos.ctypes.data, 80, grp.ctypes.data, 32)
    assert f(2, 4, 0, 12, *args) == -1 and f(4, 5, 0, 12, *args) == -1 and f(4, 4, 4, 12, *args) == -1 and f(4, 4, 0, 0, *args) == -1
    assert f(4, 4, 0, 12, head.ctypes.data, pos.ctypes.data, 8, grp.ctypes.data, 32) == -2


def test_stripe_plan_standalone(tmp_path):
    exe = tmp_path / "test_stripe_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "test_stripe_plan.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("ok:"), out
