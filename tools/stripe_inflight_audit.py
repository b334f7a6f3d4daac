#!/usr/bin/env python3
"""In-flight register audit of the stripe kernels as the library ships them.

The stripe kernel (csrc/stripe_device.hpp) hides its register loads and LDS reads from the compiler in asm statements and waits for
them by count, so the compiler holds a destination register written at the statement and may read, copy, spill or reuse it before
the data has landed.  Whether it did is a property of the generated code, so this script reads the code: it takes the gfx950 code
object that holds the kernel out of the built library, disassembles the kernel and walks it along every path (both sides of every
conditional branch, a state visited once) with
  * the vector-memory operations outstanding, a queue that `s_waitcnt vmcnt(n)` retires from the front down to n (loads, stores and
    LDS-DMAs count together, in issue order), and
  * the LDS and scalar-memory operations outstanding, retired the same way by `lgkmcnt(n)` (the compiler counts its own LDS reads;
    it waits for 0 wherever a scalar load is out, which may return out of order),
and reports every instruction that reads or writes the destination of a load no wait has covered yet (a later load of the same
queue into that register lands behind it and is none).  Branch conditions are not correlated: a path is
followed even where its conditions cannot hold together, so a report has to be read.  It also returns the kernel's
registers, spills and scratch from the code object's metadata.  tests/test_stripe_codegen_host.py runs it on every build.

    tools/stripe_inflight_audit.py [libmcmcdate_mvn.so] [kernel symbol prefix ...]
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmc-date_amd", "libmcmcdate_mvn.so")
STRIPE = "_ZN3mcd15k_logpdf_stripeILi%dELi4ELb1ELi%dE"        # k_logpdf_stripe<R, 4, true, SC>
STRIPE_FIN = "_ZN3mcd19k_logpdf_stripe_finILi%dELi4EE"        # k_logpdf_stripe_fin<R, 4>
STRIPE_REG = "_ZN3mcd19k_logpdf_stripe_regILi%dELi4EE"        # k_logpdf_stripe_reg<R, 4>


def regs(text):
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", text):
        if m.group(1):
            out |= set(range(int(m.group(1)), int(m.group(2)) + 1))
        else:
            out.add(int(m.group(3)))
    return frozenset(out)


def code_object(lib, prefix, work):
    """the code object of `lib` that defines a kernel whose symbol starts with `prefix`, and the symbol"""
    copy = os.path.join(work, "lib.so")
    if not os.path.exists(copy):
        shutil.copy(lib, copy)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], check=True, capture_output=True)
    for f in sorted(os.listdir(work)):
        if "amdgcn" not in f:
            continue
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", os.path.join(work, f)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\s(" + re.escape(prefix) + r"\S*)", syms):
            if not m.group(1).endswith(".kd"):
                return os.path.join(work, f), m.group(1)
    raise LookupError(prefix)


def metadata(obj, symbol):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, capture_output=True, text=True).stdout
    entry = [e for e in notes.split("\n  - ") if re.search(r"\.name:\s+" + re.escape(symbol) + r"\n", e)][0]
    out = {}
    for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "agpr_count"):
        m = re.search(r"\." + key + r":\s+(\d+)", entry)
        out[key] = int(m.group(1)) if m else 0
    return out


def disassemble(obj, symbol):
    """[(address, mnemonic, operands, branch target or None)]"""
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + symbol, obj],
                         check=True, capture_output=True, text=True).stdout
    base = int(re.search(r"^([0-9a-f]+) <" + re.escape(symbol) + ">:", txt, re.M).group(1), 16)
    ins = []
    for line in txt.split("\n"):
        m = re.match(r"\s+(\S+)\s*(.*?)\s*// ([0-9A-F]+):(.*)$", line)
        if not m:
            continue
        t = re.search(r"<" + re.escape(symbol) + r"\+0x([0-9a-f]+)>", m.group(4))
        ins.append((int(m.group(3), 16), m.group(1), m.group(2), base + int(t.group(1), 16) if t else None))
    return ins


def audit(ins, verbose=True):
    at = {a: i for i, (a, _, _, _) in enumerate(ins)}
    seen, found = set(), {}
    loads = set()
    most = 0
    todo = [(0, (), ())]
    while todo:
        i, vm, lgkm = todo.pop()
        while i < len(ins):
            if (i, vm, lgkm) in seen:
                break
            seen.add((i, vm, lgkm))
            addr, op, args, target = ins[i]
            if op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", args)
                if m:
                    vm = vm[max(0, len(vm) - int(m.group(1))):]
                m = re.search(r"lgkmcnt\((\d+)\)", args)
                if m:
                    lgkm = lgkm[max(0, len(lgkm) - int(m.group(1))):]
                i += 1
                continue
            vbusy, lbusy = frozenset().union(*vm), frozenset().union(*lgkm)
            bad = regs(args) & (vbusy | lbusy)
            if op.startswith(("global_load_dword", "ds_read")) and "lds" not in op:
                # a load over the destination of an earlier load of the same queue lands behind it (in order): no hazard
                dest, rest = regs(args.split(",")[0]), regs(args.split(",", 1)[1])
                bad = (rest & (vbusy | lbusy)) | (dest & (lbusy if op.startswith("global") else vbusy))
            if bad and addr not in found:
                found[addr] = f"{addr:#x}: {op} {args}: touches in-flight v{sorted(bad)[:8]}"
            if op.startswith("global_load_dword") and "lds" not in op:
                vm += (regs(args.split(",")[0]),)
                loads.add(addr)
            elif op.startswith(("global_load_lds", "global_store", "global_atomic", "scratch_", "buffer_")):
                vm += (frozenset(),)
            elif op.startswith("ds_read"):
                lgkm += (regs(args.split(",")[0]),)
            elif op.startswith(("ds_", "s_load", "s_memtime", "s_memrealtime")):
                lgkm += (frozenset(),)
            vm, lgkm = vm[-63:], lgkm[-15:]               # (the counters' widths: the hardware stalls there)
            most = max(most, len(vm))
            if op in ("s_endpgm", "s_setpc_b64"):
                break
            if op == "s_branch":
                i = at[target]
                continue
            if op.startswith("s_cbranch"):
                todo.append((at[target], vm, lgkm))
            i += 1
    if verbose:
        for a in sorted(found):
            print(found[a])
    return {"register_loads": len(loads), "most_outstanding": most, "violations": len(found)}


def report(lib, prefix, work, verbose=True):
    obj, symbol = code_object(lib, prefix, work)
    out = metadata(obj, symbol)
    ins = disassemble(obj, symbol)
    out.update(audit(ins, verbose))
    out["lds_dmas"] = sum(op.startswith("global_load_lds") for _, op, _, _ in ins)   # LDS-DMA instructions in the kernel's text
    out["symbol"] = symbol
    return out


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else LIB
    prefixes = sys.argv[2:] or [STRIPE % (R, SC) for R in (3, 4) for SC in (1, 2)]
    rc = 0
    with tempfile.TemporaryDirectory() as work:
        for p in prefixes:
            r = report(lib, p, work)
            print(r)
            rc |= r["violations"] > 0
    sys.exit(rc)
