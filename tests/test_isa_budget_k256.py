"""Static instruction budget of the headline kernel's two hot loop bodies (k256_mul_fast_kernel<32, 4>): the doubling loop and the
digit-addition loop, found in the disassembly of the built object with tools/isa_loop_report.py.  Skipped when the object is not
built (it needs hipcc's gfx950 object and the ROCm disassembler, no GPU).

"Non-pair VALU" is the VALU instruction count minus twice the v_mad_u64_u32 count: what is left around the multiply-accumulate
pairs (carry chains of the folds and subtractions, shifts, selects, moves).  Budgets in DESIGN.md section 4."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "rustcrypto-elliptic-curves_amd", "build", "ops_k256.o")
KERNEL = "k256_mul_fast_kernelILi32ELi4E"
LLVM = "/opt/rocm/lib/llvm/bin"

# the parent's loops: doubling 421 mads, 398 non-pair VALU; addition 717 mads, 567 non-pair VALU
DBL_MAD_MAX, ADD_MAD_MAX = 400, 717
DBL_NONPAIR_MAX, ADD_NONPAIR_MAX = 370, 552

pytestmark = pytest.mark.skipif(not (os.path.exists(OBJ) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))),
                                reason="ops_k256.o not built or no ROCm disassembler")


def kernel_instrs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_loop_report as R
    text = R.disassemble(OBJ).split("\n")
    start = next(i for i, l in enumerate(text) if re.match(r"^[0-9a-f]+ <", l) and KERNEL in l)
    end = next((i for i in range(start + 1, len(text)) if re.match(r"^[0-9a-f]+ <", text[i])), len(text))
    addr_re = re.compile(r"//\s*([0-9A-F]+):")
    out = []
    for l in text[start + 1:end]:
        m = addr_re.search(l)
        if m:
            out.append((int(m.group(1), 16), l.split("//")[0].strip()))
    return out


def loops(instrs):
    """(header, latch) index pairs of every backward branch, as tools/isa_loop_report.py lists them."""
    amap = {a: i for i, (a, _) in enumerate(instrs)}
    res = []
    for i, (a, t) in enumerate(instrs):
        m = re.match(r"s_c?branch\w*\s+(\d+)", t)
        if m:
            off = int(m.group(1))
            if off >= 32768:
                off -= 65536
            tgt = a + 4 + 4 * off
            if tgt <= a and tgt in amap:
                res.append((amap[tgt], i))
    return sorted(set(res))


def mix(instrs, s, e):
    ops = [t.split()[0] for _, t in instrs[s:e + 1] if t]
    valu = sum(o.startswith("v_") for o in ops)
    mad = sum(o.startswith("v_mad_u64_u32") for o in ops)
    return {"valu": valu, "mad": mad, "nonpair": valu - 2 * mad, "scratch": sum(o.startswith("scratch_") for o in ops),
            "gload": sum(o.startswith("global_load") for o in ops)}


def hot_loops():
    """The digit-addition loop: the shortest loop that reads the table (global_load) and has the most mads among the loops of
    one point operation (fewer than 1000 mads; the position loop around both has more).  The doubling loop: of the loops without
    a table read that end before the addition loop starts, the header of the one that ends last, and of the loops with that
    header the shortest (the rare carry paths sit behind each loop and jump back, which makes longer 'loops' with the same
    header)."""
    ins = kernel_instrs()
    cand = [(s, e, mix(ins, s, e)) for s, e in loops(ins)]
    cand = [c for c in cand if 0 < c[2]["mad"] < 1000]
    adds = [c for c in cand if c[2]["gload"] > 0]
    top = max(c[2]["mad"] for c in adds)
    add = min((c for c in adds if c[2]["mad"] == top), key=lambda c: c[1] - c[0])
    dbls = [c for c in cand if c[2]["gload"] == 0 and c[1] < add[0]]
    head = max(dbls, key=lambda c: c[1])[0]
    dbl = min((c for c in dbls if c[0] == head), key=lambda c: c[1] - c[0])
    return dbl[2], add[2]


def test_hot_loop_budgets():
    dbl, add = hot_loops()
    print("doubling", dbl, "addition", add)
    assert dbl["mad"] <= DBL_MAD_MAX and add["mad"] <= ADD_MAD_MAX
    assert dbl["scratch"] == 0 and add["scratch"] == 0
    assert dbl["nonpair"] <= DBL_NONPAIR_MAX, dbl
    assert add["nonpair"] <= ADD_NONPAIR_MAX, add
