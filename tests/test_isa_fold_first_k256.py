"""Static check of the headline kernel's two hot loop bodies (k256_mul_fast_kernel<32, 4>, found as in
tests/test_isa_budget_k256.py, disassembled with tools/isa_loop_report.py): every fold multiply - a v_mad_u64_u32 on the
register that holds 977 - goes in without a carry addition after it, since the fold product leads its column and cannot
carry (fe_k256.hpp, nc_bound).  Pins the VALU counts that this leaves.  Skipped when the object is not built (no GPU needed)."""
import re

import pytest

import test_isa_budget_k256 as B

pytestmark = B.pytestmark

# doubling and digit-addition loop bodies once the fold products and column 8's first products lead their columns
# (the parent's loops: doubling 1167 VALU / 367 non-pair, addition 1984 / 550)
DBL_VALU_MAX, DBL_NONPAIR_MAX = 1133, 333
ADD_VALU_MAX, ADD_NONPAIR_MAX = 1921, 487


def fold_registers(instrs):
    regs = {m.group(1) for _, t in instrs for m in [re.match(r"v_mov_b32(?:_e32)?\s+(v\d+),\s*0x3d1$", t)] if m}
    assert regs, "no register is loaded with 977"
    return regs


def hot_bodies():
    ins = B.kernel_instrs()
    dbl, add = B.hot_loops()
    spans = {}
    for s, e in B.loops(ins):
        mx = B.mix(ins, s, e)
        for name, want in (("dbl", dbl), ("add", add)):
            if mx == want and name not in spans:
                spans[name] = (mx, [t for _, t in ins[s:e + 1]])
    return ins, spans


def fold_mads(body, regs):
    """(count, count followed by a v_addc) of the v_mad_u64_u32 that multiply by the 977 register"""
    n = with_addc = 0
    for i, t in enumerate(body):
        if t.startswith("v_mad_u64_u32"):
            ops = [o.strip() for o in t.split(None, 1)[1].split(",")]
            if regs & set(ops[2:4]):
                n += 1
                with_addc += i + 1 < len(body) and body[i + 1].startswith("v_addc")
    return n, with_addc


def test_fold_multiplies_carry_free_and_valu_counts():
    ins, spans = hot_bodies()
    regs = fold_registers(ins)
    (dbl, dbl_body), (add, add_body) = spans["dbl"], spans["add"]
    nd, nd_addc = fold_mads(dbl_body, regs)
    na, na_addc = fold_mads(add_body, regs)
    print("doubling", dbl, "fold mads", nd, "addition", add, "fold mads", na)
    assert nd > 0 and na > 0
    assert nd_addc == 0 and na_addc == 0, (nd_addc, na_addc)
    assert dbl["valu"] <= DBL_VALU_MAX and dbl["nonpair"] <= DBL_NONPAIR_MAX, dbl
    assert add["valu"] <= ADD_VALU_MAX and add["nonpair"] <= ADD_NONPAIR_MAX, add
