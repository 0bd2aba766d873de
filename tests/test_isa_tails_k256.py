"""Static check of the reduction tails in the headline kernel's two hot loop bodies (k256_mul_fast_kernel<32, 4>, found with the loop
finder of tests/test_isa_budget_k256.py): the overflow count T is assembled on the carry chains and folded with two multiplies and
three carry instructions (csrc/fe_k256.hpp: add_high_chain, fold_top_words).  Skipped when the object is not built (no GPU needed).

- The multiplies are the parent's, exactly, and neither body touches scratch memory.
- A tail's fold multiplies read 977 from a scalar register (the columns' fold products read theirs from a VGPR).  In the ten
  instructions before the first of them no carry flag is turned into a 0 / 1 word (v_cndmask_b32 v, 0, 1, carry) and no 64-bit
  pair is added with v_lshl_add_u64 .., 0, ..: that is how T was assembled before.
- The VALU bounds: the parent's pinned counts (doubling 1054 VALU / 254 non-pair, addition 1792 / 358) minus 24 and minus 40, four
  instructions per tail, are the least that must go; the values reached are pinned below."""
import re

import pytest

import test_isa_budget_k256 as B
import test_isa_fold_first_k256 as F

pytestmark = B.pytestmark

DBL_MADS, ADD_MADS = 400, 717
DBL_TAILS, ADD_TAILS = 6, 10                       # 3 sqr, 2 mul, 1 mul_add_sqr;  3 sqr, 6 mul, 1 mul_add2
DBL_VALU_MAX, DBL_NONPAIR_MAX = 1013, 213          # minus 41
ADD_VALU_MAX, ADD_NONPAIR_MAX = 1725, 291          # minus 67
assert DBL_VALU_MAX <= 1054 - 24 and DBL_NONPAIR_MAX <= 254 - 24 and ADD_VALU_MAX <= 1792 - 40 and ADD_NONPAIR_MAX <= 358 - 40

# a fold multiply of a tail: by a scalar register, and in place - its addend is the pair it writes, (r0, r1) or T (the 977
# multiplies that open a squaring's reduction also read a scalar register, but add a popped carry into a fresh pair)
SCALAR_MAD = re.compile(r"v_mad_u64_u32\s+(v\[\d+:\d+\]),\s*(?:vcc|s\[\d+:\d+\]),\s*v\d+,\s*s\d+,\s*\1$")
FLAG_TO_WORD = re.compile(r"v_cndmask_b32\S*\s+v\d+,\s*0,\s*1,")
PAIR_ADD = re.compile(r"v_lshl_add_u64\s+v\[\d+:\d+\],\s*[^,]+,\s*0,")


@pytest.fixture(scope="module")
def bodies():
    ins, spans = F.hot_bodies()
    assert set(spans) == {"dbl", "add"}
    return ins, spans


def tail_folds(body):
    """index of the first fold multiply of every tail: a v_mad_u64_u32 by a scalar register with no other one in the ten
    instructions before it (a tail has one, sqr, or two of them, a few instructions apart)"""
    idx = [i for i, t in enumerate(body) if SCALAR_MAD.match(t)]
    return [i for n, i in enumerate(idx) if n == 0 or i - idx[n - 1] > 10]


def test_multiplies_unchanged_and_no_scratch(bodies):
    _, spans = bodies
    (dbl, _), (add, _) = spans["dbl"], spans["add"]
    print("doubling", dbl, "addition", add)
    assert dbl["mad"] == DBL_MADS and add["mad"] == ADD_MADS
    assert dbl["scratch"] == 0 and add["scratch"] == 0


def test_overflow_count_stays_on_the_carry_chains(bodies):
    _, spans = bodies
    for name, tails in (("dbl", DBL_TAILS), ("add", ADD_TAILS)):
        body = spans[name][1]
        folds = tail_folds(body)
        print(name, "tails", len(folds))
        assert len(folds) == tails, (name, folds)
        for i in folds:
            window = body[max(0, i - 10):i]
            bad = [t for t in window if FLAG_TO_WORD.match(t) or PAIR_ADD.match(t)]
            assert not bad, (name, i, bad)


def test_tail_multiplies_keep_977_out_of_the_column_register(bodies):
    ins, spans = bodies
    regs = F.fold_registers(ins)
    for name in ("dbl", "add"):
        n, with_addc = F.fold_mads(spans[name][1], regs)
        assert n > 0 and with_addc == 0, (name, n, with_addc)


def test_valu_counts(bodies):
    _, spans = bodies
    (dbl, _), (add, _) = spans["dbl"], spans["add"]
    print("doubling", dbl, "addition", add)
    assert dbl["valu"] <= DBL_VALU_MAX and dbl["nonpair"] <= DBL_NONPAIR_MAX, dbl
    assert add["valu"] <= ADD_VALU_MAX and add["nonpair"] <= ADD_NONPAIR_MAX, add
