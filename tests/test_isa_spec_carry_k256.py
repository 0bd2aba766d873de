"""Static check of the speculative columns in the headline kernel's two hot loop bodies (k256_mul_fast_kernel<32, 4>, found with the
loop finder of tests/test_isa_budget_k256.py): the multiplies are the parent's, the carry additions of the speculative products
are gone, the carry-out masks go to scalar-register pairs, and the rare blocks that add a missing carry lie outside the bodies.
Skipped when the object is not built (no GPU needed).

The VALU bounds: the parent's pinned counts (doubling 1133 VALU / 333 non-pair, addition 1921 / 487) minus 70 and minus 120 are the
least that must go; the values reached are pinned: doubling 1054 / 254 (minus 79), addition 1792 / 358 (minus 129)."""
import re

import pytest

import test_isa_budget_k256 as B
import test_isa_fold_first_k256 as F

pytestmark = B.pytestmark

DBL_MADS, ADD_MADS = 400, 717
DBL_VALU_MAX, DBL_NONPAIR_MAX = 1054, 254
ADD_VALU_MAX, ADD_NONPAIR_MAX = 1792, 358
assert DBL_VALU_MAX <= 1133 - 70 and DBL_NONPAIR_MAX <= 333 - 70 and ADD_VALU_MAX <= 1921 - 120 and ADD_NONPAIR_MAX <= 487 - 120


@pytest.fixture(scope="module")
def bodies():
    ins, spans = F.hot_bodies()
    assert set(spans) == {"dbl", "add"}
    return ins, spans


def sgpr_carry_mads(body):
    """the v_mad_u64_u32 whose carry destination is a scalar-register pair other than vcc"""
    return [t for t in body if re.match(r"v_mad_u64_u32\s+v\[\d+:\d+\],\s*s\[\d+:\d+\],", t)]


def test_multiplies_unchanged_and_no_scratch(bodies):
    _, spans = bodies
    (dbl, _), (add, _) = spans["dbl"], spans["add"]
    print("doubling", dbl, "addition", add)
    assert dbl["mad"] == DBL_MADS and add["mad"] == ADD_MADS
    assert dbl["scratch"] == 0 and add["scratch"] == 0


def test_fold_multiplies_still_carry_free(bodies):
    ins, spans = bodies
    regs = F.fold_registers(ins)
    for name in ("dbl", "add"):
        n, with_addc = F.fold_mads(spans[name][1], regs)
        assert n > 0 and with_addc == 0, (name, n, with_addc)


def test_speculative_mads_keep_their_mask_in_scalar_registers(bodies):
    _, spans = bodies
    for name in ("dbl", "add"):
        body = spans[name][1]
        spec = sgpr_carry_mads(body)
        checks = sum(t.startswith("s_cmp_eq_u64") or t.startswith("s_cmp_lg_u64") for t in body)
        print(name, "mads with a scalar carry destination", len(spec), "scalar mask checks", checks)
        assert len(spec) >= 1, name


COLD_FIX = re.compile(r"v_addc_co_u32(?:_e64)?\s+v\d+,\s*vcc,\s*0,\s*v\d+,\s*s\[\d+:\d+\]$")


def test_cold_blocks_outside_the_bodies(bodies):
    """the rare block of a speculative product is one v_addc_co_u32 whose carry-in is the saved scalar mask (not vcc): the kernel
    holds them (at least one per scalar mask check of the hot bodies), and none sits between a hot body's header and its latch"""
    ins, spans = bodies
    in_kernel = sum(bool(COLD_FIX.match(t)) for _, t in ins)
    checks = sum(t.startswith("s_cmp_eq_u64") or t.startswith("s_cmp_lg_u64") for name in ("dbl", "add") for t in spans[name][1])
    print("carry fix-ups in the kernel", in_kernel, "mask checks in the hot bodies", checks)
    assert checks > 0 and in_kernel >= checks
    for name in ("dbl", "add"):
        cold = [t for t in spans[name][1] if COLD_FIX.match(t)]
        assert not cold, (name, cold[:4])


def test_valu_counts(bodies):
    _, spans = bodies
    (dbl, _), (add, _) = spans["dbl"], spans["add"]
    print("doubling", dbl, "addition", add)
    assert dbl["valu"] <= DBL_VALU_MAX and dbl["nonpair"] <= DBL_NONPAIR_MAX, dbl
    assert add["valu"] <= ADD_VALU_MAX and add["nonpair"] <= ADD_NONPAIR_MAX, add
