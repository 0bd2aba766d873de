"""The related-point inputs of tests/related_point_vectors.py do what they are for: walked through the host build of the multi-point
schedules they ENTER every exceptional branch of the incomplete point additions - accumulator at infinity, addend at infinity, the
same point, opposite points - often enough, and the mid-loop branches also while the accumulator's Z has left 1.  The count comes
from the ECGPU_EXC_NOTE hook (csrc/mp32.hpp), which the host build turns into per-site counters and the product into nothing.  A
change to the vectors, or to a schedule, that silently stops reaching a branch fails here, on the CPU.

Every site in csrc/ has to be reached; there is no exempt list.  (The negated forms of the single-term secp256k1 loop,
k256::jac_add_mixed_neg, carry no hook: no multi-point schedule calls them, a single term of prime order cannot reach their
same-point branch, and tests/test_hosttwin_k256_neg_forms.py covers them case by case.  The sites of csrc/affine_ops.hpp - the sum
of two affine points after the schedules, and y from x - lie in no schedule: tests/test_hosttwin_sigsum.py enters each of them with
signatures built for it and pins the counts; here they are only listed, so that a new site still has to be asked for.)"""
import random

import pytest

from oracle import ecmodel as M
import related_point_vectors as V
import related_point_hostwalks as W

MIN_HITS = 8                                   # the bar tests/test_field_edge_coverage.py sets for rare paths
CURVES = ["k256", "p256", "p384"]
TERMS = (2, 3, 5, 16, 17, 40)
CASES = ("inf", "same", "same:z", "opp", "opp:z")
FOLD = ["jac.add." + s for s in ("p_inf", "q_inf", "same", "same:z", "opp", "opp:z")]
FORMULA_ONLY = (["jac.add_affine." + s for s in ("same", "opp")] + ["msm.xyzz_add_mixed." + s for s in CASES]          # no host-walkable schedule calls these
                + ["msm.xyzz_add." + s for s in ("p_inf", "q_inf", "same", "same:z", "opp", "opp:z")])
AFFINE_OPS = ["affsum." + s for s in ("both_inf", "one_inf", "same", "opp", "chord")] + ["lift.no_root"]       # csrc/affine_ops.hpp: two affine operands, no schedule; tests/test_hosttwin_sigsum.py enters each on its own rows
SCHEDULE_SITES = {
    "k256": ["k256.jac_add_mixed." + s for s in CASES] + FOLD,          # straus.hpp and the two-term lane body use the fused secp256k1 form
    "p256": ["jac.add_mixed." + s for s in CASES] + FOLD,
    "p384": ["jac.add_mixed." + s for s in CASES] + FOLD,
}


def _walk_schedules(cn, terms_list, count):
    c = M.CURVES[cn]
    for which in ("G", "S"):
        fam = V.family(cn, which)
        for terms in terms_list:
            for pat in V.PATTERNS:
                ks, ms = V.flatten(V.combos(fam, pat, terms, count, seed=2))
                for _, run in W.schedules(c, terms):
                    run(fam, ks, ms, None)


@pytest.mark.parametrize("cn", CURVES)
def test_schedules_reach_every_branch(cn):
    """straus.hpp at 2, 3, 5 (also with the odd group size 2 forced), 16, 17 and 40 terms, the two-term schedules (varbase_lane.hpp
    on P-256 / P-384, the two-term secp256k1 lane body): every branch of the window loop's mixed addition and of the fold's general
    addition at least MIN_HITS times, the same-point and opposite-point ones as often with Z != 1."""
    W.exc_reset()
    _walk_schedules(cn, TERMS, 6)
    got = W.exc_counts()
    low = {s: got.get(s, 0) for s in SCHEDULE_SITES[cn] if got.get(s, 0) < MIN_HITS}
    assert not low, (cn, low, got)


@pytest.mark.parametrize("cn", ["k256"])
def test_two_term_k256_lane_body_alone_reaches_every_branch(cn):
    """the two tables of the two-term secp256k1 kernel sit on the curve isomorphic by zfix0 * zfix1: "same point" and "opposite
    points" are recognised there across different original denominators"""
    c = M.CURVES[cn]
    W.exc_reset()
    for which in ("G", "S"):
        fam = V.family(cn, which)
        for pat in V.PATTERNS:
            ks, ms = V.flatten(V.combos(fam, pat, 2, 24, seed=3))
            W.k256_fast(fam, ks, ms, 2, random.Random(5) if pat == "collide" else None)
    got = W.exc_counts()
    low = {s: got.get(s, 0) for s in SCHEDULE_SITES[cn][:5] if got.get(s, 0) < MIN_HITS}
    assert not low, (low, got)
    assert not [s for s in got if s.startswith("jac.add.")]               # no fold in this walk: the counts above are the lane body's


@pytest.mark.parametrize("cn", CURVES)
def test_formulas_reach_every_site_on_family_operands(cn):
    """Every ECGPU_EXC_NOTE site of csrc/, entered one formula call at a time with operands from the family (first operand with a
    random Z, so the ":z" sites count too), and the sums are right."""
    c = M.CURVES[cn]
    fam = V.family(cn, "S")
    rng = random.Random(11)
    n = c.n
    mult = [m for m in fam.mult]
    same = [(m, m) for m in rng.sample(mult, 10)]
    opp = [(m, n - m) for m in rng.sample(mult, 10)]
    plain = [(1, 2), (3, n - 5), (16, 1 << 16)]
    W.exc_reset()
    for op, pairs in [("add_mixed", same + opp + plain + [(0, m) for m in mult[:10]]),
                      ("add_affine", same + opp + plain),
                      ("add", same + opp + plain + [(0, m) for m in mult[:10]] + [(m, 0) for m in mult[:10]] + [(0, 0)]),
                      ("xyzz_add", same + opp + plain + [(0, m) for m in mult[:10]] + [(m, 0) for m in mult[:10]] + [(0, 0)]),
                      ("xyzz", same + opp + plain + [(0, m) for m in mult[:10]])]:
        got = W.formula(fam, op, pairs, rng)
        for (a, b), g in zip(pairs, got):
            s = (a + b) % n
            assert g == (M.affine_mul(c, s, fam.base) if s else None), (op, a, b)
    hits = W.exc_counts()
    sites = W.exc_sites_in_source()
    assert sites == set(SCHEDULE_SITES["k256"]) | set(SCHEDULE_SITES["p256"]) | set(FORMULA_ONLY) | set(AFFINE_OPS) and set(hits) <= sites
    mine = {s for s in sites if not s.startswith("k256.")} - set(AFFINE_OPS)           # the fused secp256k1 form has no entry of its own: the schedules above
    low = {s: hits.get(s, 0) for s in mine if hits.get(s, 0) < MIN_HITS}
    assert not low, (cn, low)


def test_every_site_is_asked_for():
    """a new ECGPU_EXC_NOTE site in csrc/ has to be added to a list above"""
    asked = set(SCHEDULE_SITES["k256"]) | set(SCHEDULE_SITES["p256"]) | set(SCHEDULE_SITES["p384"]) | set(FORMULA_ONLY) | set(AFFINE_OPS)
    assert W.exc_sites_in_source() == asked


@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("wbits", [4, 5, 16, 19])
def test_crafted_collisions_are_collisions(cn, wbits):
    """craft_collision finds, for the window widths of every schedule (Straus 4, single-term 5, MSM 16 and 19 bits), pairs whose
    integer walk meets the same point and the opposite point with Z != 1"""
    fam = V.family(cn, "G")
    rng = random.Random(wbits)
    for want in ("same", "opp"):
        for _ in range(4):
            ks, ms, _ = V.craft_collision(fam, rng, wbits, want)
            assert V.walk_events(fam.c, ks, ms, wbits)[want + "_z"] >= 1
