"""Host build of every multi-point schedule that can be walked on the CPU - the shared-doubling many-term schedule (csrc/straus.hpp),
the two-term schedules (csrc/varbase_lane.hpp on P-256 / P-384, the lane body of the two-term secp256k1 throughput kernel) and, as
a control, the single-term ones - on RELATED points (tests/related_point_vectors.py: P, -P, jP, lambda P, 2^w P, ((n +- 1) / 2) P
of one base point), where the partial sums meet the exceptional cases of the incomplete addition formulas.  The expected group
element is (sum k_i m_i mod n) B: Python integers and one scalar multiplication of the big-integer model.
tests/test_related_point_coverage.py shows that these inputs enter the branches."""
import random

import pytest

from oracle import ecmodel as M
import related_point_vectors as V
import related_point_hostwalks as W

CURVES = ["k256", "p256", "p384"]
COUNT = 5                                      # combinations per (base, pattern, terms, format): ~1 900 per curve over all schedules


def _check(c, fam, cs, got, what):
    assert len(got) == len(cs)
    for i, ((ks, ms), g) in enumerate(zip(cs, got)):
        want = V.expected(c, ks, ms, fam.base)
        assert (bytes(g[0]), int(g[1])) == want, (what, i, [hex(k) for k in ks], [hex(m) for m in ms])


@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("pattern", V.PATTERNS)
@pytest.mark.parametrize("terms", [1, 2, 3, 5, 7, 16, 17, 40])
def test_schedules_on_related_points(cn, pattern, terms):
    c = M.CURVES[cn]
    for which in ("G", "S"):
        fam = V.family(cn, which)
        cs = V.combos(fam, pattern, terms, COUNT, seed=1)
        ks, ms = V.flatten(cs)
        for name, run in W.schedules(c, terms):
            _check(c, fam, cs, run(fam, ks, ms, None), (name, which, "affine"))
            _check(c, fam, cs, run(fam, ks, ms, random.Random(terms)), (name, which, "projective"))


@pytest.mark.parametrize("cn", CURVES)
def test_few_combinations_on_a_large_machine(cn):
    """the plan falls back to small groups when there are fewer work items than lanes: every group is one term and the fold adds 6
    related partial sums"""
    c = M.CURVES[cn]
    fam = V.family(cn, "G")
    for pattern in V.PATTERNS:
        cs = V.combos(fam, pattern, 6, COUNT, seed=4)
        ks, ms = V.flatten(cs)
        _check(c, fam, cs, W.straus(fam, ks, ms, 6, None, lanes=2, plan_lanes=1 << 20), (pattern, "g = 1"))


def test_k256_two_term_regression_shapes():
    """the hand-written cases of the C ABI tests, and their lambda forms, through the two-term secp256k1 lane body"""
    c, fam = M.K256, V.family("k256", "G")
    n, L = c.n, M.K256_LAMBDA
    cs = [([5, 5], [1, 1]), ([7, 7], [1, n - 1]), ([3, n - 3], [2, 2]), ([5, 5 * L % n], [L, 1]), ([7, 7 * L % n], [L, n - 1]),
          ([9, 3], [1, 3]), ([9, n - 3], [1, 3]), ([1, 1], [(n + 1) // 2, (n + 1) // 2]), ([2, 1], [(n - 1) // 2, 1]), ([0, 0], [1, 2])]
    ks, ms = V.flatten(cs)
    _check(c, fam, cs, W.k256_fast(fam, ks, ms, 2), "two-term")
    _check(c, fam, cs, W.straus(fam, ks, ms, 2), "straus")


def test_k256_infinity_in_the_raw_p_representation():
    """secp256k1 field elements are kept lazily reduced, so zero has two raw forms, 0 and p, and is_zero_fast prefilters on the top
    word (0 or 2^32 - 1).  An accumulator whose Z (XYZZ: ZZ) is the raw value p is at infinity: every addition has to return the
    addend, the general ones on either side.  A zero test that only knows the raw 0 runs the formula on it instead."""
    from hosttwin_util import lib, buf, outbuf
    c, fam = M.K256, V.family("k256", "S")
    p, rng = c.p, random.Random(17)
    fe = lambda v: int(v).to_bytes(32, "big")
    ms = rng.sample(fam.mult, 12)
    n = len(ms)
    garbage = lambda k: b"".join(fe(rng.randrange(p)) for _ in range(k))
    affine = b"".join(fe(fam.point(m)[0]) + fe(fam.point(m)[1]) for m in ms)

    def jac(m):
        x, y = fam.point(m)
        z = rng.randrange(2, p)
        return fe(x * z * z % p) + fe(y * z * z * z % p) + fe(z)

    def xyzz(m):
        x, y = fam.point(m)
        z = rng.randrange(2, p)
        return fe(x * z * z % p) + fe(y * z * z * z % p) + fe(z * z % p) + fe(z * z * z % p)

    def points(o):
        res = []
        for i in range(n):
            X, Y, Z = (int.from_bytes(o[96 * i + 32 * t:96 * i + 32 * (t + 1)], "big") for t in range(3))
            res.append(None if Z % p == 0 else (X * pow(Z, -2, p) % p, Y * pow(Z, -3, p) % p))
        return res

    want = [fam.point(m) for m in ms]
    inf_jac = b"".join(garbage(2) + fe(p) for _ in ms)
    inf_xyzz = b"".join(garbage(2) + fe(p) + fe(p) for _ in ms)
    out = outbuf(96 * n)
    assert lib().ht_k256_jac_add_mixed(buf(inf_jac), buf(affine), out, n) == 0 and points(bytes(out)) == want           # the fused form
    assert lib().ht_jac_op(0, 1, buf(inf_jac), buf(affine), out, n) == 0 and points(bytes(out)) == want               # jac::add_mixed
    assert lib().ht_jac_op(0, 2, buf(inf_jac), buf(b"".join(jac(m) for m in ms)), out, n) == 0 and points(bytes(out)) == want
    assert lib().ht_jac_op(0, 2, buf(b"".join(jac(m) for m in ms)), buf(inf_jac), out, n) == 0 and points(bytes(out)) == want
    assert lib().ht_xyzz_add_mixed(0, buf(inf_xyzz), buf(affine), out, n) == 0 and points(bytes(out)) == want
    assert lib().ht_xyzz_add(0, buf(inf_xyzz), buf(b"".join(xyzz(m) for m in ms)), out, n) == 0 and points(bytes(out)) == want
    assert lib().ht_xyzz_add(0, buf(b"".join(xyzz(m) for m in ms)), buf(inf_xyzz), out, n) == 0 and points(bytes(out)) == want
