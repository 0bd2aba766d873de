"""The sign-tracking forms of the k256 throughput loop (halving, one-fold double subtraction, product plus square on one set of
columns, negated doubling and mixed addition), host build of the device templates (tests/hosttwin), against big integers and the
affine model.  Raw inputs cover the weakly reduced range [0, 2^256): values >= p, 2^256 - 1, values whose folds carry out of
word 2, sums of two products close to 2^513."""
import random

import pytest

from oracle import ecmodel as M
from oracle import synth
from hosttwin_util import lib, buf, outbuf

C_ = M.K256
P = C_.p
C = 2**256 - P
MASK = 2**256 - 1
EDGE = [0, 1, 2, 3, 977, C - 1, C, C + 1, P - 2, P - 1, P, P + 1, P + 2, 2**256 - 2, 2**256 - 1, 2**255, 2**255 + 1,
        2**128 - 1, 2**256 - C - 1, 2**256 - C // 2, 2**32 - 1, 2**32, 2**64 - 1, 2**96 - 1, (1 << 256) - (1 << 32),
        (1 << 256) - (1 << 96), (1 << 255) - 1]


HALF, SUB2, MULSQ, MULSQ_TOP = 0, 1, 2, 3          # ops of ht_k256_negforms_fe_op (tests/hosttwin/hosttwin_negforms.cpp)


def run(op, xs, ys):
    n = len(xs)
    a = b"".join(x.to_bytes(32, "big") for x in xs)
    b = b"".join(y.to_bytes(32, "big") for y in ys)
    out = outbuf(32 * n)
    assert lib().ht_k256_negforms_fe_op(op, buf(a), buf(b), out, n) == 0
    o = bytes(out)
    return [int.from_bytes(o[32 * i:32 * i + 32], "big") for i in range(n)]


def pairs(count=3000, seed=5):
    rng = random.Random(seed)
    xs, ys = [], []
    for x in EDGE:
        for y in EDGE:
            xs.append(x); ys.append(y)
    for _ in range(count):
        xs.append(rng.getrandbits(256)); ys.append(rng.getrandbits(256))
    # operands near the top of the range: the sums of the fused forms then carry out of every word
    for _ in range(200):
        xs.append(MASK - rng.getrandbits(40)); ys.append(MASK - rng.getrandbits(40))
    return xs, ys


@pytest.mark.parametrize("op,fn", [
    (HALF, lambda x, y: x * pow(2, -1, P)),
    (SUB2, lambda x, y: x - y - (MASK ^ y)),
    (MULSQ, lambda x, y: x * y + y * y),
    (MULSQ_TOP, lambda x, y: (MASK ^ x) * (MASK ^ y) + (MASK ^ x) ** 2),
])
def test_new_field_forms_on_raw_inputs(op, fn):
    xs, ys = pairs()
    for x, y, g in zip(xs, ys, run(op, xs, ys)):
        assert g < 2**256 and g % P == fn(x, y) % P, (op, hex(x), hex(y), hex(g))


def test_half_is_exact_and_weakly_reduced():
    # a / 2 for even a, (a + p) / 2 for odd a: exact integers, not just congruent
    vals = EDGE + [random.Random(9).getrandbits(256) for _ in range(500)]
    for x, g in zip(vals, run(HALF, vals, vals)):
        assert g == (x // 2 if x % 2 == 0 else (x + P) // 2), hex(x)


def test_mul_add_sqr_near_2_513():
    # xy + y^2 with both near 2^256: the column sum reaches word 16 (2^512 = C^2 mod p)
    rng = random.Random(17)
    xs = [MASK - rng.getrandbits(k) for k in (0, 1, 8, 32, 64, 128) for _ in range(20)]
    ys = [MASK - rng.getrandbits(k) for k in (0, 1, 8, 32, 64, 128) for _ in range(20)]
    assert any(x * y + y * y >= 2**512 for x, y in zip(xs, ys))
    for x, y, g in zip(xs, ys, run(MULSQ, xs, ys)):
        assert g < 2**256 and g % P == (x * y + y * y) % P


def jac_to_affine(X, Y, Z):
    if Z % P == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def fe(v):
    return int(v % P).to_bytes(32, "big")


def neg_pt(a):
    return None if a is None else M.affine_neg(C_, a)


def test_negated_point_forms_including_exceptional_cases():
    rng = random.Random(41)
    cases = []
    for i in range(60):
        A = synth.point(C_, i, seed=41)
        B = synth.point(C_, 200 + i, seed=41)
        z = rng.randrange(1, P)
        cases.append(((A[0] * z * z % P, A[1] * z * z * z % P, z), B, M.affine_add(C_, A, B)))
    A = synth.point(C_, 3, seed=41)
    z = rng.randrange(1, P)
    J = (A[0] * z * z % P, A[1] * z * z * z % P, z)
    cases.append((J, A, M.affine_add(C_, A, A)))                      # same point: doubling branch
    cases.append((J, M.affine_neg(C_, A), None))                      # opposite: infinity
    cases.append(((0, 0, 0), A, A))                                   # accumulator at infinity
    cases.append(((5, 9, 0), A, A))                                   # infinity with junk X, Y
    cases.append(((A[0], A[1], 1), A, M.affine_add(C_, A, A)))        # Z = 1 doubling
    pin = b"".join(fe(j[0]) + fe(j[1]) + fe(j[2]) for j, _, _ in cases)
    qin = b"".join(fe(q[0]) + fe(q[1]) for _, q, _ in cases)
    out = outbuf(96 * len(cases))
    assert lib().ht_k256_jac_add_mixed_neg(buf(pin), buf(qin), out, len(cases)) == 0
    o = bytes(out)
    for i, (_, _, want) in enumerate(cases):
        X, Y, Z = (int.from_bytes(o[96 * i + 32 * t:96 * i + 32 * t + 32], "big") for t in range(3))
        assert jac_to_affine(X, Y, Z) == neg_pt(want), i
    out = outbuf(96 * len(cases))
    assert lib().ht_k256_jac_double_neg(buf(pin), out, len(cases)) == 0
    o = bytes(out)
    for i, (j, _, _) in enumerate(cases):
        X, Y, Z = (int.from_bytes(o[96 * i + 32 * t:96 * i + 32 * t + 32], "big") for t in range(3))
        a = jac_to_affine(*j)
        assert jac_to_affine(X, Y, Z) == neg_pt(None if a is None else M.affine_add(C_, a, a)), i


def test_doubling_sequence_matches_the_model():
    # 40 negated doublings in a row against the affine model: the sign alternates, the point is 2^k P up to it
    A = synth.point(C_, 11, seed=43)
    z = 123456789
    j = (A[0] * z * z % P, A[1] * z * z * z % P, z)
    want = A
    for k in range(40):
        out = outbuf(96)
        assert lib().ht_k256_jac_double_neg(buf(fe(j[0]) + fe(j[1]) + fe(j[2])), out, 1) == 0
        o = bytes(out)
        j = tuple(int.from_bytes(o[32 * t:32 * t + 32], "big") for t in range(3))
        want = M.affine_add(C_, want, want)
        got = jac_to_affine(*j)
        assert got == (want if k % 2 == 1 else neg_pt(want)), k
