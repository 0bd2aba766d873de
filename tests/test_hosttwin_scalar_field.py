"""Scalar fields (scalar_mont.hpp: smont::mul / add / reduce_once / to_mont / from_mont / inv modulo the three group orders),
host build of the device templates (tests/hosttwin), against Python integers on the edges of tests/field_edge_vectors.py and
random inputs.  Operands are raw little-endian words; mul, to_mont, from_mont and inv work in Montgomery form, R = 2^(32 L)."""
import random

import numpy as np
import pytest

import field_edge_vectors as V
from devtwin_util import host, scalar_op


def expected(op, a, b, n, L):
    R = 2**(32 * L)
    Ri = pow(R, -1, n)
    if op == "mul":
        return a * b * Ri % n
    if op == "add":
        return (a + b) % n
    if op == "reduce_once":
        return a % n
    if op == "to_mont":
        return a * R % n
    if op == "from_mont":
        return a * Ri % n
    if op == "inv":
        return pow(a * Ri % n, n - 2, n) * R % n


def operands(op, n, L, count, seed):
    """edge pairs plus random pairs, inside each op's domain: below n, below min(2n, 2^(32 L)) for reduce_once"""
    rng = random.Random(seed)
    ps = V.edge_pairs(n, L)
    if op == "inv":
        ps = [(a, 0) for a in V.edges(n, L)]
    ps += [(rng.randrange(n), rng.randrange(n)) for _ in range(count)]
    if op == "reduce_once":
        top = min(2 * n, 2**(32 * L))
        ps += [(top - 1 - rng.getrandbits(rng.choice([8, 64, 200])), 0) for _ in range(count)]
        ps += [(n + x, 0) for x in V.edges(n, L) if n + x < top]
    return ps


@pytest.mark.parametrize("op", ["mul", "add", "reduce_once", "to_mont", "from_mont", "inv"])
@pytest.mark.parametrize("curve", ["k256", "p256", "p384"])
def test_scalar_field_op(curve, op):
    n, L = V.SCALAR_FIELDS[curve]
    ps = operands(op, n, L, 200 if op == "inv" else 2000, seed=len(curve) * 100 + len(op))
    a, b = [p[0] for p in ps], [p[1] for p in ps]
    got = V.from_words(scalar_op(host()["scalar"], curve, op, V.to_words(a, L), V.to_words(b, L)))
    for x, y, g in zip(a, b, got):
        assert g < n and g == expected(op, x, y, n, L), (curve, op, hex(x), hex(y), hex(g))


def test_scalar_inverse_of_zero_is_zero():
    for curve, (n, L) in V.SCALAR_FIELDS.items():
        z = np.zeros((1, L), dtype=np.uint32)
        assert not scalar_op(host()["scalar"], curve, "inv", z, z).any(), curve
