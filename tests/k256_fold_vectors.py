"""Inputs that drive every column of the k256 products to its maximum (fe_k256.hpp: mul, mul_add2, mul_add_sqr), for the
tests of the carry-free leading products of each column: all-ones limbs, p - 1, p, values in [p, 2^256), operand pairs whose
high product half has words of 2^32 - 1, square operands with the top bit set (d_8 = 1), and random inputs with limbs drawn
from the extremes."""
import random

P = 2**256 - 2**32 - 977
TOP = 2**256 - 1

EDGES = [0, 1, 977, 2**32 - 1, 2**32, P - 1, P, P + 1, P + 2**32 + 976, TOP - 1, TOP, 2**255, 2**255 - 1,
         TOP - (2**32 - 1), TOP ^ (2**32 - 1) << 32, 2**128 - 1, 2**128 + 1]
WORDS = [0, 1, 2, 977, 2**31, 2**31 - 1, 2**32 - 2, 2**32 - 1]


def extreme(rng):
    """a 256-bit value whose words are mostly 0, 1, 2^31, 2^32 - 1 and the like"""
    v = 0
    for _ in range(8):
        w = rng.choice(WORDS) if rng.random() < 0.8 else rng.getrandbits(32)
        v = (v << 32) | w
    return v


def high_ones_pair(rng):
    """a, b < 2^256 with a * b just below the largest product: words 8..15 of a * b are 2^32 - 1 or close"""
    a = TOP - rng.getrandbits(rng.choice([1, 8, 32, 64, 128]))
    b = (2**512 - 2**257) // a
    return a, min(b, TOP)


def pairs(n=1500, seed=29):
    rng = random.Random(seed)
    out = [(x, y) for x in EDGES for y in EDGES]
    while len(out) < n:
        r = rng.random()
        if r < 0.3:
            out.append(high_ones_pair(rng))
        elif r < 0.8:
            out.append((extreme(rng), extreme(rng)))
        else:
            out.append((rng.getrandbits(256), rng.getrandbits(256)))
    return out


def quads(n=1500, seed=31):
    """(a, b, e, f) for a b + e f and (a, b, s) for a b + s^2 (f unused): sums up to 2^513, and sums in
    [2^512 - 2^256, 2^512) whose high half is all ones"""
    rng = random.Random(seed)
    out = [(TOP, TOP, TOP, TOP), (TOP, TOP, 2**128 + 1, 2**128), (TOP, TOP, 2**128 + 1, 2**128 + 1), (P, P, P, P),
           (P - 1, P - 1, P - 1, P - 1), (TOP, TOP, 0, 0), (0, 0, TOP, TOP), (2**255, 2**255, 2**255, 2**255)]
    out += [(x, y, x, y) for x in EDGES for y in EDGES[::2]]
    while len(out) < n:
        r = rng.random()
        if r < 0.3:
            a, b = high_ones_pair(rng)
            e = rng.getrandbits(rng.choice([64, 128, 129, 130]))
            out.append((a, b, e, e + rng.getrandbits(8)))
        elif r < 0.8:
            out.append(tuple(extreme(rng) for _ in range(4)))
        else:
            out.append(tuple(rng.getrandbits(256) for _ in range(4)))
    return out


def to_bytes(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)
