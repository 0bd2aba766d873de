"""Operands that drive the tail of the k256 reductions (csrc/fe_k256.hpp: add_high_chain, fold_top_words) to its edges, and a
Python model of the tail that says which paths an input takes.

Every product form computes V = L + H C, where H is the sum of the columns 8 .. 14 (with word 16, h8, for two products), L the sum
of the columns 0 .. 7 and C = 2^32 + 977: V = a b (+ e f, + s^2) - H p, so V is congruent to the product.  The tail splits
V = T 2^256 + r on two carry chains (T = t0 + t1 2^32 is the overflow count), adds T C to words 0 .. 2 of r, ripples a carry out of
word 2 (rare) and folds once more when the ripple crosses 2^256 (rarer).

Rows for the rare paths are SOLVED, not searched: the fully reduced result is prescribed and one operand is computed from it.
- ripple: the result is X 2^96 + eps with eps < 2^32 <= T C, so r = result - T C borrowed through words 0 .. 2 and adding T C
  back carries out of word 2; X below 2^160 - 1 keeps it from crossing 2^256.
- second fold: the result is C + eps with eps < 2^32.  r + T C is the result or the result + p; r >= 0 rules the first out as soon
  as T >= 2, so r + T C = 2^256 + eps: words 3 .. 7 of r are all ones and the ripple crosses 2^256.
The operand that is solved for: b = result / a for mul, f = (result - a b) / e for mul_add2, b = (result - s^2) / a for mul_add_sqr,
a = sqrt(result) for sqr (eps steps until the result is a square; p = 3 mod 4).  The model confirms every row (no row is dropped)."""
import random

import numpy as np

import field_edge_vectors as V

P = V.K256_P
C = V.K256_C
TOP = V.TOP
M32 = 2**32 - 1
FORMS = ["mul", "sqr", "mul_add2", "mul_add_sqr"]
# bit order of the masks of tests/hosttwin/hosttwin_k256_tails.cpp
SITES = ["sqr:c1", "chain:word7", "chain:t0", "mul:h8", "fold:k1", "fold:ripple", "fold:second"]
BIT = {s: 1 << i for i, s in enumerate(SITES)}

EXPECT = {
    "mul": lambda a, b, e, f: a * b,
    "sqr": lambda a, b, e, f: a * a,
    "mul_add2": lambda a, b, e, f: a * b + e * f,
    "mul_add_sqr": lambda a, b, e, f: a * b + e * e,
}


def words(x, n=8):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def _columns(a, b):
    aw, bw = words(a), words(b)
    return [sum(aw[i] * bw[k - i] for i in range(max(0, k - 7), min(k, 7) + 1)) for k in range(15)]


def _sqr2_columns(s):
    """the columns of s^2 as mul_add_sqr lays them out (fe_k256.hpp, sqr2_operands): the squares, and s_i times the words of
    2 sum_{j > i} s_j B^j: e_(i+1) = s_(i+1) << 1 and d_j = (s_j << 1) | (s_(j-1) >> 31), d_8 = s_7 >> 31"""
    sw = words(s)
    e = [(x << 1) & M32 for x in sw]
    d = [0, 0] + [((sw[j] << 1) & M32) | (sw[j - 1] >> 31) for j in range(2, 8)] + [sw[7] >> 31]
    cols = [0] * 15
    for i in range(8):
        cols[2 * i] += sw[i] * sw[i]
    for i in range(7):
        cols[2 * i + 1] += sw[i] * e[i + 1]
        for j in range(i + 2, 9):
            cols[i + j] += sw[i] * d[j]
    assert sum(c << (32 * k) for k, c in enumerate(cols)) == s * s
    return cols


def _fold(r, T):
    """fold_top_words on the 8-word value r: (result, mask of the fold sites)"""
    m = 0
    t0, t1 = T & M32, T >> 32
    r0, r1 = r & M32, (r >> 32) & M32
    a = t0 * 977 + r0
    if a + (r1 << 32) >= 2**64:
        m |= BIT["fold:k1"]
    low = (r & (2**96 - 1)) + T * C
    if low >= 2**96:
        m |= BIT["fold:ripple"]
        if r + T * C >= 2**256:
            m |= BIT["fold:second"]
    return (r + T * C) % P, m


def tail(form, a, b, e, f):
    """(T, mask of SITES, value mod p) of one product, computed the way the kernels compute it"""
    if form == "sqr":
        w = words(a * a, 16)
        lo = a * a % 2**256
        hi = a * a >> 256
        U = hi * 977
        top = U >> 256
        t = lo + U % 2**256
        c1 = t >> 256
        t %= 2**256
        r = t + ((hi % 2**224) << 32)
        c2 = r >> 256
        r %= 2**256
        x = top + c1
        T = x + w[15] + c2
        m = (BIT["sqr:c1"] if c1 else 0) | (BIT["chain:word7"] if c2 else 0) | (BIT["chain:t0"] if T >> 32 else 0)
        assert top < 2**11 and T < 2**32 + 2**11 + 2
    else:
        cols = _columns(a, b)
        if form == "mul_add2":
            cols = [x + y for x, y in zip(cols, _columns(e, f))]
        if form == "mul_add_sqr":
            cols = [x + y for x, y in zip(cols, _sqr2_columns(e))]
        H = sum(cols[k] << (32 * (k - 8)) for k in range(8, 15))
        h = words(H, 9)
        assert h[8] <= 1 and H < 2**257
        L = sum((cols[k] + h[k] * 977) << (32 * k) for k in range(8))
        t, c = L % 2**256, L >> 256
        assert c < 2**37
        r = t + ((H % 2**224) << 32)
        cy = r >> 256
        r %= 2**256
        cl = c + 977 * h[8]
        s0 = (cl & M32) + h[7] + cy
        T = cl + h[7] + cy + (h[8] << 32)
        assert T < 2**38
        m = (BIT["chain:word7"] if cy else 0) | (BIT["chain:t0"] if s0 >> 32 else 0) | (BIT["mul:h8"] if h[8] else 0)
    val, fm = _fold(r, T)
    assert val == EXPECT[form](a, b, e, f) % P
    return T, m | fm, val


def t_max(form):
    """the largest overflow count of a form: all-ones operands (every column sum is monotone in the words)"""
    return tail(form, TOP, TOP, TOP, TOP)[0]


def _inv(x):
    return pow(x % P, -1, P)


def _sqrt(x):
    r = pow(x, (P + 1) // 4, P)
    return r if r * r % P == x % P else None


def solve(form, result, rng):
    """operands (a, b, e, f) of `form` whose product is congruent to `result`; for sqr `result` must be a square (None if not)"""
    big = lambda: TOP - rng.getrandbits(200)              # large operands: T is near 2^32, far above 2
    if form == "sqr":
        a = _sqrt(result)
        if a is None:
            return None
        a = max(a, P - a)                                 # the larger root: a^2 fills the high half
        return (a, 0, 0, 0)
    if form == "mul":
        a = big()
        return (a, result * _inv(a) % P, 0, 0)
    if form == "mul_add2":
        a, b, e = big(), big(), big()
        return (a, b, e, (result - a * b) * _inv(e) % P)
    a, s = big(), big()
    return (a, (result - s * s) * _inv(a) % P, s, 0)


def ripple_rows(form, n=12, seed=5, second=False):
    """n solved rows that take the ripple out of word 2 (second: and the second fold)"""
    rng = random.Random(seed * 100 + FORMS.index(form) + (50 if second else 0))
    out = []
    while len(out) < n:
        eps = rng.getrandbits(31)
        while True:                                        # sqr: step eps to the next square (every second value is one)
            result = C + eps if second else (rng.getrandbits(159) << 96) + eps
            row = solve(form, result, rng)
            if row is not None:
                break
            eps += 1
        out.append(row)
    return out


def edge_rows(form):
    """the largest T, word 16 set and clear, and the chain carries in every combination the pools of field_edge_vectors reach"""
    rows = [(TOP, TOP, TOP, TOP), (TOP, TOP, 2**128 + 1, 2**128 + 1), (TOP, TOP, 0, 0), (0, 0, 0, 0), (1, 1, 1, 1), (P, P, P, P),
            (P - 1, P - 1, P - 1, P - 1), (2**255, 2**255, 2**255, 2**255)]
    rows += [(a, b, a, b) for a, b in V.pairs(400, seed=29)]
    rows += V.quads(400, seed=31)
    return rows


def vector_set(form):
    """four (n, 8) uint32 operand arrays: the edges, then the solved ripple rows, then the solved second-fold rows"""
    rows = edge_rows(form) + ripple_rows(form) + ripple_rows(form, second=True)
    return [V.to_words([r[k] for r in rows], 8) for k in range(4)]


def masks(form, ops):
    ints = [V.from_words(x) for x in ops]
    return np.array([tail(form, a, b, e, f)[1] for a, b, e, f in zip(*ints)], dtype=np.uint32)
