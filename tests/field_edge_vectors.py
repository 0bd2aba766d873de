"""Inputs at the carry extremes of the field and scalar primitives (csrc/fe_k256.hpp, fe_mont.hpp, scalar_mont.hpp and the
column forms of mp32.hpp), with a Python predicate for every rare path they are built to take.

- For every modulus m on L words: 0, 1, 2, m - 1, m - 2, (m +- 1) / 2, m - 2^(32 k), R, R^2 and R^-1 mod m, values whose words
  are all taken from {0, 1, 2^31, 2^32 - 2, 2^32 - 1} below m, and pairs whose product is close to (m - 1)^2.
- For the Montgomery fields (P-256, P-384: -p^-1 = 1 mod 2^32), pairs whose quotient digits are chosen: a b = -D p mod R makes
  the digits of D the quotient digits m_0, m_1, .. of the product scanning, so they can be 0 or 2^32 - 1 on purpose.
- For k256 raw values (any integer below 2^256): the column-maximising vectors (EDGES, pairs, quads) and inputs that take the
  rare carry blocks of add, sub, sub2, fold_top_fast and shl<K>.
- For mac_cols<M, FRESH, NC>: accumulators near 2^64 - 1 / 2^32 - 1, all-ones products, and the NC bound of the call sites.

tests/test_field_edge_coverage.py asserts that enough inputs take every rare path; tests/test_gpu_field_primitives.py runs them
through the device build."""
import random

import numpy as np

# ---- moduli -------------------------------------------------------------------------------------------------------------
K256_P = 2**256 - 2**32 - 977
K256_C = 2**256 - K256_P                           # 2^32 + 977
P256_P = 2**256 - 2**224 + 2**192 + 2**96 - 1
P384_P = 2**384 - 2**128 - 2**96 + 2**32 - 1
K256_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P256_N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
P384_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973

MONT_FIELDS = {"p256": (P256_P, 8), "p384": (P384_P, 12)}            # index = curve argument of dt_mont_op
SCALAR_FIELDS = {"k256": (K256_N, 8), "p256": (P256_N, 8), "p384": (P384_N, 12)}   # index = curve argument of dt_scalar_op

WORD_EXTREMES = [0, 1, 2**31, 2**32 - 2, 2**32 - 1]
MASK32 = 2**32 - 1
MASK64 = 2**64 - 1


# ---- word arrays ----------------------------------------------------------------------------------------------------------
def to_words(vals, nwords):
    """integers -> (n, nwords) little-endian uint32 array"""
    raw = b"".join(int(v).to_bytes(4 * nwords, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u4").reshape(len(vals), nwords).astype(np.uint32)


def from_words(arr):
    """(n, nwords) uint32 array -> list of integers"""
    a = np.ascontiguousarray(arr, dtype="<u4")
    w = 4 * a.shape[1]
    raw = a.tobytes()
    return [int.from_bytes(raw[w * i:w * i + w], "little") for i in range(a.shape[0])]


# ---- generic edges of a modulus -------------------------------------------------------------------------------------------
def word_extreme_values(m, nwords, count, rng):
    """values below m whose words all come from WORD_EXTREMES (the top word drawn until the value is below m)"""
    out = []
    while len(out) < count:
        v = 0
        for _ in range(nwords):
            v = (v << 32) | rng.choice(WORD_EXTREMES)
        if v < m:
            out.append(v)
    return out


def edges(m, nwords, seed=1):
    """the edge values of one modulus, all below m"""
    R = 2**(32 * nwords)
    vals = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, R % m, R * R % m, pow(R, -1, m)]
    vals += [m - 2**(32 * k) for k in range(nwords) if 2**(32 * k) < m]
    vals += [m - 1 - 2**(32 * k) for k in range(nwords)]
    vals += word_extreme_values(m, nwords, 24, random.Random(seed * 1000 + nwords))
    seen, out = set(), []
    for v in vals:
        v %= m
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def near_max_product_pairs(m, count, rng):
    """a, b < m with a b close to (m - 1)^2: both near m - 1, or one a bit smaller and the other chosen to compensate"""
    out = []
    for _ in range(count):
        if rng.random() < 0.5:
            out.append((m - 1 - rng.getrandbits(rng.choice([1, 8, 32])), m - 1 - rng.getrandbits(rng.choice([1, 8, 32]))))
        else:
            a = m - 1 - rng.getrandbits(rng.choice([16, 40, 64, 100]))
            b = min(((m - 1)**2 - rng.getrandbits(40)) // a, m - 1)
            out.append((a, b))
    return out


def edge_pairs(m, nwords, seed=1):
    """every pair of edges, and pairs with a product close to (m - 1)^2"""
    e = edges(m, nwords, seed)
    rng = random.Random(seed * 7 + nwords)
    return [(x, y) for x in e for y in e] + near_max_product_pairs(m, 256, rng)


# ---- Montgomery quotient digits -------------------------------------------------------------------------------------------
MONT_TERMS = {   # fe_mont.hpp: reduction terms (offset, multiplier) added and offsets subtracted per quotient digit
    P256_P: ([(3, 1), (6, 1), (7, MASK32)], []),
    P384_P: ([(1, 1), (12, 1)], [3, 4]),
}


def mont_trace(w, m, nwords):
    """the product scanning of fe_mont.hpp on the 2L-word product w (a list of column sums: column K holds sum_{i+j=K} a_i b_j,
    or w[K] for the reduction-only pass of a separate squaring).  Returns (quotient digits, result before the final subtraction,
    smallest accumulator value seen after any column): the accumulator is signed while subtracted terms are in flight."""
    terms, negs = MONT_TERMS[m]
    c, q, t, low = 0, [], [], 0
    for K in range(2 * nwords):
        c += w[K] if K < len(w) else 0
        for off, mul in terms:
            i = K - off
            if 0 <= i < nwords:
                c += q[i] * mul
        for off in negs:
            i = K - off
            if 0 <= i < nwords:
                c -= q[i]
                low = min(low, c)
        if K < nwords:
            q.append(c & MASK32)
        elif K < 2 * nwords - 1:
            t.append(c & MASK32)
        else:
            t.append(c & MASK64)
            break
        c >>= 32                               # arithmetic shift, as acc_pop_signed
    res = sum(x << (32 * i) for i, x in enumerate(t))
    return q, res, low


def product_columns(a, b, nwords):
    aw = [(a >> (32 * i)) & MASK32 for i in range(nwords)]
    bw = [(b >> (32 * i)) & MASK32 for i in range(nwords)]
    return [sum(aw[i] * bw[k - i] for i in range(max(0, k - nwords + 1), min(k, nwords - 1) + 1)) for k in range(2 * nwords - 1)]


def square_words(a, nwords):
    s = a * a
    return [(s >> (32 * k)) & MASK32 for k in range(2 * nwords)]


def quotient_digit_targets(nwords, rng):
    """digit strings D (as integers below R) whose low digits are 0 or 2^32 - 1"""
    out = []
    for _ in range(4 * nwords):
        k = rng.randrange(1, nwords + 1)                     # the first k digits are extremes
        d = [rng.choice([0, MASK32]) for _ in range(k)]
        d += [rng.choice([0, MASK32, rng.getrandbits(32)]) for _ in range(nwords - k)]
        out.append(sum(x << (32 * i) for i, x in enumerate(d)))
    out += [0, MASK32, 2**(32 * nwords) - 2**32] + [2**(32 * nwords) - 1] * 4     # all ones: tried with several a
    return out


def quotient_digit_pairs(m, nwords, seed=3):
    """(a, b), both below m, with quotient digits D: a b = -D m (mod R), a odd"""
    rng = random.Random(seed * 13 + nwords)
    R = 2**(32 * nwords)
    out = []
    for D in quotient_digit_targets(nwords, rng):
        for _ in range(6):
            a = rng.choice([1, 3, m - 2, m - 4, rng.getrandbits(32 * nwords) | 1, (m - 1 - rng.getrandbits(64)) | 1,
                            rng.getrandbits(32) | 1, 2**(32 * nwords - 1) + 1])
            a %= m
            if a % 2 == 0:
                continue
            b = (-D * m * pow(a, -1, R)) % R
            if b < m:
                out.append((a, b))
    return out


def sqrt_mod_2k(x, k):
    """a square root of an odd x = 1 (mod 8) modulo 2^k"""
    r = 1
    for i in range(3, k):                  # r^2 = x (mod 2^i) -> (mod 2^(i+1))
        if ((r * r - x) >> i) & 1:
            r += 1 << (i - 1)
    return r % (1 << k)


def quotient_digit_squares(m, nwords, seed=5):
    """a below m whose squaring has quotient digits D: a^2 = -D m (mod R).  -D m = D (mod 2^32) must be a square, so the
    low digit is 1 or 2^32 - 7 (both 1 mod 8) and the others are extremes"""
    rng = random.Random(seed * 17 + nwords)
    R = 2**(32 * nwords)
    out = []
    for _ in range(8 * nwords):
        d = [rng.choice([1, MASK32 - 6])] + [rng.choice([0, MASK32, MASK32, rng.getrandbits(32)]) for _ in range(nwords - 1)]
        D = sum(x << (32 * i) for i, x in enumerate(d))
        r = sqrt_mod_2k((-D * m) % R, 32 * nwords)
        for a in (r, R - r, (r + R // 2) % R, (R - r + R // 2) % R):
            if a < m:
                out.append(a)
    return out


def mont_mul_min_acc(a, b, m, nwords):
    return mont_trace(product_columns(a, b, nwords), m, nwords)[2]


def mont_sqr_min_acc(a, m, nwords):
    return mont_trace(square_words(a, nwords), m, nwords)[2]


def mont_first_digit(a, b, m, nwords):
    return mont_trace(product_columns(a, b, nwords), m, nwords)[0][0]


# ---- k256 raw values: the column-maximising vectors -------------------------------------------------------------------------
P = K256_P
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


# ---- k256 rare carry paths: predicates (when the block runs with a non-zero carry) ------------------------------------------
def add_rare(a, b):
    """add: the fold of the carry out of 2^256 carries out of word 1"""
    s = a + b
    return s >> 256 == 1 and (s & MASK64) + K256_C > MASK64


def add_second_wrap(a, b):
    """add: the rippled carry crosses 2^256 again"""
    s = a + b
    return s >> 256 == 1 and (s & TOP) + K256_C > TOP


def sub_rare(a, b):
    """sub: the fold of the borrow borrows out of word 1"""
    return a < b and ((a - b) & MASK64) < K256_C


def sub_second_wrap(a, b):
    return a < b and ((a - b) & TOP) < K256_C


def sub2_borrows(a, b, e):
    v = a - b - e
    lo = v & TOP
    return lo, (lo - v) >> 256


def sub2_rare(a, b, e):
    """sub2: the fold of the combined borrow w in {1, 2} borrows out of word 1"""
    lo, w = sub2_borrows(a, b, e)
    return w > 0 and (lo & MASK64) < w * K256_C


def sub2_second_wrap(a, b, e):
    lo, w = sub2_borrows(a, b, e)
    return w > 0 and lo < w * K256_C


def fold_t(b):
    """the T of the K_FOLD_TOP_FAST op: b's low word plus 2^32 times the low byte of its second word"""
    return (b & MASK32) | (((b >> 32) & 0xFF) << 32)


def fold_top_fast_rare(r, T):
    """fold_top_fast: r + T C carries out of word 2"""
    return (r & (2**96 - 1)) + T * K256_C >= 2**96


def fold_top_fast_second_wrap(r, T):
    return r + T * K256_C > TOP


def shl_rare(a, K):
    """shl<K>: the fold of the K bits shifted out of the top carries out of word 1"""
    top = a >> (256 - K)
    return top > 0 and ((a << K) & MASK64) + top * K256_C > MASK64


def shl_second_wrap(a, K):
    """shl<K>: the rippled carry crosses 2^256 again"""
    return ((a << K) & TOP) + (a >> (256 - K)) * K256_C > TOP


# ---- k256 rare carry paths: constructions ---------------------------------------------------------------------------------
def make_add_rare(rng, second):
    t = TOP - rng.randrange(K256_C) if second else (rng.getrandbits(192) << 64) | (MASK64 - rng.randrange(K256_C))
    a = t + 1 + rng.randrange(TOP - t)
    return a, 2**256 + t - a


def make_sub_rare(rng, second):
    t = 1 + rng.randrange(K256_C - 1) if second else (rng.getrandbits(192) << 64) | rng.randrange(K256_C)
    t = max(t, 1)
    a = rng.randrange(t)
    return a, a + 2**256 - t


def make_sub2_rare(rng, second):
    w = rng.choice([1, 2])
    lo = 2 + rng.randrange(w * K256_C - 2) if second else (rng.getrandbits(192) << 64) | (2 + rng.randrange(w * K256_C - 2))
    a = rng.randrange(lo - 1)
    S = a - lo + w * 2**256                       # b + e
    blo, bhi = max(0, S - TOP), min(S, TOP)
    b = rng.choice([blo, bhi, rng.randint(blo, bhi)])
    return a, b, S - b


def make_fold_rare(rng, second):
    T = rng.choice([1, 2, rng.getrandbits(20), rng.getrandbits(40), 2**40 - 1])
    T = max(T, 1)
    if second:
        r = TOP - rng.randrange(T * K256_C)
    else:
        r = (rng.getrandbits(160) << 96) | (2**96 - 1 - rng.randrange(min(T * K256_C, 2**96)))
    b = (T & MASK32) | ((T >> 32) << 32) | (rng.getrandbits(24) << 40)     # bits above 40 are ignored by the op
    return r, b


def make_shl_rare(rng, K):
    top = rng.randrange(1, 2**K)
    need = -(-(2**64 - top * K256_C) // 2**K)              # (a mod 2^(64-K)) << K >= 2^64 - top C
    low = rng.randrange(max(need, 0), 2**(64 - K))
    return (top << (256 - K)) | (rng.getrandbits(192) << (64 - K)) | low


def k256_rare_inputs(per_path=64, seed=41):
    """{path name: list of operand tuples} for the rare carry blocks"""
    rng = random.Random(seed)
    out = {
        "add": [make_add_rare(rng, False) for _ in range(per_path)],
        "add_second_wrap": [make_add_rare(rng, True) for _ in range(per_path)],
        "sub": [make_sub_rare(rng, False) for _ in range(per_path)],
        "sub_second_wrap": [make_sub_rare(rng, True) for _ in range(per_path)],
        "sub2": [make_sub2_rare(rng, False) for _ in range(per_path)],
        "sub2_second_wrap": [make_sub2_rare(rng, True) for _ in range(per_path)],
        "fold_top_fast": [make_fold_rare(rng, False) for _ in range(per_path)],
        "fold_top_fast_second_wrap": [make_fold_rare(rng, True) for _ in range(per_path)],
    }
    for K in (1, 2, 3):
        out[f"shl{K}"] = [(make_shl_rare(rng, K),) for _ in range(per_path)]
    out["shl_edges"] = [(TOP,), (TOP - 1,), (2**255,), (P,), (TOP - K256_C,)]
    return out


def k256_rare_predicates():
    """{path name: (predicate on the op's operands, the operand tuples it applies to: (a, b) or (a, b, e) or (a,))}"""
    preds = {
        "add": (add_rare, 2), "add_second_wrap": (add_second_wrap, 2),
        "sub": (sub_rare, 2), "sub_second_wrap": (sub_second_wrap, 2),
        "sub2": (sub2_rare, 3), "sub2_second_wrap": (sub2_second_wrap, 3),
        "fold_top_fast": (lambda r, b: fold_top_fast_rare(r, fold_t(b)), 2),
        "fold_top_fast_second_wrap": (lambda r, b: fold_top_fast_second_wrap(r, fold_t(b)), 2),
    }
    for K in (1, 2, 3):
        preds[f"shl{K}"] = ((lambda a, K=K: shl_rare(a, K)), 1)
    return preds


# ---- mac_cols -------------------------------------------------------------------------------------------------------------
MAC_MAX_M = 13


def mac_forms():
    """every (M, FRESH, NC) that mac_cols instantiates"""
    return [(M, fresh, nc) for M in range(1, MAC_MAX_M + 1) for fresh in (0, 1) for nc in (0, 1, 2) if nc <= M]


def mac_inputs(M, fresh, nc, n, seed=0):
    """(c_in (n, 3), pa (n, 13), pb (n, 13)) uint32 arrays for mac_cols<M, fresh, nc>: c.lo near 2^64 - 1 or anywhere, c.hi 0
    for FRESH and near 2^32 - 1 otherwise, products of all-ones words; for NC > 0 the call sites' bound instead: c.lo < 2^37
    and a leading product below 2^42, or (NC = 2) c.lo < 2^32, a product below 2^32 and then any product."""
    g = np.random.default_rng([M, fresh, nc, seed])
    ext = np.array(WORD_EXTREMES + [MASK32, MASK32, MASK32 - 1], dtype=np.uint64)
    pick = g.random((n, MAC_MAX_M))
    pa = np.where(pick < 0.5, MASK32, np.where(pick < 0.8, ext[g.integers(0, len(ext), (n, MAC_MAX_M))],
                                               g.integers(0, 2**32, (n, MAC_MAX_M), dtype=np.uint64))).astype(np.uint64)
    pick = g.random((n, MAC_MAX_M))
    pb = np.where(pick < 0.5, MASK32, np.where(pick < 0.8, ext[g.integers(0, len(ext), (n, MAC_MAX_M))],
                                               g.integers(0, 2**32, (n, MAC_MAX_M), dtype=np.uint64))).astype(np.uint64)
    sel = g.random(n)
    lo = np.where(sel < 0.5, np.uint64(MASK64) - g.integers(0, 2**20, n, dtype=np.uint64),
                  np.where(sel < 0.9, g.integers(0, 2**63, n, dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, n, dtype=np.uint64),
                           g.integers(0, 2**16, n, dtype=np.uint64)))
    sel = g.random(n)
    hi = np.where(sel < 0.6, np.uint64(MASK32) - g.integers(0, 2**8, n, dtype=np.uint64),
                  g.integers(0, 2**32, n, dtype=np.uint64))
    if fresh:
        hi[:] = 0
    if nc >= 1:
        lo = g.integers(0, 2**37, n, dtype=np.uint64)
        lo[: n // 8] = 2**37 - 1
        pb[:, 0] = np.where(g.random(n) < 0.5, 977, g.integers(0, 2**10, n, dtype=np.uint64))
    if nc == 2:
        small_first = g.random(n) < 0.5
        # the d_8 form: c.lo < 2^32, s_0 * d_8 with d_8 in {0, 1}, then any product on it
        lo = np.where(small_first, g.integers(0, 2**32, n, dtype=np.uint64), lo)
        pb[:, 0] = np.where(small_first, g.integers(0, 2, n, dtype=np.uint64), pb[:, 0])
        pb[:, 1] = np.where(small_first, pb[:, 1], g.integers(0, 2**10, n, dtype=np.uint64))
    # first rows: the extremes outright (all-ones products on the largest accumulator each form allows)
    X = 16
    pa[:X] = MASK32
    pb[:X] = MASK32
    if not fresh:
        hi[:X] = MASK32 - np.arange(X, dtype=np.uint64) % 2
    if nc == 0:
        lo[:X] = MASK64 - np.arange(X, dtype=np.uint64)
        lo[X - 2:X] = [0, 2**63]
    if nc >= 1:
        lo[:X] = 2**37 - 1
        pb[:X, 0] = 977
    if nc == 2:
        lo[:X] = 2**32 - 1
        pb[:X, 0] = 1
    c = np.stack([lo & np.uint64(MASK32), lo >> np.uint64(32), hi], axis=1).astype(np.uint32)
    return c, pa.astype(np.uint32), pb.astype(np.uint32)


def mac_expected(c, pa, pb, M):
    """(c + sum_{m < M} pa[m] pb[m]) mod 2^96 as (n, 3) uint32, and whether anything carried out of c.lo"""
    p = pa[:, :M].astype(np.uint64) * pb[:, :M].astype(np.uint64)
    s0 = c[:, 0].astype(np.uint64) + (p & np.uint64(MASK32)).sum(axis=1)
    s1 = c[:, 1].astype(np.uint64) + (p >> np.uint64(32)).sum(axis=1) + (s0 >> np.uint64(32))
    s2 = c[:, 2].astype(np.uint64) + (s1 >> np.uint64(32))
    out = np.stack([s0 & np.uint64(MASK32), s1 & np.uint64(MASK32), s2 & np.uint64(MASK32)], axis=1).astype(np.uint32)
    return out, (s1 >> np.uint64(32)) > 0


def mac_nc_bound_holds(c, pa, pb, nc):
    """the first nc products, added one by one to c.lo, never cross 2^64 (the bound every NC call site states)"""
    lo = [int(x) | (int(y) << 32) for x, y in zip(c[:, 0], c[:, 1])]
    for k in range(nc):
        lo = [v + int(x) * int(y) for v, x, y in zip(lo, pa[:, k], pb[:, k])]
        if max(lo) > MASK64:
            return False
    return True
