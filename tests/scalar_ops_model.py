"""Python model of the scalar-field ops (ecgpu_scalar_op_batch / ecgpu_scalar_reduce_batch) and their edge inputs, shared by the
host-twin and the GPU tests.  SQRT restates the reference's algorithms (k256 scalar.rs:290-327, p256 scalar.rs:240-277 Tonelli-Shanks;
p384 scalar.rs:129-... a^((n+1)/4)) so that the root it returns is pinned, not only r^2 = a."""
import random

import field_edge_vectors as V

MUL, SQR, ADD, SUB, NEG, INV, SQRT = range(7)
OPS = {"mul": MUL, "sqr": SQR, "add": ADD, "sub": SUB, "neg": NEG, "inv": INV, "sqrt": SQRT}
BINARY = (MUL, ADD, SUB)
CURVE_INDEX = {"k256": 0, "p256": 1, "p384": 2}
GENERATOR = {"k256": 7, "p256": 7, "p384": 2}          # MULTIPLICATIVE_GENERATOR of each scalar field


def two_adicity(n):
    m = n - 1
    s = (m & -m).bit_length() - 1
    return s, m >> s


def root_of_unity(curve):
    n, _ = V.SCALAR_FIELDS[curve]
    _, t = two_adicity(n)
    return pow(GENERATOR[curve], t, n)


def sqrt_ref(curve, a):
    """(root, is_some) exactly as the reference computes it"""
    n, _ = V.SCALAR_FIELDS[curve]
    S, t = two_adicity(n)
    if S == 1:
        x = pow(a, (n + 1) // 4, n)
        return x, x * x % n == a
    w = pow(a, (t - 1) // 2, n)
    v, x = S, a * w % n
    b, z = x * w % n, root_of_unity(curve)
    for max_v in range(S, 0, -1):
        k, tmp, j_less_than_v = 1, b * b % n, True
        for j in range(2, max_v):
            tmp_is_one = tmp == 1
            squared = (z if tmp_is_one else tmp) ** 2 % n
            tmp = tmp if tmp_is_one else squared
            new_z = squared if tmp_is_one else z
            j_less_than_v = j_less_than_v and j != v
            k = k if tmp_is_one else j
            z = new_z if j_less_than_v else z
        result = x * z % n
        x = x if b == 1 else result
        z = z * z % n
        b = b * z % n
        v = k
    return x, x * x % n == a


def expected(curve, op, a, b=0):
    """(out, ok) of one element"""
    n, _ = V.SCALAR_FIELDS[curve]
    if a >= n or (op in BINARY and b >= n):
        return 0, 0
    if op == MUL:
        return a * b % n, 1
    if op == SQR:
        return a * a % n, 1
    if op == ADD:
        return (a + b) % n, 1
    if op == SUB:
        return (a - b) % n, 1
    if op == NEG:
        return -a % n, 1
    if op == INV:
        return (pow(a, -1, n), 1) if a else (0, 0)
    r, ok = sqrt_ref(curve, a)
    return (r, 1) if ok else (0, 0)


def expected_reduce(curve, x, nonzero):
    n, _ = V.SCALAR_FIELDS[curve]
    return x % (n - 1) + 1 if nonzero else x % n


def edge_values(curve):
    """the issue's scalar edges, valid ones below n, plus n, n + 1 and 2^(32 L) - 1 that must come back rejected"""
    n, L = V.SCALAR_FIELDS[curve]
    vals = [0, 1, 2, n - 2, n - 1, (n - 1) // 2, (n + 1) // 2, 2**32 - 1, 2**(32 * L - 1)] + V.edges(n, L)
    vals += [n, n + 1, 2**(32 * L) - 1]
    out, seen = [], set()
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def edge_pairs(curve, count=None):
    """every pair of edges, the edge pairs of field_edge_vectors (word extremes, near-maximal products) and its quotient-digit
    pairs; pairs with an invalid member included"""
    n, L = V.SCALAR_FIELDS[curve]
    e = edge_values(curve)
    ps = [(x, y) for x in e for y in e] + V.edge_pairs(n, L) + V.quotient_digit_pairs(n, L)
    return ps if count is None else ps[:count]


def okm_inputs(curve, count, seed):
    """FromOkm inputs: 48 (k256, p256) or 72 (p384) uniform bytes, as expand_message produces them; the reference takes
    d0 2^192 + d1 (d0 2^288 + d1), which equals the whole string mod n"""
    rng = random.Random(seed)
    width = 72 if curve == "p384" else 48
    out = []
    for _ in range(count):
        raw = rng.getrandbits(8 * width).to_bytes(width, "big")
        half = width // 2
        d0, d1 = int.from_bytes(raw[:half], "big"), int.from_bytes(raw[half:], "big")
        out.append((raw, d0 * 2**(8 * half) + d1))
    return width, out


def wide_inputs(curve, in_bytes, count, seed):
    """values of in_bytes bytes: extremes, values near multiples of n and n - 1, and random ones"""
    n, _ = V.SCALAR_FIELDS[curve]
    top = 2**(8 * in_bytes)
    rng = random.Random(seed)
    vals = [0, 1, top - 1, top - 2, top // 2, top // 2 - 1]
    for m in (n, n - 1):
        for q in (1, 2, 3, (top - 1) // m, rng.randrange(1, max(2, (top - 1) // m + 1))):
            for d in (-2, -1, 0, 1, 2):
                vals.append(q * m + d)
    vals += [rng.randrange(top) for _ in range(count)]
    return [v for v in vals if 0 <= v < top]
