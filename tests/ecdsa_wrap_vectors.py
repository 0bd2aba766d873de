"""ECDSA where x(R) lies in [n, p): the second candidate r + n of verification, recovery ids 2 and 3, and x_reduced of signing.
Pure Python on oracle.ecmodel; every expected value is the oracle's.

p > n on all three curves, so R can have n <= x(R) < p; then r = x(R) - n, and the code that handles it (csrc/ecdsa_kernels.hpp:
`second` of verify_check_kernel, `recid & 2` of recover_prep_kernel, `x_reduced` of sign_finish_kernel) runs for no R = k G that a
search finds: p - n is 2^129 (secp256k1), 2^127 (P-256), 2^190 (P-384).  Such signatures are constructed instead: lift an x in
[n, p) to R, choose any s and z, set r = x - n and Q = r^-1 (s R - z G); (z, r, s) verifies under Q, and Q is what recovery
returns for the recovery id 2 | parity(y_R).  With W = 2^(8 nbytes) and x' a small on-curve x:

verify (z, r || s, Q -> valid):
  wrap           x(R) = r + n at each anchor of [n, p), both parities of y_R                                        valid
  wrap_ainf      the same with z = 0 and z = n (the bytes of n reduce to 0): A is the identity, the operand arm      valid
  wrap_bad       a wrap row with r + 1 and r - 1                                                                     invalid
  no_p_check     x(R) = x', r = x' + p - n: r + n = p + x', accepted by an addition in the field or without r2 < p   invalid
  dropped_carry  x(R) = x', r = x' + W - n: r + n = W + x', accepted where the carry is ignored                      invalid
  first_small    x(R) = r with r + n < p: valid by the first candidate while `second` is true                        valid
  r_is_x         a wrap row with r replaced by x(R) >= n: the range check                                            invalid
  z_edge         wrap rows with z = n - 1, n + 1, W - 1: reduce_once on the prehash                                  valid
  chord, chord_bad, rejected   ordinary valid, ordinary invalid, r = 0 or s = n
recovery (z, r || s, recid -> key or None):
  wrap           recid 2 | parity, z random / 0 / n                          the key
  wrong_parity   the other parity                                            the other key
  ge_p           r = p - n + j (r + n >= p), j = 0 and the x' among them     None
  carry          r = W - n + j                                               None
  no_root        r = j with n + j not on the curve                           None
  recid_4_7      a wrap r with recid 4 .. 7                                  None
  high_s         a wrap row with s in the high half                          None on secp256k1, the other key elsewhere
  chord_bit1     ordinary rows with bit 1 of the recid set                   the oracle's verdict
  chord, chord_bad, rejected   ordinary rows with recid 0 / 1, the other root, r = 0 or s = n
sign_finish and verify_check rows for the device twin (tests/devtwin/devtwin_ecdsa.hip): sign_rows, check_rows below.

Layout: as tests/signature_edge_vectors.py.  The batched kernels give lane l of a launch with T lanes the rows l, l + T, ..; T = 256
up to 4096 rows, so of N = 4 * 256 + 7 rows a lane holds four, lanes 0 .. 6 five.  A lane therefore cannot hold all eight classes
of a family: each of the thirteen MIXED lanes holds four different ones, rotated so that the MIXED lanes together hold every class
at least six times and each holds a valid row and an invalid one, and its neighbour lane holds a rejected row; elsewhere every eleventh row takes the classes in turn, so that
the whole pool is used; the other rows are ordinary, every third one invalid.  A wrong
element that leaked into a lane's shared inversion would spoil the lane's other rows.  rows[:257] and [:1] keep lane 0's mix: its
first row is a wrap row.  Rows come from a pool of POOL distinct rows per class, tiled."""
import functools
import itertools
import random
from collections import Counter, namedtuple

from oracle import ecmodel as M

T = 256
N = 4 * T + 7
SIZES = (1, 257, N)
MIXED = [0] + [5 + 21 * k for k in range(12)]
POOL = 8
LOW_S = 2                                               # ecgpu.ECDSA_LOW_S

VERIFY_CLASSES = ("wrap", "wrap_ainf", "wrap_bad", "no_p_check", "dropped_carry", "first_small", "r_is_x", "z_edge")
RECOVER_CLASSES = ("wrap", "ge_p", "carry", "no_root", "wrong_parity", "recid_4_7", "high_s", "chord_bit1")
SIGN_CLASSES = ("wrap", "x_eq_n", "wrap_low_s", "s_zero", "wrap", "r_inf", "wrap_low_s", "k_bad")
VERIFY_VALID = ("wrap", "wrap_ainf", "first_small", "z_edge", "chord")


def layout(exc, fill=("chord_bad", "chord", "chord"), rejected="rejected"):
    """class of each of the N rows; exc: the eight classes of the family"""
    cls = [fill[i % 3] if i % 11 != 7 else exc[i // 11 % 8] for i in range(N)]      # every eleventh row: the classes in turn
    for k, lane in enumerate(MIXED):
        for b in range(4):
            cls[lane + T * b] = exc[(k + 3 * b) % 8]
        cls[lane + 1 + T * (k % 4)] = rejected
    for j in range(7):                                  # lanes 0 .. 6: a fifth row
        cls[4 * T + j] = exc[(j + 4) % 8]
    return cls


def class_counts(rs):
    return dict(Counter(r.cls for r in rs))


# the exact number of rows of each class among the N
VERIFY_COUNTS = {"wrap": 18, "wrap_ainf": 18, "wrap_bad": 20, "no_p_check": 18, "dropped_carry": 20, "first_small": 18, "r_is_x": 17, "z_edge": 18,
                 "rejected": 13, "chord_bad": 292, "chord": 579}
RECOVER_COUNTS = {"wrap": 18, "wrong_parity": 20, "ge_p": 18, "carry": 20, "no_root": 18, "recid_4_7": 18, "high_s": 17, "chord_bit1": 18,
                  "rejected": 13, "chord_bad": 292, "chord": 579}
SIGN_COUNTS = {"wrap": 38, "wrap_low_s": 37, "x_eq_n": 18, "s_zero": 18, "r_inf": 18, "k_bad": 31, "control": 871}     # P-256: x_eq_n rows are wrap rows
assert dict(Counter(layout(VERIFY_CLASSES))) == VERIFY_COUNTS and dict(Counter(layout(RECOVER_CLASSES))) == RECOVER_COUNTS
assert dict(Counter(layout(SIGN_CLASSES, ("control",) * 3, "k_bad"))) == SIGN_COUNTS


# ---------------------------------------------------------------------------------------------------------------------------------
# anchors
# ---------------------------------------------------------------------------------------------------------------------------------
Anchors = namedtuple("Anchors", "n_on_curve lo mid hi xs0 xs1")     # lo, mid, hi: on-curve x in (n, p); xs0 >= 0, xs1 >= 1: small ones
# (n on the curve, lo - n, hi - p, xs0): what the searches must find
ANCHOR_TABLE = {"k256": (True, 2, -3, 1), "p256": (False, 3, -3, 0), "p384": (True, 2, -1, 0)}


@functools.lru_cache(maxsize=None)
def anchors(cn):
    c = M.CURVES[cn]
    on = lambda x: M.decompress(c, x, 0) is not None
    up = lambda x: next(v for v in itertools.count(x) if on(v))
    a = Anchors(on(c.n), up(c.n + 1), up(c.n + (c.p - c.n) // 2), next(v for v in itertools.count(c.p - 1, -1) if on(v)), up(0), up(1))
    assert c.n < a.lo < a.mid < a.hi < c.p and a.xs0 <= a.xs1 < c.p - c.n
    assert (a.n_on_curve, a.lo - c.n, a.hi - c.p, a.xs0) == ANCHOR_TABLE[cn]
    return a


def wrap_points(cn):
    """R at the three anchors of [n, p), both parities of y"""
    c, a = M.CURVES[cn], anchors(cn)
    return [M.decompress(c, x, o) for x in (a.lo, a.mid, a.hi) for o in (0, 1)]


def small_points(cn):
    """R at the small anchors x', both parities"""
    c, a = M.CURVES[cn], anchors(cn)
    return [M.decompress(c, x, o) for x in sorted({a.xs0, a.xs1}) for o in (0, 1)]


def _G(c):
    return (c.gx, c.gy)


def _mulG(c, k):
    return M.affine_mul(c, k, _G(c))


def _W(c):
    return 1 << (8 * c.nbytes)


def _s(c, rng):
    """a random s; on secp256k1 in the low half"""
    return rng.randrange(1, c.n // 2 + 1) if c.name == "k256" else rng.randrange(1, c.n)


def key_for(c, R, r, s, z):
    """Q = r^-1 (s R - z G): the key under which (z, r, s) leads verification to R"""
    ri = pow(r, -1, c.n)
    Q = M.affine_add(c, M.affine_mul(c, s * ri % c.n, R), _mulG(c, -(M.b2i(z) % c.n) * ri % c.n))
    assert Q is not None
    return Q


def _ordinary(c, rng):
    d, k, z = rng.randrange(1, c.n), rng.randrange(1, c.n), rng.randbytes(c.nbytes)
    r, s, rid = M.ecdsa_sign_prehashed(c, d, k, z, normalize_s=(c.name == "k256"))
    return _mulG(c, d), z, r, s, rid


def _tile(classes, pool):
    seen = Counter()
    rows = []
    for cls in classes:
        rows.append(pool[cls][seen[cls] % len(pool[cls])])
        seen[cls] += 1
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# ECDSA verify
# ---------------------------------------------------------------------------------------------------------------------------------
VRow = namedtuple("VRow", "cls inputs R want")          # inputs: z, r || s, Q; R: the point the row is built on (None: a control)


def _vrow(c, cls, R, z, r, s, Q):
    want = M.ecdsa_verify_prehashed(c, Q, z, r, s, reject_high_s=(c.name == "k256"))
    return VRow(cls, (z, M.i2b(c, r) + M.i2b(c, s), M.i2b(c, Q[0]) + M.i2b(c, Q[1])), R, want)


def second(c, row):
    """`second` of verify_check_kernel for the row's r: r + n does not carry and is below p"""
    return M.b2i(row.inputs[1][:c.nbytes]) + c.n < c.p


def sum_point(c, row):
    """(A, B) = (u1 G, u2 Q) of a row whose r and s are in range, by the oracle"""
    z, sig, q = row.inputs
    nb = c.nbytes
    r, s = M.b2i(sig[:nb]), M.b2i(sig[nb:])
    w = pow(s, -1, c.n)
    return _mulG(c, M.b2i(z) % c.n * w % c.n), M.affine_mul(c, r * w % c.n, (M.b2i(q[:nb]), M.b2i(q[nb:])))


@functools.lru_cache(maxsize=None)
def verify_pool(cn):
    c, a = M.CURVES[cn], anchors(cn)
    rng = random.Random("ecdsa-wrap-verify-" + cn)
    n, p, W, tob = c.n, c.p, _W(c), lambda v: M.i2b(c, v)
    wp, sp = wrap_points(cn), small_points(cn)
    pool = {cls: [] for cls in VERIFY_CLASSES + ("chord", "chord_bad", "rejected")}
    for i in range(POOL):
        R = wp[i % 6]
        r = R[0] - n
        s, z = _s(c, rng), rng.randbytes(c.nbytes)
        Q = key_for(c, R, r, s, z)
        pool["wrap"].append(_vrow(c, "wrap", R, z, r, s, Q))
        pool["wrap_bad"].append(_vrow(c, "wrap_bad", R, z, r + (1, -1)[(i + i // 6) % 2], s, Q))
        pool["r_is_x"].append(_vrow(c, "r_is_x", R, z, R[0], s, Q))
        z = tob((0, n)[i // 6])
        pool["wrap_ainf"].append(_vrow(c, "wrap_ainf", R, z, r, s, key_for(c, R, r, s, z)))
        z = tob((n - 1, n + 1, W - 1)[(i + i // 6) % 3])
        pool["z_edge"].append(_vrow(c, "z_edge", R, z, r, s, key_for(c, R, r, s, z)))
        R = sp[i % len(sp)]
        s, z = _s(c, rng), rng.randbytes(c.nbytes)
        for cls, r in (("no_p_check", R[0] + p - n), ("dropped_carry", R[0] + W - n)):
            pool[cls].append(_vrow(c, cls, R, z, r, s, key_for(c, R, r, s, z)))
        # x(R) = r below p - n: the smallest x >= 1, then random ones
        R = M.decompress(c, a.xs1, i) if i < 2 else next(P for P in (M.decompress(c, rng.randrange(1, p - n), i) for _ in itertools.count()) if P)
        pool["first_small"].append(_vrow(c, "first_small", R, z, R[0], s, key_for(c, R, R[0], s, z)))
    for i in range(8):
        Q, z, r, s, _ = _ordinary(c, rng)
        pool["chord"].append(_vrow(c, "chord", None, z, r, s, Q))
        pool["chord_bad"].append(_vrow(c, "chord_bad", None, z, r % (n - 1) + 1, s, Q))
        pool["rejected"].append(_vrow(c, "rejected", None, z, *((0, s), (r, n))[i % 2], Q))
    return pool


@functools.lru_cache(maxsize=None)
def verify_rows(cn):
    return _tile(layout(VERIFY_CLASSES), verify_pool(cn))


# ---------------------------------------------------------------------------------------------------------------------------------
# recovery
# ---------------------------------------------------------------------------------------------------------------------------------
RRow = namedtuple("RRow", "cls inputs R want")          # inputs: z, r || s, recid; want: the key (x, y) or None


def _rrow(c, cls, R, z, r, s, recid):
    want = M.ecdsa_recover_prehashed(c, z, r, s, recid, reject_high_s=(c.name == "k256"))
    return RRow(cls, (z, M.i2b(c, r) + M.i2b(c, s), recid), R, want)


@functools.lru_cache(maxsize=None)
def recover_pool(cn):
    c, a = M.CURVES[cn], anchors(cn)
    rng = random.Random("ecdsa-wrap-recover-" + cn)
    n, p, W, tob = c.n, c.p, _W(c), lambda v: M.i2b(c, v)
    wp = wrap_points(cn)
    no_root = [j for j in range(1, 64) if M.decompress(c, n + j, 0) is None][:POOL]
    ge_p = sorted({0, a.xs0, a.xs1} | set(range(POOL)))[:POOL]
    pool = {cls: [] for cls in RECOVER_CLASSES + ("chord", "chord_bad", "rejected")}
    for i in range(POOL):
        R = wp[i % 6]
        r, rid = R[0] - n, 2 | (R[1] & 1)
        s = _s(c, rng)
        z = (rng.randbytes(c.nbytes), tob(0), tob(n))[(i + i // 6) % 3]
        pool["wrap"].append(_rrow(c, "wrap", R, z, r, s, rid))
        pool["wrong_parity"].append(_rrow(c, "wrong_parity", R, z, r, s, rid ^ 1))
        pool["recid_4_7"].append(_rrow(c, "recid_4_7", R, z, r, s, 4 + (i + i // 6) % 4))
        pool["high_s"].append(_rrow(c, "high_s", R, z, r, s if s > n // 2 else n - s, rid))
        s, z = _s(c, rng), rng.randbytes(c.nbytes)
        pool["ge_p"].append(_rrow(c, "ge_p", None, z, p - n + ge_p[i], s, 2 | (i & 1)))
        pool["carry"].append(_rrow(c, "carry", None, z, W - n + i, s, 2 | (i & 1)))
        pool["no_root"].append(_rrow(c, "no_root", None, z, no_root[i], s, 2 | (i & 1)))
    for i in range(POOL):
        _, z, r, s, rid = _ordinary(c, rng)
        pool["chord"].append(_rrow(c, "chord", None, z, r, s, rid))
        pool["chord_bad"].append(_rrow(c, "chord_bad", None, z, r, s, rid ^ 1))
        pool["chord_bit1"].append(_rrow(c, "chord_bit1", None, z, r, s, rid | 2))
        pool["rejected"].append(_rrow(c, "rejected", None, z, *((0, s), (r, n))[i % 2], rid))
    return pool


@functools.lru_cache(maxsize=None)
def recover_rows(cn):
    return _tile(layout(RECOVER_CLASSES), recover_pool(cn))


def rows(cn, kind):
    return {"verify": verify_rows, "recover": recover_rows}[kind](cn)


# ---------------------------------------------------------------------------------------------------------------------------------
# message-level rows: z is the digest of a random message
# ---------------------------------------------------------------------------------------------------------------------------------
MRow = namedtuple("MRow", "cls msg sig Q recid valid key")      # valid, key: the oracle's verdict and recovered key on digest(msg)


def msg_rows(cn, name, digest, count=64):
    """count rows wrap / wrap_bad / no_p_check in turn; digest: bytes -> bytes of the field's size"""
    c = M.CURVES[cn]
    rng = random.Random("ecdsa-wrap-msg-" + cn + name)
    wp, sp = wrap_points(cn), small_points(cn)
    low = cn == "k256"
    out = []
    for i in range(count):
        cls = ("wrap", "wrap_bad", "no_p_check")[i % 3]
        msg = rng.randbytes(rng.randrange(0, 200))
        z = M.bits2field(c, digest(msg))
        R = sp[i % len(sp)] if cls == "no_p_check" else wp[i % 6]
        r = R[0] + c.p - c.n if cls == "no_p_check" else R[0] - c.n
        s = _s(c, rng)
        Q = key_for(c, R, r, s, z)
        if cls == "wrap_bad":
            r += (1, -1)[(i // 3) % 2]
        rid = 2 | (R[1] & 1)
        out.append(MRow(cls, msg, M.i2b(c, r) + M.i2b(c, s), M.i2b(c, Q[0]) + M.i2b(c, Q[1]), rid,
                        M.ecdsa_verify_prehashed(c, Q, z, r, s, reject_high_s=low), M.ecdsa_recover_prehashed(c, z, r, s, rid, reject_high_s=low)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# sign_finish: d, k, z, R, r_inf, flags -> r || s, recid, ok
# ---------------------------------------------------------------------------------------------------------------------------------
def sign_finish_model(c, d, k, z, R, r_inf, low_s):
    """the body of M.ecdsa_sign_prehashed with R supplied -> (r, s, recovery id) or None"""
    n = c.n
    if not (0 < k < n and 0 < d < n) or r_inf:
        return None
    e = M.b2i(z) % n
    r = R[0] % n
    s = pow(k, -1, n) * (e + r * d) % n
    if r == 0 or s == 0:
        return None
    y_odd = R[1] & 1
    x_reduced = 1 if R[0] >= n else 0
    if low_s and s > n // 2:
        s = n - s
        y_odd ^= 1
    return r, s, y_odd | (x_reduced << 1)


SRow = namedtuple("SRow", "cls d k z R r_inf want")     # want: {flags: (r, s, recid) or None} for flags 0 and LOW_S


def _srow(c, cls, d, k, z, R, r_inf=0):
    R = (0, 0) if r_inf else R
    return SRow(cls, d, k, z, R, r_inf, {f: sign_finish_model(c, d, k, z, R, r_inf, bool(f)) for f in (0, LOW_S)})


def sign_classes(cn):
    """x(R) = n needs n on the curve"""
    return tuple(cls if cls != "x_eq_n" or anchors(cn).n_on_curve else "wrap" for cls in SIGN_CLASSES)


@functools.lru_cache(maxsize=None)
def sign_pool(cn):
    """wrap: R at the anchors with k chosen so that s = k^-1 (z + r d) is in the low half, wrap_low_s: in the high half, where LOW_S
    negates s and flips the parity bit: together recovery ids 2 and 3, both from either parity"""
    c = M.CURVES[cn]
    rng = random.Random("ecdsa-wrap-sign-" + cn)
    n = c.n
    wp = wrap_points(cn)
    pool = {cls: [] for cls in SIGN_CLASSES + ("control",)}
    ctl = []
    while len(ctl) < POOL:
        P = M.decompress(c, rng.randrange(1, n), len(ctl))
        if P:
            ctl.append(P)
    for i in range(POOL):
        R = wp[i % 6]
        d, z = rng.randrange(1, n), rng.randbytes(c.nbytes)
        num = (M.b2i(z) + R[0] % n * d) % n
        for cls, high in (("wrap", False), ("wrap_low_s", True)):
            s = rng.randrange(n // 2 + 1, n) if high else rng.randrange(1, n // 2 + 1)
            pool[cls].append(_srow(c, cls, d, num * pow(s, -1, n) % n, z, R))
        k = rng.randrange(1, n)
        if anchors(cn).n_on_curve:
            pool["x_eq_n"].append(_srow(c, "x_eq_n", d, k, z, M.decompress(c, n, i)))
        Rz = (R, ctl[i])[i % 2]
        pool["s_zero"].append(_srow(c, "s_zero", d, k, M.i2b(c, -(Rz[0] % n) * d % n), Rz))
        pool["r_inf"].append(_srow(c, "r_inf", d, k, z, None, 1))
        pool["k_bad"].append(_srow(c, "k_bad", d, (0, n)[i % 2], z, R))
        pool["control"].append(_srow(c, "control", d, k, z, ctl[i]))
    return pool


@functools.lru_cache(maxsize=None)
def sign_rows(cn):
    return _tile(layout(sign_classes(cn), ("control",) * 3, "k_bad"), sign_pool(cn))


# ---------------------------------------------------------------------------------------------------------------------------------
# verify_check: A, a_inf, B, b_inf, r || s, ok_in -> ok
# ---------------------------------------------------------------------------------------------------------------------------------
CHECK_KINDS = ("tangent", "chord", "a_inf", "b_inf", "opp")
CHECK_CLASSES = ("wrap", "wrap_bad", "no_p_check", "dropped_carry", "first_small", "ok_in_0")


def check_model(c, A, B, r, ok_in):
    """x(A + B) mod n == r, for a row not rejected before"""
    S = M.affine_add(c, A, B)
    return bool(ok_in) and S is not None and S[0] % c.n == r


CRow = namedtuple("CRow", "cls kind A B r ok_in want")  # A, B: (x, y) or None for the identity


@functools.lru_cache(maxsize=None)
def check_pool(cn):
    """every point of wrap_points and small_points as a sum of each kind - tangent: A = B = ((n + 1) / 2) R; chord: A random,
    B = R - A; a_inf, b_inf: the other operand is R; opp: A = R, B = -R, the identity, which has no x - under every r its class names"""
    c = M.CURVES[cn]
    rng = random.Random("ecdsa-wrap-check-" + cn)
    n, p, W = c.n, c.p, _W(c)
    out = []

    def sums(R):
        H = M.affine_mul(c, (n + 1) // 2, R)
        A = _mulG(c, rng.randrange(1, n))
        got = {"tangent": (H, H), "chord": (A, M.affine_add(c, R, M.affine_neg(c, A))), "a_inf": (None, R), "b_inf": (R, None),
               "opp": (R, M.affine_neg(c, R))}
        assert all(M.affine_add(c, *got[k]) == R for k in CHECK_KINDS[:4]) and M.affine_add(c, *got["opp"]) is None
        return got

    def add(cls, kind, AB, r, ok_in=1):
        out.append(CRow(cls, kind, AB[0], AB[1], r, ok_in, check_model(c, AB[0], AB[1], r, ok_in)))

    for R in wrap_points(cn):
        for kind, AB in sums(R).items():
            r = R[0] - n
            add("wrap", kind, AB, r)
            add("wrap_bad", kind, AB, r + 1)
            add("wrap_bad", kind, AB, r - 1)
            add("ok_in_0", kind, AB, r, 0)
    for R in small_points(cn):
        for kind, AB in sums(R).items():
            add("no_p_check", kind, AB, R[0] + p - n)
            add("dropped_carry", kind, AB, R[0] + W - n)
            if R[0] >= 1:
                add("first_small", kind, AB, R[0])
    return out


def check_rows(cn, size):
    pool = check_pool(cn)
    return [pool[i % len(pool)] for i in range(size)]
