"""Signatures whose final affine sum A + B is exceptional, and the lift / curve-check inputs of the kernels around the scalar
multiplications (csrc/affine_ops.hpp).  Pure Python on oracle.ecmodel; every expected value is the oracle's verdict.

ECDSA verify, Q = d G, A = u1 G, B = u2 Q:
  same      r = x(2 t G) mod n, s = r d / t, z = r d: u1 G = u2 Q = t G, the tangent - valid
  opp       the same r, s with z = -r d: A = -B, the sum is the identity - invalid
  a_inf     r = x(t G) mod n, s = r d / t, z = 0: A is the identity - valid
  chord     ordinary signatures, valid and with r + 1
  rejected  r = 0 or s = n: ok is already 0 when the check kernel runs
recovery, R = k G, r = x(R), any s:  z = -s k the tangent (a key), z = s k the identity (none), z = 0 A at infinity.
BIP340 in the challenge form (e is an input), P = d G of even y, R = s G + (-e) P:
  same      s = -e d with 2 s G of even y, r its x - valid;  opp  s = e d - invalid;  b_inf  e = 0, r = x(s G) of even y - valid
  no_root   a key x without a curve point;  r_ge_p  r = p.

Layout: the batched kernels give lane l of a launch with T lanes the elements l, l + T, l + 2 T, ..; T = 256 up to 4096 elements.
N = 4 * 256 + 7 rows, so lanes 0 .. 6 hold five.  MIXED lanes hold one element of every kind, rotated from lane to lane: an
exceptional element that entered the lane's prefix product (a zero denominator, or an operand of the identity) would spoil the lane's
valid elements.  rows(..)[:257] and [:1] keep lane 0's mix: its first element is a tangent."""
import functools
import hashlib
import random
from collections import namedtuple

from oracle import ecmodel as M

T = 256
N = 4 * T + 7
SIZES = (1, 257, N)
MIXED = [0] + [5 + 21 * k for k in range(12)]           # lanes with one element of every kind; every wave has three
KINDS4 = ("same", "opp", "inf", "chord")                # "inf": a_inf (ECDSA, recovery) or b_inf (BIP340)
EXCEPTIONAL = ("same", "opp", "inf")

Row = namedtuple("Row", "cls inputs A B want")          # A, B: the two products (None = identity); want: the oracle's verdict


def layout():
    """class of each of the N elements"""
    cls = [("chord_bad" if i % 3 == 0 else "chord") for i in range(N)]
    for k, lane in enumerate(MIXED):
        for b in range(4):
            cls[lane + T * b] = KINDS4[(b + k) % 4]
        cls[lane + 1 + T * (k % 4)] = "rejected"
    cls[0 + 4 * T] = "same"                             # lanes 0 .. 6: a fifth element
    cls[3 + 4 * T] = "opp"
    cls[4 + 4 * T] = "inf"
    return cls


COUNTS = {"same": 14, "opp": 14, "inf": 14, "rejected": 13}
COUNTS["chord_bad"] = sum(1 for c in layout() if c == "chord_bad")
COUNTS["chord"] = N - sum(COUNTS.values())


def _G(c):
    return (c.gx, c.gy)


def _low(c, s):
    """s as the curve's verifier wants it: the low half on secp256k1"""
    return c.n - s if c.name == "k256" and s > c.n // 2 else s


def _mulG(c, k):
    return M.affine_mul(c, k, _G(c))


# ---------------------------------------------------------------------------------------------------------------------------------
# ECDSA verify
# ---------------------------------------------------------------------------------------------------------------------------------
def _ecdsa_row(c, cls, d, Q, z, r, s):
    low = c.name == "k256"
    want = M.ecdsa_verify_prehashed(c, Q, z, r, s, reject_high_s=low)
    A = B = None
    if 0 < r < c.n and 0 < s < c.n and not (low and s > c.n // 2):
        w = pow(s, -1, c.n)
        A, B = _mulG(c, M.b2i(z) % c.n * w % c.n), M.affine_mul(c, r * w % c.n, Q)
    return Row(cls, (z, M.i2b(c, r) + M.i2b(c, s), M.i2b(c, Q[0]) + M.i2b(c, Q[1])), A, B, want)


@functools.lru_cache(maxsize=None)
def ecdsa_rows(cn):
    c = M.CURVES[cn]
    rng = random.Random("ecdsa-edges-" + cn)
    n = c.n
    pool = {"chord": [], "chord_bad": []}
    for _ in range(8):
        d, k, z = rng.randrange(1, n), rng.randrange(1, n), rng.randbytes(c.nbytes)
        r, s, _ = M.ecdsa_sign_prehashed(c, d, k, z, normalize_s=(cn == "k256"))
        Q = _mulG(c, d)
        pool["chord"].append(_ecdsa_row(c, "chord", d, Q, z, r, s))
        pool["chord_bad"].append(_ecdsa_row(c, "chord_bad", d, Q, z, r % (n - 1) + 1, s))
    rows, seen = [], {}
    for i, cls in enumerate(layout()):
        if cls in pool:
            rows.append(pool[cls][seen.setdefault(cls, 0) % 8])
            seen[cls] += 1
            continue
        d, t = rng.randrange(1, n), rng.randrange(1, n)
        Q = _mulG(c, d)
        if cls in ("same", "opp", "rejected"):
            r = _mulG(c, 2 * t)[0] % n
            z = r * d % n if cls != "opp" else (-r * d) % n
        else:
            r, z = _mulG(c, t)[0] % n, 0
        s = _low(c, r * d * pow(t, -1, n) % n)
        if cls == "rejected":
            r, s = ((0, s), (r, n))[i % 2]
        rows.append(_ecdsa_row(c, cls, d, Q, M.i2b(c, z), r, s))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# recovery
# ---------------------------------------------------------------------------------------------------------------------------------
def _recover_row(c, cls, z, r, s, recid):
    low = c.name == "k256"
    want = M.ecdsa_recover_prehashed(c, z, r, s, recid, reject_high_s=low)
    A = B = None
    R = M.decompress(c, r, recid & 1) if recid < 2 else None
    if 0 < r < c.n and 0 < s < c.n and not (low and s > c.n // 2) and R is not None:
        ri = pow(r, -1, c.n)
        A, B = _mulG(c, -(ri * (M.b2i(z) % c.n)) % c.n), M.affine_mul(c, ri * s % c.n, R)
    return Row(cls, (z, M.i2b(c, r) + M.i2b(c, s), recid), A, B, want)


@functools.lru_cache(maxsize=None)
def recover_rows(cn):
    c = M.CURVES[cn]
    rng = random.Random("recover-edges-" + cn)
    n = c.n
    pool = {"chord": [], "chord_bad": []}
    for _ in range(8):
        d, k, z = rng.randrange(1, n), rng.randrange(1, n), rng.randbytes(c.nbytes)
        r, s, rid = M.ecdsa_sign_prehashed(c, d, k, z, normalize_s=(cn == "k256"))
        pool["chord"].append(_recover_row(c, "chord", z, r, s, rid))
        pool["chord_bad"].append(_recover_row(c, "chord_bad", z, r, s, rid ^ 1))     # the other root: another key, still a chord
    rows, seen = [], {}
    for i, cls in enumerate(layout()):
        if cls in pool:
            rows.append(pool[cls][seen.setdefault(cls, 0) % 8])
            seen[cls] += 1
            continue
        k, s = rng.randrange(1, n), _low(c, rng.randrange(1, n))
        R = _mulG(c, k)
        r, rid = R[0], R[1] & 1
        assert r < n
        z = {"same": -s * k % n, "rejected": -s * k % n, "opp": s * k % n, "inf": 0}[cls]
        if cls == "rejected":
            r, rid = ((0, rid), (r, 4))[i % 2]
        rows.append(_recover_row(c, cls, M.i2b(c, z), r, s, rid))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# BIP340, challenge form
# ---------------------------------------------------------------------------------------------------------------------------------
def bip340_verdict(px: bytes, sig: bytes, e: bytes):
    """(valid, A, B) of the EC part of BIP340 verification from the challenge hash: affine_add and the rules of the BIP"""
    c = M.K256
    x, r, s = M.b2i(px), M.b2i(sig[:32]), M.b2i(sig[32:])
    P = M.decompress(c, x, 0)
    if P is None or not (0 < r < c.p) or not (0 < s < c.n):
        return False, None, None
    A, B = _mulG(c, s), M.affine_mul(c, -(M.b2i(e) % c.n) % c.n, P)
    R = M.affine_add(c, A, B)
    return R is not None and R[1] % 2 == 0 and R[0] == r, A, B


def _even_key(c, rng):
    d = rng.randrange(1, c.n)
    P = _mulG(c, d)
    return (c.n - d, (P[0], c.p - P[1])) if P[1] & 1 else (d, P)


def _schnorr_row(cls, px, sig, e):
    want, A, B = bip340_verdict(px, sig, e)
    return Row(cls, (px, sig, e), A, B, want)


@functools.lru_cache(maxsize=None)
def schnorr_rows():
    c = M.K256
    rng = random.Random("bip340-edges")
    n = c.n
    tob = lambda v: M.i2b(c, v)
    pool = {"chord": [], "chord_bad": []}
    for _ in range(8):
        sk, msg, aux = tob(rng.randrange(1, n)), rng.randbytes(32), rng.randbytes(32)
        sig, px = M.schnorr_sign_prehash(sk, msg, aux)
        e = M._tagged_hash(b"BIP0340/challenge", sig[:32], px, msg)
        assert M.schnorr_verify_prehash(px, msg, sig)
        pool["chord"].append(_schnorr_row("chord", px, sig, e))
        pool["chord_bad"].append(_schnorr_row("chord_bad", px, sig[:63] + bytes([sig[63] ^ 4]), e))
    x_no_root = next(x for x in range(1, 100) if M.decompress(c, x, 0) is None)
    rows, seen = [], {}
    for i, cls in enumerate(layout()):
        if cls in pool:
            rows.append(pool[cls][seen.setdefault(cls, 0) % 8])
            seen[cls] += 1
            continue
        d, P = _even_key(c, rng)
        while True:
            e = rng.randrange(1, n) if cls != "inf" else 0
            s = {"same": -e * d % n, "rejected": -e * d % n, "opp": e * d % n, "inf": rng.randrange(1, n)}[cls]
            R = _mulG(c, 2 * s if cls in ("same", "rejected") else s)
            if R[1] % 2 == 0:
                break
        px, r = tob(P[0]), R[0]
        if cls == "rejected":                               # would be valid but for the key or the range of r
            px, r = ((tob(x_no_root), r), (px, c.p))[i % 2]
        rows.append(_schnorr_row(cls, px, tob(r) + tob(s), tob(e)))
    return rows


def rows(cn, kind):
    return {"ecdsa": ecdsa_rows, "recover": recover_rows}[kind](cn) if kind != "schnorr" else schnorr_rows()


def class_counts(rs):
    out = {}
    for r in rs:
        out[r.cls] = out.get(r.cls, 0) + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# y from x, canonical and on the curve
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lift_rows(cn):
    """[(x, y_is_odd)]: x with and without a root at both parities, p - 1, 0, x >= p"""
    c = M.CURVES[cn]
    rng = random.Random("lift-" + cn)
    xs = [rng.randrange(c.p) for _ in range(24)] + [c.p - 1, 0, 1, 2, 3, c.p, c.p + 1, c.p + 5, (1 << (8 * c.nbytes)) - 1]
    out = [(x, o) for x in xs for o in (0, 1)]
    has = [M.decompress(c, x, o) is not None for x, o in out]
    assert has.count(True) >= 16 and has.count(False) >= 16
    return out


@functools.lru_cache(maxsize=None)
def curve_check_rows(cn):
    """[(x, y, canonical and on the curve)]: points, y off by one, and aliases x + p, y + p of points with small coordinates, which
    satisfy the equation mod p; (0, 0) is not on any of the curves (the callers' identity policy is theirs)"""
    c = M.CURVES[cn]
    rng = random.Random("oncurve-" + cn)
    top = 1 << (8 * c.nbytes)
    pts = []
    while len(pts) < 12:
        P = M.decompress(c, rng.randrange(c.p), rng.randrange(2))
        if P is not None:
            pts.append(P)
    out = [(x, y, True) for x, y in pts] + [(x, y ^ 1, False) for x, y in pts[:6]] + [(x ^ 1, y, False) for x, y in pts[6:]]
    small = [P for P in (M.decompress(c, x, o) for x in range(1, 40) for o in (0, 1)) if P is not None]
    out += [(x + c.p, y, False) for x, y in small[:6]]
    ys = sorted((P for P in small), key=lambda P: P[1])[:4]
    out += [(x, y + c.p, False) for x, y in ys if y + c.p < top]
    out += [(c.p, 0, False), (0, c.p, False), (0, 0, False), (c.p - 1, c.p - 1, False)]
    assert all(x < top and y < top for x, y, _ in out)
    for x, y, ok in out:
        assert ok == (x < c.p and y < c.p and M.on_curve(c, (x, y)))
    return out
