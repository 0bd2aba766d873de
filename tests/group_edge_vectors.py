"""Operand pairs for the point formulas one at a time (tests/devtwin/group_ops.hpp), as integers, with the class of each pair and
the affine points it stands for, so that the expected result is oracle.ecmodel.affine_add / affine_neg on Python integers.  Pure
Python: nothing here depends on the library or on its host build.

Classes (Row.cls), per curve and op where the op can take them:
    ordinary            random distinct points, random denominators (a different one for each operand)
    p_inf, q_inf, both_inf, and for secp256k1 the same with the denominator given as raw p instead of raw 0 (":rawp")
    same:z=.., opp:z=.. the same point / opposite points with the first denominator 1, 2, p - 1, random; ":q1" the second one 1
    noncanon:C:lo|hi    secp256k1: coordinate C of the first operand (or the affine x of the second, C = qx) is congruent to a value
                        t < 2^32 + 977 and given as t (lo) or as t + p (hi, still below 2^256); ":same" on the same point
    near:+t, near:-t    distinct points whose H (or P of the XYZZ forms) is +-t for a small t in the field's internal form: the top
                        word passes the prefilter of is_zero_fast, the exact test behind it must say "not zero"
    mask:e=.:zd=.       the masked forms with every combination of the `empty` and zero-digit masks; ":inf" with the accumulator
                        all zero (what `empty` stands for in the kernels), ":same" / ":opp" where the unmasked formula would be exceptional
Row.branch says which exceptional branch of the formula the pair must reach (None: the ordinary path), Row.z1 whether the first
operand's denominator is one; tests/test_hosttwin_group_edges.py checks both against the ECGPU_EXC_NOTE counters.

layouts(rows) lays the same rows out in three lane orders: sorted by class and padded to whole waves of 64, interleaved so that
neighbouring lanes differ in class, and one exceptional lane (at 0, 31, 32, 63) in a wave of ordinary ones."""
import functools
import random
from collections import namedtuple

import numpy as np

from oracle import ecmodel as M

WAVE = 64
MAX_CALL = 1 << 13
IN_FE, OUT_FE, AUX = 4, 5, 2
ONES = 0xFFFFFFFF
K256_SMALL = (1 << 32) + 977            # t below this: t + p < 2^256

Row = namedtuple("Row", "cls p q aux Pa Qa branch z1")
# name: (code in twin::PtOp, form of p, form of q, kind, curves)
OpSpec = namedtuple("OpSpec", "code pform qform kind curves")
ALL, NIST, K = ("k256", "p256", "p384"), ("p256", "p384"), ("k256",)
OPS = {
    "dbl": OpSpec(0, "jac", None, "dbl", ALL),
    "add_mixed": OpSpec(1, "jac", "aff", "add", ALL),
    "add_affine": OpSpec(2, "aff", "aff", "add", ALL),
    "add": OpSpec(3, "jac", "jac", "add", ALL),
    "xyzz_add_mixed": OpSpec(4, "xyzz", "aff", "add", ALL),
    "xyzz_add_affine": OpSpec(5, "aff", "aff", "add", ALL),
    "xyzz_add": OpSpec(6, "xyzz", "xyzz", "add", ALL),
    "xyzz_roundtrip": OpSpec(7, "jac", None, "roundtrip", ALL),
    "fb_accumulate": OpSpec(8, "xyzz", "aff", "masked", ALL),
    "vbct_accumulate": OpSpec(9, "jac", "aff", "masked", NIST),
    "k_jac_add_mixed": OpSpec(10, "jac", "aff", "add", K),
    "k_jac_add_mixed_neg": OpSpec(11, "jac", "aff", "add_neg", K),
    "k_jac_double": OpSpec(12, "jac", None, "dbl", K),
    "k_jac_double_neg": OpSpec(13, "jac", None, "dbl_neg", K),
    "k_jac_double_affine": OpSpec(14, "aff", None, "dbl", K),
    "k_coz_double_affine": OpSpec(15, "aff", None, "coz_dbl", K),
    "k_coz_add_update": OpSpec(16, "jac", "coz", "coz_add", K),
    "k_add_mixed_raw": OpSpec(17, "jac", "aff", "raw_add", K),
    "k_ct_accumulate": OpSpec(18, "jac", "aff", "masked", K),
    "k_jac_add_mixed_nozr": OpSpec(19, "jac", "aff", "add", K),      # zr = nullptr, as the kernels call it: the rows of k_jac_add_mixed
}
XYZZ_OUT = ("xyzz_add_mixed", "xyzz_add_affine", "xyzz_add", "fb_accumulate")
MASKED = tuple(o for o, s in OPS.items() if s.kind == "masked")
K256_OPS = tuple(o for o, s in OPS.items() if s.curves == K)
# the ECGPU_EXC_NOTE sites of an op: prefix, and the names of its infinity sites
SITES = {
    "add_mixed": ("jac.add_mixed", {"p_inf": "inf"}),
    "add_affine": ("jac.add_affine", {}),
    "add": ("jac.add", {"p_inf": "p_inf", "q_inf": "q_inf", "both_inf": "p_inf"}),
    "xyzz_add_mixed": ("msm.xyzz_add_mixed", {"p_inf": "inf"}),
    "xyzz_add": ("msm.xyzz_add", {"p_inf": "p_inf", "q_inf": "q_inf", "both_inf": "q_inf"}),
    "k_jac_add_mixed": ("k256.jac_add_mixed", {"p_inf": "inf"}),
    "k_jac_add_mixed_nozr": ("k256.jac_add_mixed", {"p_inf": "inf"}),
}
Z_KINDS = ("1", "2", "p-1", "rand")


def ops_of(cname):
    return [o for o, s in OPS.items() if cname in s.curves]


def words_of(c):
    return c.nbytes // 4


def sqrt_mod(c, a):
    """p = 3 mod 4 on all three curves"""
    r = pow(a % c.p, (c.p + 1) // 4, c.p)
    return r if r * r % c.p == a % c.p else None


def cbrt_k256(a):
    """p = 7 mod 9: a cubic residue a has the root a^((p + 2) / 9)"""
    p = M.K256.p
    r = pow(a % p, (p + 2) // 9, p)
    return r if pow(r, 3, p) == a % p else None


def rhs(c, x):
    return (x * x * x + c.a * x + c.b) % c.p


@functools.lru_cache(maxsize=None)
def pool(cname):
    """40 random points of the curve"""
    c = M.CURVES[cname]
    rng = random.Random("pool/" + cname)
    return [M.affine_mul(c, rng.randrange(1, c.n), (c.gx, c.gy)) for _ in range(40)]


def internal_small(c, t):
    """the field value whose INTERNAL form (raw for secp256k1, Montgomery for the NIST curves) is the small integer t"""
    return t % c.p if c.name == "k256" else t * pow(1 << (8 * c.nbytes), -1, c.p) % c.p


# ---- representations: 4-tuples of integers ------------------------------------------------------------------------------------
def zval(c, kind, rng):
    return {"1": 1, "2": 2, "p-1": c.p - 1}.get(kind) or rng.randrange(3, c.p - 1)


def jac(c, A, z, rng):
    if A is None:
        return (rng.randrange(c.p), rng.randrange(c.p), 0, 0)
    return (A[0] * z * z % c.p, A[1] * pow(z, 3, c.p) % c.p, z % c.p, 0)


def xyzz(c, A, u, rng):
    if A is None:
        return (rng.randrange(c.p), rng.randrange(c.p), 0, rng.randrange(c.p))
    return (A[0] * u * u % c.p, A[1] * pow(u, 3, c.p) % c.p, u * u % c.p, pow(u, 3, c.p))


def aff(A):
    return (A[0], A[1], 0, 0)


def rep(c, form, A, z, rng):
    if form == "aff":
        return (A[0], A[1], 1, 1)
    return jac(c, A, z, rng) if form in ("jac", "coz") else xyzz(c, A, z, rng)


def is_z1(c, form, r):
    return form == "aff" or r[2] % c.p == 1


# ---- secp256k1: operands with a coordinate congruent to a small t ---------------------------------------------------------------
def small_x_point(start):
    """the first point (t, y) of secp256k1 with t >= start"""
    c = M.K256
    t = start
    while True:
        y = sqrt_mod(c, rhs(c, t))
        if y is not None:
            return (t, y)
        t += 1


def noncanon_z(A, coord, form, start):
    """denominator z such that coordinate `coord` ("x", "y", "z") of the Jacobian / XYZZ form of A is congruent to a small t >= start"""
    c = M.K256
    p = c.p
    t = start
    while True:
        if coord == "x":                                           # x z^2 = t
            z = sqrt_mod(c, t * pow(A[0], -1, p))
        elif coord == "y":                                         # y z^3 = t
            z = cbrt_k256(t * pow(A[1], -1, p))
        elif form == "xyzz":                                       # zz = z^2 = t
            z = sqrt_mod(c, t)
        else:
            z = t
        if z:
            return z, t
        t += 1


def lift(r, idx, hi):
    """coordinate idx of r given as t + p"""
    assert r[idx] < K256_SMALL
    return tuple(v + M.K256.p if (k == idx and hi) else v for k, v in enumerate(r))


# ---- near misses of the prefilter -------------------------------------------------------------------------------------------------
def near_pair(c, spec, A, B, sign, rng):
    """(p, q, A', B): representations of distinct points whose H = U2 - U1 (P of the XYZZ forms) has the internal form +-t, t small"""
    p = c.p
    t = 1
    if spec.pform == "aff":                                        # H = x2 - x1: a second point at that distance
        while True:
            x2 = (A[0] + sign * internal_small(c, t)) % p
            y2 = sqrt_mod(c, rhs(c, x2))
            if y2 is not None:
                B = (x2, y2)
                return rep(c, "aff", A, 1, rng), aff(B), B, t
            t += 1
    zq = rng.randrange(3, p - 1)
    d = (B[0] - A[0]) * (zq * zq if spec.qform != "aff" else 1) % p
    while True:                                                    # H = (x2 - x1) z1^2 [z2^2]
        z = sqrt_mod(c, sign * internal_small(c, t) * pow(d, -1, p))
        if z:
            q = aff(B) if spec.qform == "aff" else rep(c, spec.qform, B, zq, rng)
            return rep(c, spec.pform, A, z, rng), q, B, t
        t += 1


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows(cname, op):
    c = M.CURVES[cname]
    spec = OPS[op]
    assert cname in spec.curves
    if op == "k_jac_add_mixed_nozr":                               # the two forms of one formula run over the same operands
        return rows(cname, "k_jac_add_mixed")
    rng = random.Random("rows/%s/%s" % (cname, op))
    pts = pool(cname)
    p = c.p
    k256 = cname == "k256"
    out = []

    def two():
        A, B = rng.sample(pts, 2)
        return A, B

    def emit(cls, pr, qr, Pa, Qa, branch=None, aux=(0, 0)):
        out.append(Row(cls, tuple(pr), tuple(qr), aux, Pa, Qa, branch, is_z1(c, spec.pform, pr)))

    def qrep(B, zq=None):
        if spec.qform == "aff":
            return aff(B)
        return rep(c, spec.qform, B, zq if zq is not None else rng.randrange(3, p - 1), rng)

    # ---- one operand ----
    if spec.qform is None:
        for zk in Z_KINDS if spec.pform == "jac" else ("1",):
            for _ in range(6):
                A = rng.choice(pts)
                emit("ordinary:z=" + zk, rep(c, spec.pform, A, zval(c, zk, rng), rng), (0,) * 4, A, None)
        if spec.pform == "jac":
            for _ in range(4):
                emit("dbl_inf", jac(c, None, 0, rng), (0,) * 4, None, None, "inf")
            if k256:
                for _ in range(4):
                    r = jac(c, None, 0, rng)
                    emit("dbl_inf:rawp", (r[0], r[1], p, 0), (0,) * 4, None, None, "inf")
        if k256:
            for coord, idx in (("x", 0), ("y", 1), ("z", 2)):
                if spec.pform == "aff" and coord != "x":
                    continue
                for hi in (0, 1):
                    for s in range(2):
                        if spec.pform == "aff":
                            A = small_x_point(3 + 1000 * s)
                            r = rep(c, "aff", A, 1, rng)
                        else:
                            A = rng.choice(pts)
                            z, _ = noncanon_z(A, coord, "jac", 2 + 50 * s)
                            r = jac(c, A, z, rng)
                        emit("noncanon:%s:%s" % (coord, "hi" if hi else "lo"), lift(r, idx, hi), (0,) * 4, A, None)
        return out

    # ---- co-Z addition with update: two points over one denominator; exceptional operands are outside its contract ----
    if spec.kind == "coz_add":
        for zk in Z_KINDS:
            for _ in range(6):
                A, B = two()
                z = zval(c, zk, rng)
                emit("ordinary:z=" + zk, jac(c, A, z, rng), jac(c, B, z, rng), A, B)
        for hi in (0, 1):
            for s in range(2):
                A, B = two()
                z, _ = noncanon_z(A, "x", "jac", 2 + 50 * s)
                emit("noncanon:x:%s" % ("hi" if hi else "lo"), lift(jac(c, A, z, rng), 0, hi), jac(c, B, z, rng), A, B)
        return out

    masked = spec.kind == "masked"
    exact = spec.kind in ("add", "add_neg")                        # the formulas that handle their exceptional operands
    pz_kinds = Z_KINDS if spec.pform != "aff" else ("1",)

    def ordinary(cls, n, aux=(0, 0)):
        for _ in range(n):
            A, B = two()
            emit(cls, rep(c, spec.pform, A, rng.randrange(3, p - 1), rng), qrep(B), A, B, aux=aux)

    def near(aux=(0, 0), suffix=""):
        for sign in (1, -1):
            for _ in range(12):
                A, B = two()
                pr, qr, B, t = near_pair(c, spec, A, B, sign, rng)
                emit("near:%s%d%s" % ("+" if sign > 0 else "-", t, suffix), pr, qr, A, B, aux=aux)

    def noncanon(situations, aux=(0, 0)):
        coords = [("x", 0)] if spec.pform == "aff" else [("x", 0), ("y", 1), ("zz" if spec.pform == "xyzz" else "z", 2)]
        for coord, idx in coords:
            for hi in (0, 1):
                for sit in situations:
                    for s in range(2):
                        if spec.pform == "aff":
                            A = small_x_point(3 + 1000 * s)
                            r = rep(c, "aff", A, 1, rng)
                        else:
                            A = rng.choice(pts)
                            z, _ = noncanon_z(A, coord[0], spec.pform, 2 + 50 * s)
                            r = rep(c, spec.pform, A, z, rng)
                        B = A if sit == "same" else rng.choice([x for x in pts if x != A])
                        emit("noncanon:%s:%s%s" % (coord, "hi" if hi else "lo", ":same" if sit == "same" else ""), lift(r, idx, hi), qrep(B), A, B,
                             "same" if sit == "same" and not masked else None, aux=aux)
        for hi in (0, 1) if spec.qform == "aff" else ():          # the affine x of the second operand
            for sit in situations:
                B = small_x_point(5000 + 77 * hi)
                A = B if sit == "same" else rng.choice(pts)
                qr = lift(qrep(B), 0, hi)
                emit("noncanon:qx:%s%s" % ("hi" if hi else "lo", ":same" if sit == "same" else ""), rep(c, spec.pform, A, rng.randrange(3, p - 1), rng), qr, A, B,
                     "same" if sit == "same" and not masked else None, aux=aux)

    if masked:
        for e in (0, ONES):
            for zd in (0, ONES):
                ordinary("mask:e=%d:zd=%d" % (e & 1, zd & 1), 32, (e, zd))
                for _ in range(4 if e else 0):                     # the unmasked formula meets P at infinity
                    B = rng.choice(pts)
                    emit("mask:e=1:zd=%d:inf" % (zd & 1), (0, 0, 0, 0), qrep(B), None, B, aux=(e, zd))
                if e and k256 and spec.pform == "jac":
                    for _ in range(2):
                        B = rng.choice(pts)
                        emit("mask:e=1:zd=%d:inf:rawp" % (zd & 1), (0, 0, p, 0), qrep(B), None, B, aux=(e, zd))
        for sit in ("same", "opp"):                                # a zero digit keeps the accumulator whatever the entry is
            for zk in pz_kinds:
                A = rng.choice(pts)
                B = A if sit == "same" else M.affine_neg(c, A)
                emit("mask:e=0:zd=1:%s:z=%s" % (sit, zk), rep(c, spec.pform, A, zval(c, zk, rng), rng), qrep(B), A, B, aux=(0, ONES))
        near((0, 0), ":mask")
        if k256:
            noncanon(("ordinary",))
        return out

    ordinary("ordinary", 160)
    if exact and spec.pform != "aff":
        variants = [("", 0)] + ([(":rawp", p)] if k256 else [])
        for suffix, zero in variants:
            for _ in range(4):
                B = rng.choice(pts)
                r = rep(c, spec.pform, None, 0, rng)
                emit("p_inf" + suffix, (r[0], r[1], zero, r[3]), qrep(B), None, B, "p_inf")
            if spec.qform != "aff":
                for _ in range(4):
                    A = rng.choice(pts)
                    r = rep(c, spec.qform, None, 0, rng)
                    emit("q_inf" + suffix, rep(c, spec.pform, A, rng.randrange(3, p - 1), rng), (r[0], r[1], zero, r[3]), A, None, "q_inf")
                for _ in range(2):
                    r, s = rep(c, spec.pform, None, 0, rng), rep(c, spec.qform, None, 0, rng)
                    emit("both_inf" + suffix, (r[0], r[1], zero, r[3]), (s[0], s[1], zero, s[3]), None, None, "both_inf")
    if exact:
        for sit in ("same", "opp"):
            for zk in pz_kinds:
                for _ in range(12):
                    A = rng.choice(pts)
                    B = A if sit == "same" else M.affine_neg(c, A)
                    emit("%s:z=%s" % (sit, zk), rep(c, spec.pform, A, zval(c, zk, rng), rng), qrep(B), A, B, sit)
            if spec.qform != "aff":                                # the second denominator one, the first not
                for _ in range(12):
                    A = rng.choice(pts)
                    B = A if sit == "same" else M.affine_neg(c, A)
                    emit("%s:z=rand:q1" % sit, rep(c, spec.pform, A, rng.randrange(3, p - 1), rng), qrep(B, 1), A, B, sit)
    near()
    if k256:
        noncanon(("ordinary", "same") if exact else ("ordinary",))
    return out


def class_counts(cname):
    """{class: rows} summed over the ops of a curve"""
    n = {}
    for op in ops_of(cname):
        for r in rows(cname, op):
            n[r.cls] = n.get(r.cls, 0) + 1
    return n


def is_exceptional(r):
    return not r.cls.startswith("ordinary") and r.cls != "mask:e=0:zd=0"


# ---- lane layouts: lists of row indices -----------------------------------------------------------------------------------------------
def layouts(rs):
    by_cls = {}
    for i, r in enumerate(rs):
        by_cls.setdefault(r.cls, []).append(i)
    srt = []
    for idx in by_cls.values():
        n = -(-len(idx) // WAVE) * WAVE
        srt += [idx[k % len(idx)] for k in range(n)]
    inter, k = [], 0
    while len(inter) < len(rs):
        for idx in by_cls.values():
            if k < len(idx):
                inter.append(idx[k])
        k += 1
    plain = [i for i, r in enumerate(rs) if not is_exceptional(r)]
    single = []
    for n, i in enumerate(i for i, r in enumerate(rs) if is_exceptional(r)):
        wave = [plain[(n + k) % len(plain)] for k in range(WAVE)]
        wave[(0, 31, 32, 63)[n % 4]] = i
        single += wave
    return {"sorted": srt, "interleaved": inter, "single": single}


# ---- words ----------------------------------------------------------------------------------------------------------------------------
def to_internal(c, v):
    """the integer whose little-endian words are the field's internal form of v (secp256k1: v itself, possibly >= p)"""
    return v if c.name == "k256" else v * (1 << (8 * c.nbytes)) % c.p


def pack(c, rs):
    """rows -> p, q (n x 4 NW), aux (n x 2) uint32 arrays"""
    nb = c.nbytes
    pb = b"".join(to_internal(c, v).to_bytes(nb, "little") for r in rs for v in r.p)
    qb = b"".join(to_internal(c, v).to_bytes(nb, "little") for r in rs for v in r.q)
    n = len(rs)
    return (np.frombuffer(pb, dtype="<u4").reshape(n, IN_FE * nb // 4).astype(np.uint32),
            np.frombuffer(qb, dtype="<u4").reshape(n, IN_FE * nb // 4).astype(np.uint32),
            np.array([r.aux for r in rs], dtype=np.uint32).reshape(n, AUX))


def unpack(c, out_row):
    """one output row -> ([5 internal integers], flag)"""
    nw = words_of(c)
    raw = np.ascontiguousarray(out_row[:OUT_FE * nw], dtype="<u4").tobytes()
    return [int.from_bytes(raw[4 * nw * e:4 * nw * (e + 1)], "little") for e in range(OUT_FE)], int(out_row[OUT_FE * nw])


def run(fn, c, op, rs):
    """fn: dt_pt_op / ht_pt_op.  Returns the n x (5 NW + 1) output words, in calls of at most 2^13 pairs"""
    import ctypes
    P = ctypes.POINTER(ctypes.c_uint32)
    nw = words_of(c)
    out = np.zeros((len(rs), OUT_FE * nw + 1), dtype=np.uint32)
    for lo in range(0, len(rs), MAX_CALL):
        part = rs[lo:lo + MAX_CALL]
        p, q, aux = pack(c, part)
        o = np.zeros((len(part), OUT_FE * nw + 1), dtype=np.uint32)
        rc = fn(M.CURVE_IDS[c.name], OPS[op].code, p.ctypes.data_as(P), q.ctypes.data_as(P), aux.ctypes.data_as(P), o.ctypes.data_as(P), len(part))
        if rc != 0:
            raise RuntimeError("%s %s returned %d" % (c.name, op, rc))
        out[lo:lo + len(part)] = o
    return out


# ---- RFC 6979 with an order that rejects often -------------------------------------------------------------------------------------
# name: (hash id, hash, bytes, q, seed, inputs, extra on index i iff i % EXTRA_MOD == EXTRA_REM): the streams of
# tests/test_hosttwin_signing.py::test_generate_k_rejection_branch and ..._sha384
RFC_STREAMS = {
    "sha256": (0, "sha256", 32, (1 << 255) + 0x1D, 0x7e1ec7, 2000, 4, 3),
    "sha384": (1, "sha384", 48, (1 << 383) + 0x1D, 0x384, 300, 2, 1),
}


def wave_mixes_rounds(rejections):
    """one wave of 64 consecutive inputs holds lanes with 0, 1, 2 and >= 3 rejections together"""
    return any({min(r, 3) for r in rejections[w:w + WAVE]} == {0, 1, 2, 3} for w in range(0, len(rejections), WAVE))


@functools.lru_cache(maxsize=None)
def rfc6979_stream(name):
    """(hash id, q, [(x, h1, extra)], [(k, rejections)] of tests/rfc6979_model.py): the stream of the host-twin test, continued with
    further inputs of the same generator, a wave at a time, until the model says that a wave mixes the rounds"""
    import rfc6979_model as R
    hid, hname, nb, q, seed, count, mod, rem = RFC_STREAMS[name]
    rng = random.Random(seed)
    ins, want = [], []
    while len(ins) < count or not wave_mixes_rounds([r for _, r in want]):
        for _ in range(count if not ins else WAVE):
            i = len(ins)
            x, h1 = rng.randbytes(nb), rng.randbytes(nb)
            extra = rng.randbytes(nb) if i % mod == rem else b""
            ins.append((x, h1, extra))
            want.append(R.generate_k(q, hname, x, h1, extra))
    return hid, q, ins, want


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def check(c, op, r, out_row):
    """None if the output row is what the integer model says for row r, else a description of the difference"""
    spec = OPS[op]
    p = c.p
    o, flag = unpack(c, out_row)
    raw = list(o)
    if c.name != "k256":                                           # Montgomery outputs are canonical
        if any(v >= p for v in o):
            return "an output word string is not below the modulus"
        ri = pow(1 << (8 * c.nbytes), -1, p)
        o = [v * ri % p for v in o]
    v = [x % p for x in o]

    def affine_jac(X, Y, Z):
        return None if Z == 0 else (X * pow(Z, -2, p) % p, Y * pow(Z, -3, p) % p)

    def affine_xyzz(X, Y, ZZ, ZZZ):
        if ZZ == 0:
            return None
        if pow(ZZ, 3, p) != ZZZ * ZZZ % p:
            return "ZZ^3 != ZZZ^2"
        return (X * pow(ZZ, -1, p) % p, Y * pow(ZZ * ZZZ, -1, p) * ZZ % p)

    got = affine_xyzz(*v[:4]) if op in XYZZ_OUT else affine_jac(*v[:3])
    add = M.affine_add(c, r.Pa, r.Qa)
    if spec.kind == "masked":
        e, zd = r.aux
        want_flag = e & zd
        if zd:                                                     # the accumulator is kept, word for word
            nf = 4 if op in XYZZ_OUT else 3
            if raw[:nf] != [to_internal(c, x) for x in r.p[:nf]]:
                return "a zero digit changed the accumulator"
            want = got
        else:
            want = r.Qa if e else add
        if op == "vbct_accumulate":
            if (flag >> 1) & 1 != (1 if v[2] == 0 else 0):
                return "fe_zero_mask disagrees with Z"
            flag = ONES if flag & 1 else 0
        if flag != want_flag:
            return "empty mask %#x, expected %#x" % (flag, want_flag)
        if e and not zd and (v[2] != 1 or (op in XYZZ_OUT and v[3] != 1)):
            return "first entry taken with a denominator that is not one"
    elif spec.kind in ("add", "raw_add"):
        want = add
    elif spec.kind == "add_neg":
        want = M.affine_neg(c, add)
    elif spec.kind == "dbl":
        want = M.affine_add(c, r.Pa, r.Pa)
    elif spec.kind == "dbl_neg":
        want = M.affine_neg(c, M.affine_add(c, r.Pa, r.Pa))
    elif spec.kind == "roundtrip":
        want = r.Pa
        if r.Pa is not None and v[3] != pow(r.p[2], 3, p):
            return "ZZZ of the round trip"
    elif spec.kind == "coz_dbl":                                   # d = 2P over Z = 2y, (qx, qy) = P over that Z
        want = M.affine_add(c, r.Pa, r.Pa)
        if affine_jac(v[3], v[4], v[2]) != r.Pa:
            return "the rewritten P is not P"
    elif spec.kind == "coz_add":                                   # r + q and q over Z h
        z3 = r.p[2] * v[2] % p
        got = affine_jac(v[0], v[1], z3)
        want = add
        if affine_jac(v[3], v[4], z3) != r.Qa:
            return "the rewritten q is not q"
    if isinstance(got, str):
        return got
    if got != want:
        return "result %s, expected %s" % (got, want)
    if op == "k_jac_add_mixed_nozr" and raw[4] != 0:
        return "element 4 written without zr"
    if op in ("k_jac_add_mixed", "k_add_mixed_raw"):               # zr = Z3 / Z1; an accumulator at infinity has no ratio: zr = 1
        if r.Pa is None:
            if v[4] != 1:
                return "zr of an accumulator at infinity is not one"
        elif v[2] != r.p[2] * v[4] % p:
            return "Z3 != Z1 zr"
    return None
