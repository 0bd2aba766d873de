"""The host-walkable multi-point schedules (tests/hosttwin) behind one call shape, for the related-point tests: a schedule takes the
flat scalars and multipliers of n combinations of `terms` terms over one family and returns [(x || y bytes, infinity flag)] per
combination.  Also the exceptional-case counters of the ECGPU_EXC_NOTE hook (csrc/mp32.hpp)."""
import ctypes
import os
import re

import related_point_vectors as V
from hosttwin_util import lib, buf, outbuf

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rustcrypto-elliptic-curves_amd", "csrc")


def exc_reset():
    lib().ht_exc_reset()


def exc_counts():
    """{site: hits} since the last reset"""
    f = lib().ht_exc_counts
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    b = ctypes.create_string_buffer(1 << 14)
    assert f(b, len(b)) < len(b)
    return {k: int(v) for k, v in (line.split("=") for line in b.value.decode().splitlines())}


def exc_sites_in_source():
    """every site name an ECGPU_EXC_NOTE of csrc/ carries"""
    names = set()
    for fn in os.listdir(CSRC):
        with open(os.path.join(CSRC, fn)) as f:
            names.update(re.findall(r'ECGPU_EXC_NOTE\("([^"]+)"', f.read()))
    return names


def _split(c, raw_xy, raw_inf, n):
    w = 2 * c.nbytes
    return [(raw_xy[w * i:w * (i + 1)], raw_inf[i]) for i in range(n)]


def _inputs(fam, ks, ms, proj_rng):
    return buf(V.scalar_bytes(fam.c, ks)), buf(V.point_bytes(fam, ms, proj_rng)), 1 if proj_rng is not None else 0


def straus(fam, ks, ms, terms, proj_rng=None, lanes=2, plan_lanes=1, g_force=0):
    """csrc/straus.hpp: both stages, the product's own plan for plan_lanes resident lanes or a forced group size"""
    c = fam.c
    n = len(ks) // terms
    sb, pb, fmt = _inputs(fam, ks, ms, proj_rng)
    out, inf = outbuf(2 * c.nbytes * n), outbuf(n)
    f = lib().ht_straus
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                  ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    assert f(V.CURVE_IDS[c.name], sb, pb, fmt, terms, out, 0, inf, n, lanes, plan_lanes, g_force, None) == 0
    return _split(c, bytes(out), bytes(inf), n)


def vb_lincomb(fam, ks, ms, terms, proj_rng=None, lanes=3):
    """csrc/varbase_lane.hpp, P-256 / P-384: one or two terms per unit over shared doublings"""
    c = fam.c
    assert c.name != "k256" and terms in (1, 2)
    n = len(ks) // terms
    sb, pb, fmt = _inputs(fam, ks, ms, proj_rng)
    out, inf = outbuf(2 * c.nbytes * n), outbuf(n)
    f = lib().ht_vb_lincomb
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                  ctypes.c_size_t]
    assert f(V.CURVE_IDS[c.name], sb, pb, fmt, terms, out, 0, inf, n, lanes) == 0
    return _split(c, bytes(out), bytes(inf), n)


def k256_fast(fam, ks, ms, terms, proj_rng=None, batch=5):
    """secp256k1: the single-term throughput loop (terms = 1) or the lane body of the two-term throughput kernel (terms = 2)"""
    c = fam.c
    assert c.name == "k256" and terms in (1, 2)
    n = len(ks) // terms
    sb, pb, fmt = _inputs(fam, ks, ms, proj_rng)
    out = outbuf(65 * n)
    f = lib().ht_k256_mul_fast if terms == 1 else lib().ht_k256_lincomb2_fast
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert f(pb, fmt, sb, out, n, batch) == 0
    o = bytes(out)
    return [(o[65 * i:65 * i + 64], o[65 * i + 64]) for i in range(n)]


def schedules(c, terms):
    """[(name, callable(fam, ks, ms, proj_rng))]: every host-walkable schedule that takes `terms` terms on this curve"""
    out = []
    if terms <= 2:
        if c.name == "k256":
            out.append(("k256_fast", lambda fam, ks, ms, pr: k256_fast(fam, ks, ms, terms, pr)))
        else:
            out.append(("vb_lincomb", lambda fam, ks, ms, pr: vb_lincomb(fam, ks, ms, terms, pr)))
    if terms >= 2:
        out.append(("straus", lambda fam, ks, ms, pr: straus(fam, ks, ms, terms, pr)))
        if terms in (5, 7):                                    # odd group sizes forced: 5 = 2 + 2 + 1, 7 = 3 + 3 + 1
            out.append(("straus_g%d" % (terms // 2), lambda fam, ks, ms, pr: straus(fam, ks, ms, terms, pr, g_force=terms // 2)))
    return out


# ---- the formulas one at a time, on operands from the family ----------------------------------------------------------------------
def _fe(c, v):
    return int(v % c.p).to_bytes(c.nbytes, "big")


def formula(fam, op, pairs, rng):
    """op: "add_mixed" / "add_affine" / "add" (csrc/jacobian.hpp through ht_jac_op), "xyzz" (msm::xyzz_add_mixed and, for every fourth
    pair, the general msm::xyzz_add: ht_xyzz_add_mixed), "xyzz_add" (msm::xyzz_add, both operands XYZZ: ht_xyzz_add).  pairs: (m_a, m_b) multipliers of the family, 0 = infinity (where the
    operand can be); the first operand gets a random Z (none for add_affine), the second too for "add".  Returns the multiples as
    affine points (None: infinity)."""
    c = fam.c
    p, nb, cid = c.p, c.nbytes, V.CURVE_IDS[c.name]

    def jacp(m, affine=False):
        A = fam.point(m)
        if A is None:
            return (rng.randrange(p), rng.randrange(p), 0)
        z = 1 if affine else rng.randrange(2, p)
        return (A[0] * z * z % p, A[1] * z * z * z % p, z)

    def aff(m):
        A = fam.point(m)
        return _fe(c, A[0]) + _fe(c, A[1])

    n = len(pairs)
    out = outbuf(3 * nb * n)
    if op in ("xyzz", "xyzz_add"):
        xyzz = lambda ms_: b"".join(b"".join(_fe(c, v) for v in (X, Y, Z * Z, Z * Z * Z)) for X, Y, Z in (jacp(m) for m in ms_))
        pin = xyzz([a for a, _ in pairs])
        if op == "xyzz":
            assert lib().ht_xyzz_add_mixed(cid, buf(pin), buf(b"".join(aff(b) for _, b in pairs)), out, n) == 0
        else:
            assert lib().ht_xyzz_add(cid, buf(pin), buf(xyzz([b for _, b in pairs])), out, n) == 0
    else:
        code = {"add_mixed": 1, "add": 2, "add_affine": 3}[op]
        pin = b"".join(b"".join(_fe(c, v) for v in jacp(a, op == "add_affine")) for a, _ in pairs)
        qin = b"".join(b"".join(_fe(c, v) for v in jacp(b)) if op == "add" else aff(b) for _, b in pairs)
        assert lib().ht_jac_op(cid, code, buf(pin), buf(qin), out, n) == 0
    o = bytes(out)
    res = []
    for i in range(n):
        X, Y, Z = (int.from_bytes(o[3 * nb * i + nb * t:3 * nb * i + nb * (t + 1)], "big") for t in range(3))
        res.append(None if Z == 0 else (X * pow(Z, -2, p) % p, Y * pow(Z, -3, p) % p))
    return res
