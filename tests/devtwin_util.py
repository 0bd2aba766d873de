"""Loader for the test-only gfx950 builds of the field and scalar primitives, the point formulas, the RFC 6979 generator and
the ECDSA sign_finish / verify_check kernels (tests/devtwin) and their host counterpart (tests/hosttwin, the same op tables).  Arrays are (n, words) little-endian uint32; every call checks the return code and
raises at the first non-zero one."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEVTWIN = os.path.join(HERE, "devtwin")
BUILDS = {"default": "libecdevtwin.so", "bf": "libecdevtwin_bf.so", "grouped": "libecdevtwin_grouped.so",
          # the point formulas (devtwin_group.hip) in the two configurations that ship them, and the RFC 6979 generator
          "group": "libecdevtwin_group.so", "group_bf": "libecdevtwin_group_bf.so", "rfc6979": "libecdevtwin_rfc6979.so",
          # ecdsa::sign_finish_kernel and ecdsa::verify_check_kernel on chosen R, A and B
          "ecdsa": "libecdevtwin_ecdsa.so"}
_LIBS = {}

# op tables of tests/devtwin/primitive_ops.hpp
K256_OPS = ["mul", "sqr", "add", "sub", "neg", "inv", "sqrt", "mul_small", "shl1", "shl2", "shl3", "mul_add2", "mul_add_sqr",
            "half", "sub2", "normalize", "fold_top_fast", "is_zero_fast"]
MONT_OPS = ["mul", "sqr", "add", "sub", "neg", "dbl", "half", "to_mont", "from_mont", "inv", "sqrt"]
SCALAR_OPS = ["mul", "add", "reduce_once", "to_mont", "from_mont", "inv"]
MONT_CURVES = ["p256", "p384"]
SCALAR_CURVES = ["k256", "p256", "p384"]
MAC_MAX_M = 13

_P = ctypes.POINTER(ctypes.c_uint32)


def lib(build="default"):
    if build not in _LIBS:
        override = os.environ.get("ECGPU_DEVTWIN_DIR")     # the same objects built elsewhere (e.g. from a patched csrc)
        if override:
            _LIBS[build] = ctypes.CDLL(os.path.join(override, BUILDS[build]))
        else:
            subprocess.run(["make", "-s", "-C", DEVTWIN, BUILDS[build]], check=True)
            _LIBS[build] = ctypes.CDLL(os.path.join(DEVTWIN, BUILDS[build]))
    return _LIBS[build]


def _ptr(a):
    return a.ctypes.data_as(_P)


def _in(a, words):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    assert a.ndim == 2 and a.shape[1] == words, (a.shape, words)
    return a


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} returned {rc}")


def k256_op(fn, op, a, b, e, f):
    a, b, e, f = (_in(x, 8) for x in (a, b, e, f))
    n = a.shape[0]
    assert b.shape[0] == e.shape[0] == f.shape[0] == n
    out = np.zeros((n, 9), dtype=np.uint32)
    _check(fn(K256_OPS.index(op), _ptr(a), _ptr(b), _ptr(e), _ptr(f), _ptr(out), n), f"k256 {op}")
    return out


def mont_op(fn, curve, op, a, b):
    w = 8 if curve == "p256" else 12
    a, b = _in(a, w), _in(b, w)
    n = a.shape[0]
    assert b.shape[0] == n
    out = np.zeros((n, w + 1), dtype=np.uint32)
    _check(fn(MONT_CURVES.index(curve), MONT_OPS.index(op), _ptr(a), _ptr(b), _ptr(out), n), f"{curve} mont {op}")
    return out


def scalar_op(fn, curve, op, a, b):
    w = 12 if curve == "p384" else 8
    a, b = _in(a, w), _in(b, w)
    n = a.shape[0]
    assert b.shape[0] == n
    out = np.zeros((n, w), dtype=np.uint32)
    _check(fn(SCALAR_CURVES.index(curve), SCALAR_OPS.index(op), _ptr(a), _ptr(b), _ptr(out), n), f"{curve} scalar {op}")
    return out


def mac_cols(fn, M, fresh, nc, c, pa, pb):
    c, pa, pb = _in(c, 3), _in(pa, MAC_MAX_M), _in(pb, MAC_MAX_M)
    n = c.shape[0]
    out = np.zeros((n, 3), dtype=np.uint32)
    _check(fn(M, fresh, nc, _ptr(c), _ptr(pa), _ptr(pb), _ptr(out), n), f"mac_cols<{M}, {fresh}, {nc}>")
    return out


# the entry points by side: dt_* of a device build, ht_* of the host twin
def device(build="default"):
    L = lib(build)
    return {"k256": L.dt_k256_op, "mont": L.dt_mont_op, "scalar": L.dt_scalar_op, "mac": L.dt_mac_cols}


def host():
    from hosttwin_util import lib as hlib
    L = hlib()
    return {"k256": L.ht_k256_prim_op, "mont": L.ht_mont_prim_op, "scalar": L.ht_scalar_op, "mac": L.ht_mac_cols}


# the point-formula op table (tests/devtwin/group_ops.hpp; callers: tests/group_edge_vectors.py run())
def device_pt_op(build="group"):
    assert build in ("group", "group_bf")
    return lib(build).dt_pt_op


def host_pt_op():
    from hosttwin_util import lib as hlib
    return hlib().ht_pt_op


def rfc6979_generate_k(hash_id, xs, h1s, extras, q):
    """dt_rfc6979_generate_k over lists of byte strings (big-endian, one digest long; extras: b"" where a lane has none) and the
    order q -> ([k], [rejections])"""
    nw = 8 if hash_id == 0 else 12
    n = len(xs)
    limbs = lambda bs, w: np.frombuffer(b"".join(int.from_bytes(b, "big").to_bytes(4 * w, "little") for b in bs), dtype="<u4").reshape(len(bs), w).astype(np.uint32)
    x, h1 = limbs(xs, nw), limbs(h1s, nw)
    ex = np.zeros((n, nw + 1), dtype=np.uint32)
    ex[:, :nw] = limbs([e or bytes(4 * nw) for e in extras], nw)
    ex[:, nw] = [1 if e else 0 for e in extras]
    qw = limbs([q.to_bytes(4 * nw, "big")], nw)
    k = np.zeros((n, nw), dtype=np.uint32)
    rej = np.zeros(n, dtype=np.uint32)
    _check(lib("rfc6979").dt_rfc6979_generate_k(hash_id, _ptr(x), _ptr(h1), _ptr(ex) if any(extras) else None, _ptr(qw), _ptr(k), _ptr(rej), n),
           "rfc6979 generate_k")
    raw = np.ascontiguousarray(k, dtype="<u4").tobytes()
    return [int.from_bytes(raw[4 * nw * i:4 * nw * (i + 1)], "little") for i in range(n)], [int(r) for r in rej]


# the ECDSA kernels (tests/devtwin/devtwin_ecdsa.hip): rows of big-endian bytes, as on the C ABI
def _byte_rows(rows, width):
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy()
    assert a.ctypes.data % 4 == 0
    return a


def _bp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def ecdsa_sign_finish(curve, d, k, z, r_xy, r_inf, flags):
    """dt_ecdsa_sign_finish over lists of byte strings (d, k, z: one scalar long; r_xy: x || y of R) and a list of identity flags
    -> (sig (n, 2 nb), recid (n,), ok (n,)), uint8"""
    nb = 48 if curve == "p384" else 32
    n = len(d)
    assert len(k) == len(z) == len(r_xy) == len(r_inf) == n
    cols = [_byte_rows(d, nb), _byte_rows(k, nb), _byte_rows(z, nb), _byte_rows(r_xy, 2 * nb), np.array(r_inf, dtype=np.uint8)]
    sig, recid, ok = np.zeros((n, 2 * nb), dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8)
    _check(lib("ecdsa").dt_ecdsa_sign_finish(SCALAR_CURVES.index(curve), *map(_bp, cols), int(flags), _bp(sig), _bp(recid), _bp(ok), n),
           f"{curve} ecdsa sign_finish")
    return sig, recid, ok


def ecdsa_verify_check(curve, a_xy, a_inf, b_xy, b_inf, sig, ok_in):
    """dt_ecdsa_verify_check over lists of byte strings (a_xy, b_xy: x || y; sig: r || s) and lists of flags -> ok (n,) uint8"""
    nb = 48 if curve == "p384" else 32
    n = len(sig)
    assert len(a_xy) == len(a_inf) == len(b_xy) == len(b_inf) == len(ok_in) == n
    ok = np.array(ok_in, dtype=np.uint8)
    cols = [_byte_rows(a_xy, 2 * nb), np.array(a_inf, dtype=np.uint8), _byte_rows(b_xy, 2 * nb), np.array(b_inf, dtype=np.uint8), _byte_rows(sig, 2 * nb)]
    _check(lib("ecdsa").dt_ecdsa_verify_check(SCALAR_CURVES.index(curve), *map(_bp, cols), _bp(ok), n), f"{curve} ecdsa verify_check")
    return ok
