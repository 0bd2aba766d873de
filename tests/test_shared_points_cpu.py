"""Shared points at the boundary, without a GPU: the flag and the four options have one value in the header, the package and the Rust
shim, and the Python wrappers marshal a shared point as the C ABI wants it - `terms` rows (one key), n taken from the scalars -
checked on a stub library that records what reaches it (the style of test_binding_calls_cpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import ecgpu

PKG = os.path.join(ROOT, "rustcrypto-elliptic-curves_amd")
NAMES = {"ECGPU_SHARED_POINTS": 64, "ECGPU_OPT_SHARED_WINDOW": 9, "ECGPU_OPT_SHARED_MIN": 10, "ECGPU_OPT_SHARED_TABLE_BUDGET": 11,
         "ECGPU_OPT_SHARED_TABLE_BUILDS": 12, "ECGPU_OPT_COUNT_": 13}


def test_constants_agree():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecgpu.h")).read(), flags=re.S)
    rust = open(os.path.join(PKG, "rust", "ecgpu-sys", "src", "lib.rs")).read()
    for name, value in NAMES.items():
        m = re.search(r"\b%s\s*=\s*(\d+)u?\b" % name, header)
        assert m and int(m.group(1)) == value, name
        m = re.search(r"pub const %s: \w+ = (\d+);" % name, rust)
        assert m and int(m.group(1)) == value, name
        if name != "ECGPU_OPT_COUNT_":
            assert getattr(ecgpu, name[len("ECGPU_"):]) == value, name
    assert sorted(getattr(ecgpu, n) for n in dir(ecgpu) if n.startswith("OPT_")) == list(range(NAMES["ECGPU_OPT_COUNT_"]))
    # the flag's bit is its own: no other flag of the scalar-multiplication and ECDSA calls shares it
    others = (ecgpu.EXACT_REFERENCE, ecgpu.ECDSA_LOW_S, ecgpu.PUBLIC_SCALARS, ecgpu.SECRET_SCALARS, ecgpu.BATCH_VERDICT_ONLY, ecgpu.BATCH_EQUATION_ALWAYS)
    assert all(ecgpu.SHARED_POINTS & f == 0 for f in others)


class _Lib:
    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        if not name.startswith("ecgpu_"):
            raise AttributeError(name)

        def fn(*args):
            self._calls.append((name, args))
            return 0
        return fn


class _Ctx:
    def __init__(self):
        self.calls = []
        self.lib, self.handle = _Lib(self.calls), ctypes.c_void_p(0x7E570000)

    def check(self, rc):
        assert rc == 0


def _value(a):
    return a.value if isinstance(a, ctypes._SimpleCData) else a


@pytest.mark.parametrize("curve,nb", [("k256", 32), ("p384", 48)])
@pytest.mark.parametrize("terms", [1, 3])
def test_lincomb_passes_terms_rows_and_n_from_the_scalars(curve, nb, terms):
    ctx = _Ctx()
    cv = ecgpu.Curve(ctx, ecgpu.CURVE_IDS[curve])
    n = 5
    s = np.arange(n * terms * nb, dtype=np.uint8).reshape(n * terms, nb)
    p = np.arange(terms * 2 * nb, dtype=np.uint8).reshape(terms, 2 * nb)
    out, inf = cv.lincomb(s, p, terms=terms, flags=ecgpu.SHARED_POINTS)
    assert out.shape == (n, 2 * nb) and inf.shape == (n,)
    (name, args), = ctx.calls
    assert name == "ecgpu_lincomb_batch"
    handle, cid, sp, pp, pfmt, t, op, ofmt, ip, count, mem, flags = [_value(a) for a in args]
    assert (cid, pfmt, t, ofmt, count, mem, flags) == (ecgpu.CURVE_IDS[curve], ecgpu.AFFINE, terms, ecgpu.AFFINE, n, ecgpu.HOST, ecgpu.SHARED_POINTS)
    assert sp == s.ctypes.data and pp == p.ctypes.data and op == out.ctypes.data and ip == inf.ctypes.data
    # the bytes behind the points pointer are the `terms` rows, nothing replicated
    assert ctypes.string_at(pp, terms * 2 * nb) == p.tobytes()


def test_mul_and_checked_form():
    ctx = _Ctx()
    cv = ecgpu.Curve(ctx, ecgpu.K256)
    s = np.zeros((4, 32), dtype=np.uint8)
    p = np.ones((1, 64), dtype=np.uint8)
    cv.mul(s, p, flags=ecgpu.SHARED_POINTS | ecgpu.SECRET_SCALARS)
    cv.lincomb(s, p, flags=ecgpu.SHARED_POINTS, checked=True)
    (n1, a1), (n2, a2) = ctx.calls
    assert n1 == "ecgpu_lincomb_batch" and _value(a1[5]) == 1 and _value(a1[9]) == 4 and _value(a1[11]) == ecgpu.SHARED_POINTS | ecgpu.SECRET_SCALARS
    assert n2 == "ecgpu_lincomb_batch_checked" and _value(a2[10]) == 4 and _value(a2[12]) == ecgpu.SHARED_POINTS


def test_wrong_row_counts_raise():
    ctx = _Ctx()
    cv = ecgpu.Curve(ctx, ecgpu.P256)
    s = np.zeros((6, 32), dtype=np.uint8)
    for rows, terms in ((6, 1), (2, 1), (6, 2), (1, 2), (3, 2)):          # replicated, too many, replicated, too few, n rows
        with pytest.raises(ValueError):
            cv.lincomb(s, np.zeros((rows, 64), dtype=np.uint8), terms=terms, flags=ecgpu.SHARED_POINTS)
    with pytest.raises(ValueError):
        cv.lincomb(s, None, flags=ecgpu.SHARED_POINTS)
    with pytest.raises(ValueError):                                       # a projective point has many encodings of one key
        cv.lincomb(s, np.zeros((1, 96), dtype=np.uint8), point_format=ecgpu.PROJECTIVE, flags=ecgpu.SHARED_POINTS)
    with pytest.raises(ValueError):
        cv.mul_device(0xD0000000, np.zeros((2, 64), dtype=np.uint8), 0xD0100000, 6, flags=ecgpu.SHARED_POINTS)
    with pytest.raises(ValueError):
        cv.ecdsa_verify(s, np.zeros((6, 64), dtype=np.uint8), np.zeros((6, 64), dtype=np.uint8), flags=ecgpu.SHARED_POINTS)
    with pytest.raises(ValueError):
        cv.ecdsa_verify_device(0xD0000000, 0xD0100000, np.zeros((2, 64), dtype=np.uint8), 0xD0200000, 6, flags=ecgpu.SHARED_POINTS)
    assert ctx.calls == []
    # without the flag the old rule stands
    with pytest.raises(ValueError):
        cv.lincomb(s, np.zeros((1, 64), dtype=np.uint8))


def test_device_forms_pass_the_host_point():
    ctx = _Ctx()
    cv = ecgpu.Curve(ctx, ecgpu.K256)
    key = np.arange(64, dtype=np.uint8).reshape(1, 64)
    cv.mul_device(0xD0000000, key, 0xD0100000, 9, flags=ecgpu.SHARED_POINTS)
    cv.ecdsa_verify_device(0xD0000000, 0xD0100000, key.tobytes(), 0xD0200000, 9, flags=ecgpu.SHARED_POINTS | ecgpu.ECDSA_LOW_S)
    cv.ecdsa_verify(np.zeros((3, 32), dtype=np.uint8), np.zeros((3, 64), dtype=np.uint8), key, flags=ecgpu.SHARED_POINTS)
    (n1, a1), (n2, a2), (n3, a3) = ctx.calls
    assert n1 == "ecgpu_mul_batch" and _value(a1[8]) == 9 and _value(a1[9]) == ecgpu.DEVICE and ctypes.string_at(_value(a1[3]), 64) == key.tobytes()
    assert n2 == "ecgpu_ecdsa_verify_batch" and _value(a2[6]) == 9 and _value(a2[7]) == ecgpu.DEVICE and ctypes.string_at(_value(a2[4]), 64) == key.tobytes()
    assert n3 == "ecgpu_ecdsa_verify_batch" and _value(a3[6]) == 3 and _value(a3[7]) == ecgpu.HOST and ctypes.string_at(_value(a3[4]), 64) == key.tobytes()


def test_group_lincomb_refuses_the_flag():
    class _Group(ecgpu.Group):
        def __init__(self):                                               # no devices: the refusal comes before any call
            self.calls = []
            self.lib, self.handle = _Lib(self.calls), ctypes.c_void_p(0x7E580000)

        def __del__(self):
            pass

    g = _Group()
    with pytest.raises(ValueError):
        g.lincomb("k256", np.zeros((4, 32), dtype=np.uint8), np.zeros((1, 64), dtype=np.uint8), flags=ecgpu.SHARED_POINTS)
    with pytest.raises(ValueError):
        g.mul("k256", np.zeros((4, 32), dtype=np.uint8), np.zeros((1, 64), dtype=np.uint8), flags=ecgpu.SHARED_POINTS)
    assert g.calls == []
