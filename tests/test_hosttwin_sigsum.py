"""csrc/affine_ops.hpp on the host twin (tests/hosttwin/hosttwin_sigsum.cpp) against the oracle, on the rows of
tests/signature_edge_vectors.py: the affine sum A + B of every row's two products is word for word ecmodel.affine_add, through the
batched driver in the kernels' lane layout and through sum_kind + slope_terms alone, and the ECGPU_EXC_NOTE counters show each
class reaching exactly the site it names - which is what lets tests/test_gpu_signature_edges.py claim that the same rows reach those
arms on the device, where the hook is empty.  Then y from x and the curve check."""
import ctypes
import functools

import pytest

import signature_edge_vectors as V
from hosttwin_util import lib, buf, outbuf
from oracle import ecmodel as M
from related_point_hostwalks import exc_counts, exc_reset

CURVES = ["k256", "p256", "p384"]
KINDS = [(cn, kind) for cn in CURVES for kind in ("ecdsa", "recover")] + [("k256", "schnorr")]
SITE = {"same": "affsum.same", "opp": "affsum.opp", "inf": "affsum.one_inf", "chord": "affsum.chord", "chord_bad": "affsum.chord"}
P = ctypes.c_void_p


def _pt(c, A):
    return bytes(2 * c.nbytes) if A is None else M.i2b(c, A[0]) + M.i2b(c, A[1])


def _sum(c, rs, T, batched=True):
    """(sums, kinds) of the rows' products; a rejected row comes with ok = 0, as its prep kernel leaves it"""
    n = len(rs)
    a, b = buf(b"".join(_pt(c, r.A) for r in rs)), buf(b"".join(_pt(c, r.B) for r in rs))
    ai, bi = buf(bytes(r.A is None for r in rs)), buf(bytes(r.B is None for r in rs))
    ok = buf(bytes(r.cls != "rejected" for r in rs))
    out, kinds = outbuf(2 * c.nbytes * n), outbuf(n)
    if batched:
        f = lib().ht_aff_sum_batch
        f.argtypes = [ctypes.c_int, P, P, P, P, P, ctypes.c_size_t, ctypes.c_size_t, P, P]
        assert f(M.CURVE_IDS[c.name], a, ai, b, bi, ok, n, T, out, kinds) == 0
    else:
        f = lib().ht_aff_sum_each
        f.argtypes = [ctypes.c_int, P, P, P, P, ctypes.c_size_t, P, P]
        assert f(M.CURVE_IDS[c.name], a, ai, b, bi, n, out, kinds) == 0
    w = 2 * c.nbytes
    return [bytes(out)[w * i:w * (i + 1)] for i in range(n)], list(bytes(kinds))


def _want_kind(r):
    if r.cls == "rejected" or (r.A is None and r.B is None):
        return 0
    if r.A is None or r.B is None:
        return 1
    return 0 if r.cls == "opp" else 3 if r.cls == "same" else 2


@pytest.mark.parametrize("cn,kind", KINDS)
def test_rows_per_class(cn, kind):
    rs = V.rows(cn, kind)
    assert len(rs) == V.N == 1031
    assert V.class_counts(rs) == {"same": 14, "opp": 14, "inf": 14, "rejected": 13, "chord_bad": 324, "chord": 652} == V.COUNTS
    cls = V.layout()
    for lane in V.MIXED:                                      # one element of every kind in the lane's one batch
        assert {cls[lane + V.T * b] for b in range(4)} == set(V.KINDS4)
    assert [cls[i] for i in (0, 256, 512, 768, 1024)] == ["same", "opp", "inf", "chord", "same"]
    assert len({lane // 64 for lane in V.MIXED}) == 4
    for r in rs:                                              # the classes are what their names say, by the oracle
        c = M.CURVES[cn]
        if r.cls in ("same", "chord", "chord_bad"):
            assert r.A is not None and r.B is not None and (r.A == r.B) == (r.cls == "same")
        if r.cls == "opp":
            assert r.A == M.affine_neg(c, r.B) and r.A != r.B and not r.want
        if r.cls == "inf":
            assert (r.A is None) != (r.B is None) and r.want
        if r.cls == "rejected":
            assert not r.want
        if r.cls in ("same", "chord"):
            assert r.want
    assert not any(r.want for r in rs if r.cls == "chord_bad") or kind == "recover"      # the other root recovers another key


@pytest.mark.parametrize("cn,kind", KINDS)
@pytest.mark.parametrize("n", V.SIZES)
def test_batched_sum_equals_affine_add(cn, kind, n):
    c = M.CURVES[cn]
    rs = V.rows(cn, kind)[:n]
    out, kinds = _sum(c, rs, V.T)
    for i, r in enumerate(rs):
        want = None if r.cls == "rejected" else M.affine_add(c, r.A, r.B)
        assert out[i] == _pt(c, want), (cn, kind, i, r.cls)
        assert kinds[i] == _want_kind(r), (cn, kind, i, r.cls)
    if kind == "recover":                                     # the sum is the recovered key
        assert all(out[i] == _pt(c, r.want) for i, r in enumerate(rs))


@pytest.mark.parametrize("cn,kind", KINDS)
def test_sum_from_kind_and_slope_terms(cn, kind):
    """the inversion-free verifier's two calls (ecdsa::verify_check_kernel), finished with an inversion of their own"""
    c = M.CURVES[cn]
    rs = [r for r in V.rows(cn, kind) if r.cls != "rejected"]
    rs = [r for r in rs if r.cls in V.EXCEPTIONAL] + [r for r in rs if r.cls not in V.EXCEPTIONAL][:64]
    out, kinds = _sum(c, rs, 0, batched=False)
    for i, r in enumerate(rs):
        assert out[i] == _pt(c, M.affine_add(c, r.A, r.B)) and kinds[i] == _want_kind(r), (cn, kind, i, r.cls)


@pytest.mark.parametrize("cn,kind", KINDS)
@pytest.mark.parametrize("batched", [True, False])
def test_each_class_reaches_the_site_it_names(cn, kind, batched):
    c = M.CURVES[cn]
    by_cls = {}
    for r in V.rows(cn, kind):
        by_cls.setdefault(r.cls, []).append(r)
    for cls, part in by_cls.items():
        if cls == "rejected" and not batched:
            continue                                          # the unbatched callers skip a rejected element before classifying it
        exc_reset()
        _sum(c, part, V.T, batched)
        want = {} if cls == "rejected" else {SITE[cls]: len(part)}
        assert exc_counts() == want, (cn, kind, cls)
    both = [V.Row("both_inf", None, None, None, None)] * 8
    exc_reset()
    out, kinds = _sum(c, both, V.T, batched)
    assert exc_counts() == {"affsum.both_inf": 8} and kinds == [0] * 8 and not any(b"".join(out))
    exc_reset()


@functools.lru_cache(maxsize=None)
def _lift(cn):
    c = M.CURVES[cn]
    rows = V.lift_rows(cn)
    n, nb = len(rows), c.nbytes
    top = 1 << (8 * nb)
    xs = buf(b"".join((x % top).to_bytes(nb, "big") for x, _ in rows))
    odd = buf(bytes(o for _, o in rows))
    canon, has, roots, lifted = outbuf(n), outbuf(n), outbuf(2 * nb * n), outbuf(nb * n)
    f = lib().ht_aff_lift
    f.argtypes = [ctypes.c_int, P, P, ctypes.c_size_t, P, P, P, P]
    exc_reset()
    assert f(M.CURVE_IDS[cn], xs, odd, n, canon, has, roots, lifted) == 0
    counts = exc_counts()
    exc_reset()
    return rows, bytes(canon), bytes(has), bytes(roots), bytes(lifted), counts


@pytest.mark.parametrize("cn", CURVES)
def test_lift_x_and_sqrt_rhs(cn):
    c = M.CURVES[cn]
    nb = c.nbytes
    rows, canon, has, roots, lifted, counts = _lift(cn)
    no_root = 0
    for i, (x, odd) in enumerate(rows):
        assert canon[i] == (x < c.p), (cn, hex(x))
        want = M.decompress(c, x % c.p, odd)                  # the field element the kernels load from a non-canonical x is x mod p
        assert has[i] == (3 if want is not None else 0), (cn, hex(x))
        assert (M.decompress(c, x, odd) is not None) == bool(canon[i] and has[i])
        if want is None:
            no_root += 1
            continue
        y, ny = M.b2i(roots[2 * nb * i:2 * nb * i + nb]), M.b2i(roots[2 * nb * i + nb:2 * nb * (i + 1)])
        assert {y, ny} == {want[1], (c.p - want[1]) % c.p}
        assert M.b2i(lifted[nb * i:nb * (i + 1)]) == want[1] and (want[1] & 1) == odd
        if cn != "k256":                                      # the two roots sqrt_rhs hands the SEC1 tag-5 arm are the pair the oracle's smaller-root
            ok, pt = M.group_from_bytes(c, bytes([5]) + M.i2b(c, x % c.p))       # rule chooses from; the rule itself is the kernel's (sec1_kernels.hpp) and
            assert ok and pt[1] == min(y, ny)                                    # runs in tests/test_gpu_signature_edges.py only
    assert counts == {"lift.no_root": 2 * no_root} and no_root >= 16       # sqrt_rhs and lift_x, once each per x


@pytest.mark.parametrize("cn", CURVES)
def test_canonical_and_on_curve(cn):
    c = M.CURVES[cn]
    rows = V.curve_check_rows(cn)
    n, nb = len(rows), c.nbytes
    xy = buf(b"".join(x.to_bytes(nb, "big") + y.to_bytes(nb, "big") for x, y, _ in rows))
    canon, on = outbuf(n), outbuf(n)
    f = lib().ht_aff_curve_check
    f.argtypes = [ctypes.c_int, P, ctypes.c_size_t, P, P]
    assert f(M.CURVE_IDS[cn], xy, n, canon, on) == 0
    aliases = 0
    for i, (x, y, ok) in enumerate(rows):
        assert canon[i] == (x < c.p and y < c.p), (cn, i)
        assert on[i] == M.on_curve(c, (x % c.p, y % c.p)), (cn, i)
        assert bool(canon[i] and on[i]) == ok
        aliases += bool(on[i] and not canon[i])
    assert aliases >= 6 and sum(ok for _, _, ok in rows) == 12
