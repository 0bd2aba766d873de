"""Host build of the k256 products whose columns start with the products that cannot carry (the fold product h[K] * 977 of
each low column, the first product of high column 8, and the s_i d_8 terms of mul_add_sqr): mul, mul_add2 and mul_add_sqr
against Python integers on inputs that maximise every column (tests/k256_fold_vectors.py).  The host build drops the carry
of those products exactly as the device code does, so a bound that did not hold would show here as a wrong value."""
import pytest

from hosttwin_util import lib, buf, outbuf
import k256_fold_vectors as V

P = V.P


def run(op, a, b, e, f):
    n = len(a)
    out = outbuf(32 * n)
    assert lib().ht_k256_fold_first_op(op, buf(V.to_bytes(a)), buf(V.to_bytes(b)), buf(V.to_bytes(e)), buf(V.to_bytes(f)), out, n) == 0
    o = bytes(out)
    return [int.from_bytes(o[32 * i:32 * i + 32], "big") for i in range(n)]


def test_mul_maximal_columns():
    ps = V.pairs()
    a, b = [p[0] for p in ps], [p[1] for p in ps]
    got = run(0, a, b, a, b)
    for i, (x, y) in enumerate(ps):
        assert got[i] % P == x * y % P, (i, hex(x), hex(y))


@pytest.mark.parametrize("op", [1, 2], ids=["mul_add2", "mul_add_sqr"])
def test_two_product_forms_maximal_columns(op):
    qs = V.quads()
    a, b, e, f = ([q[k] for q in qs] for k in range(4))
    got = run(op, a, b, e, f)
    for i, (x, y, u, v) in enumerate(qs):
        want = (x * y + (u * v if op == 1 else u * u)) % P
        assert got[i] % P == want, (op, i, hex(x), hex(y), hex(u), hex(v))


def test_vectors_reach_the_column_extremes():
    """the vectors do what they are for: all-ones high halves, sums above 2^512, square operands with the top bit set"""
    ps, qs = V.pairs(), V.quads()
    assert any((x * y) >> 256 >= 2**256 - 2 for x, y in ps)
    assert any((x * y + u * v) >> 256 == 2**256 - 1 for x, y, u, v in qs)
    assert any(x * y + u * v >= 2**512 for x, y, u, v in qs)
    assert any(x * y + u * u >= 2**512 for x, y, u, _ in qs)
    assert sum(u >> 255 for _, _, u, _ in qs) > 100
