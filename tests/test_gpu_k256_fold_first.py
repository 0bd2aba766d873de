"""GPU side of tests/test_hosttwin_k256_fold_first.py: the k256 products whose columns start with the products that cannot
carry, on the inputs that maximise every column (tests/k256_fold_vectors.py), through FE_MUL / FE_SQR, the point operations
(whose formulas use mul and mul_add2) and the variable-base scalar multiplication (the doubling's mul_add_sqr).  Bit-exact
against Python integers and the oracle."""
import random

import numpy as np
import pytest

from oracle import ecmodel as M
from oracle import synth
import k256_fold_vectors as V

pytestmark = pytest.mark.gpu

C = M.K256
P = C.p


@pytest.fixture(scope="module")
def curve():
    import ecgpu
    ctx = ecgpu.Context(0)
    yield ctx.curve("k256")
    ctx.close()


def arr(vals, width=32):
    return np.frombuffer(V.to_bytes(vals), dtype=np.uint8).reshape(-1, width).copy()


def to_ints(a):
    return [int.from_bytes(bytes(r), "big") for r in a]


def test_field_mul_sqr_maximal_columns(curve):
    import ecgpu
    ps = V.pairs()
    a, b = [p[0] for p in ps], [p[1] for p in ps]
    assert to_ints(curve.field_op(ecgpu.FE_MUL, arr(a), arr(b))) == [x * y % P for x, y in ps]
    assert to_ints(curve.field_op(ecgpu.FE_SQR, arr(a))) == [x * x % P for x in a]


def coords(rng, n):
    """field elements below p with extreme limbs (the point formulas read canonical coordinates)"""
    out = [v for v in V.EDGES if 0 < v < P]
    while len(out) < n:
        v = V.extreme(rng) % P
        out.append(v if v else 1)
    return out[:n]


def test_point_ops_maximal_columns(curve):
    rng = random.Random(41)
    n = 400
    cs = coords(rng, 3 * n)
    ps = [tuple(cs[3 * i:3 * i + 3]) for i in range(n)]
    qs = [tuple(cs[3 * ((i * 7 + 3) % n):3 * ((i * 7 + 3) % n) + 3]) for i in range(n)]
    pa = np.frombuffer(b"".join(M.proj_bytes(C, p) for p in ps), dtype=np.uint8).reshape(-1, 96).copy()
    qa = np.frombuffer(b"".join(M.proj_bytes(C, q) for q in qs), dtype=np.uint8).reshape(-1, 96).copy()
    assert bytes(curve.add(pa, qa)) == b"".join(M.proj_bytes(C, M.k256_add(p, q)) for p, q in zip(ps, qs))
    assert bytes(curve.double(pa)) == b"".join(M.proj_bytes(C, M.k256_double(p)) for p in ps)
    aff = [(q[0], q[1], 0) for q in qs]
    xa = np.frombuffer(b"".join(M.i2b(C, x) + M.i2b(C, y) for x, y, _ in aff), dtype=np.uint8).reshape(-1, 64).copy()
    assert bytes(curve.add_mixed(pa, xa)) == b"".join(M.proj_bytes(C, M.k256_add_mixed(p, a)) for p, a in zip(ps, aff))


def test_scalar_mul_extreme_scalars(curve):
    n = 48
    ks = [C.n - 1, C.n - 2, 2**255, 2**256 - 2**128 - 1, 1, 2, 3, 2**32 - 1] + synth.scalars(C, n - 8)
    ks = [k % C.n or 1 for k in ks]
    pts = synth.points(C, n)
    sb = np.frombuffer(b"".join(M.i2b(C, k) for k in ks), dtype=np.uint8).reshape(n, 32).copy()
    pb = np.frombuffer(b"".join(M.i2b(C, x) + M.i2b(C, y) for x, y in pts), dtype=np.uint8).reshape(n, 64).copy()
    xy, inf = curve.mul(sb, pb)
    for i in range(n):
        w = M.affine_mul(C, ks[i], pts[i])
        assert bytes(xy[i]) == M.i2b(C, w[0]) + M.i2b(C, w[1]) and inf[i] == 0, i
