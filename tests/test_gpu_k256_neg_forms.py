"""GPU parity of the k256 throughput schedule (k256_mul_fast_kernel) on scalars that drive its sign-tracking accumulator through
its edge paths: zero digits (the accumulator's sign is left as it is), an accumulator at infinity at the first addition and again
after k = 0 mod n, long runs of doublings between sparse digits, and the GLV halves with one of them zero.  Checked against the
affine double-and-add model of the oracle."""
import random

import numpy as np
import pytest

from oracle import ecmodel as M
from oracle import synth

pytestmark = pytest.mark.gpu

C = M.K256
N, P = C.n, C.p


@pytest.fixture(scope="module")
def curve():
    import ecgpu
    ctx = ecgpu.Context(0)
    yield ctx.curve("k256")
    ctx.close()


def edge_scalars():
    ks = [0, 1, 2, 3, 4, 5, 16, 17, 31, 32, 33, N - 1, N - 2, N - 3, N - 16, N - 32, (N - 1) // 2, (N + 1) // 2,
          2**128 - 1, 2**128, 2**128 + 1, 2**255, 2**256 - 1 - N]
    ks += [32**j for j in range(52)]                                  # one non-zero digit, every other one zero
    ks += [(32**j) * 31 for j in range(0, 51, 5)]
    ks += [N - 32**j for j in range(0, 51, 5)]
    ks += [2**j - 1 for j in range(1, 256, 17)]
    return [k % N for k in ks]


def test_mul_fast_edge_scalars(curve):
    rng = random.Random(2027)
    ks = edge_scalars()
    ks += [rng.randrange(N) for _ in range(512 - len(ks))]
    pts = [synth.point(C, 9000 + i, seed=13) for i in range(len(ks))]
    sb = np.frombuffer(b"".join(M.i2b(C, k) for k in ks), dtype=np.uint8).reshape(-1, 32).copy()
    pb = np.frombuffer(b"".join(M.i2b(C, x) + M.i2b(C, y) for x, y in pts), dtype=np.uint8).reshape(-1, 64).copy()
    xy, inf = curve.mul(sb, pb)
    for i, (k, p) in enumerate(zip(ks, pts)):
        want = M.affine_mul(C, k, p)
        if want is None:
            assert inf[i] == 1 and not any(bytes(xy[i])), (i, hex(k))
        else:
            assert inf[i] == 0 and bytes(xy[i]) == M.i2b(C, want[0]) + M.i2b(C, want[1]), (i, hex(k))
