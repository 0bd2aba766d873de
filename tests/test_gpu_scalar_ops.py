"""ecgpu_scalar_op_batch and ecgpu_scalar_reduce_batch on an MI355X against Python integers (tests/scalar_ops_model.py), for the three
group orders: every op on 2^16 random elements plus the edges, the `ok` bytes included; batched inversion across partial lane batches
and the grid tail, with zeros and invalid values scattered through the batch; device- against host-memory calls byte for byte; every
reduction width with and without ECGPU_REDUCE_NONZERO and the FromOkm widths; staging hygiene and the argument errors."""
import ctypes
import random

import numpy as np
import pytest

import field_edge_vectors as V
import scalar_ops_model as S

pytestmark = pytest.mark.gpu

CURVES = ["k256", "p256", "p384"]
NRAND = 2**16
ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


def enc(vals, nb):
    return np.frombuffer(b"".join(int(v).to_bytes(nb, "big") for v in vals), dtype=np.uint8).reshape(len(vals), nb).copy()


def dec(arr):
    return [int.from_bytes(bytes(r), "big") for r in arr]


def operands(curve, op, seed):
    n, L = V.SCALAR_FIELDS[curve]
    rng = random.Random(seed)
    if op in S.BINARY:
        ps = S.edge_pairs(curve)
    else:
        ps = [(x, 0) for x in S.edge_values(curve)] + [(a, 0) for a, _ in V.quotient_digit_pairs(n, L)]
    nrand = NRAND if op != S.SQRT else NRAND // 4
    ps += [(rng.randrange(n), rng.randrange(n)) for _ in range(nrand)]
    if op == S.SQRT:
        ps += [(rng.randrange(n) ** 2 % n, 0) for _ in range(nrand)]
    return [p[0] for p in ps], [p[1] for p in ps]


@pytest.mark.parametrize("op", ["mul", "sqr", "add", "sub", "neg", "inv", "sqrt"])
@pytest.mark.parametrize("curve", CURVES)
def test_scalar_op_exact(ctx, curve, op):
    code = S.OPS[op]
    cv = ctx.curve(curve)
    a, b = operands(curve, code, seed=S.CURVE_INDEX[curve] * 10 + code)
    out, ok = cv.scalar_op(code, enc(a, cv.nb), enc(b, cv.nb) if code in S.BINARY else None)
    got = dec(out)
    bad = [(hex(x), hex(y), hex(g), int(k)) for x, y, g, k in zip(a, b, got, ok) if (g, int(k)) != S.expected(curve, code, x, y)]
    assert not bad, (curve, op, len(bad), bad[:4])


@pytest.mark.parametrize("count", [1, 2**20 + 7])
@pytest.mark.parametrize("curve", CURVES)
def test_inversion_batches_and_tail(ctx, curve, count):
    """partial lane batches and the grid tail; zeros and invalid values scattered through the batch give 0 / ok 0 and leave
    every other element exact"""
    n, L = V.SCALAR_FIELDS[curve]
    cv = ctx.curve(curve)
    g = np.random.default_rng(count + L)
    raw = g.integers(0, 256, (count, cv.nb), dtype=np.uint8)
    raw[:, 0] &= 0x7F                                   # below 2^(8 NB - 1) < n
    if count > 1:
        for pos, val in ((0, 0), (count - 1, 0), (count // 2, n), (count // 3, 2**(32 * L) - 1), (5, n + 1)):
            raw[pos] = np.frombuffer(int(val).to_bytes(cv.nb, "big"), dtype=np.uint8)
        scatter = g.choice(count, 4096, replace=False)
        raw[scatter[:2048]] = 0
        raw[scatter[2048:]] = 0xFF                      # 2^(8 NB) - 1 >= n
    out, ok = cv.scalar_op(S.INV, raw)
    vals, got = dec(raw), dec(out)
    bad = [(i, hex(x)) for i, (x, y, k) in enumerate(zip(vals, got, ok)) if (y, int(k)) != S.expected(curve, S.INV, x)]
    assert not bad, (curve, count, len(bad), bad[:4])
    if count > 1:
        assert int(ok.sum()) < count - 4000        # the scattered rejects are there


@pytest.mark.parametrize("curve", CURVES)
def test_device_memory_matches_host_memory(ctx, curve):
    import torch
    cv = ctx.curve(curve)
    n, L = V.SCALAR_FIELDS[curve]
    rng = random.Random(17)
    cnt = 50_003
    a = [rng.choice([0, n, rng.randrange(n)]) if rng.random() < 0.05 else rng.randrange(n) for _ in range(cnt)]
    b = [rng.randrange(n) for _ in range(cnt)]
    ha, hb = enc(a, cv.nb), enc(b, cv.nb)
    da, db = torch.from_numpy(ha).cuda(), torch.from_numpy(hb).cuda()
    for code in range(7):
        ho, hk = cv.scalar_op(code, ha, hb if code in S.BINARY else None)
        do = torch.zeros((cnt, cv.nb), dtype=torch.uint8, device="cuda")
        dk = torch.zeros(cnt, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        cv.scalar_op_device(code, da, db if code in S.BINARY else None, do, dk, cnt)
        ctx.synchronize()
        assert np.array_equal(do.cpu().numpy(), ho) and np.array_equal(dk.cpu().numpy(), hk), (curve, code)
    # ok may be NULL
    do = torch.zeros((cnt, cv.nb), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cv.scalar_op_device(S.INV, da, None, do, None, cnt)
    ctx.synchronize()
    assert np.array_equal(do.cpu().numpy(), cv.scalar_op(S.INV, ha)[0])


@pytest.mark.parametrize("nonzero", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_reduce_every_width(ctx, curve, nonzero):
    cv = ctx.curve(curve)
    for in_bytes in range(1, 2 * cv.nb + 1):
        vals = S.wide_inputs(curve, in_bytes, 2000, seed=in_bytes * 5 + nonzero)
        out = cv.scalar_reduce(enc(vals, in_bytes), nonzero=nonzero)
        got = dec(out)
        bad = [(hex(x), hex(y)) for x, y in zip(vals, got) if y != S.expected_reduce(curve, x, nonzero)]
        assert not bad, (curve, in_bytes, nonzero, bad[:3])


@pytest.mark.parametrize("curve", CURVES)
def test_reduce_from_okm(ctx, curve):
    n, _ = V.SCALAR_FIELDS[curve]
    cv = ctx.curve(curve)
    width, recs = S.okm_inputs(curve, 20000, seed=11)
    raw = np.frombuffer(b"".join(r for r, _ in recs), dtype=np.uint8).reshape(len(recs), width).copy()
    got = dec(cv.scalar_reduce(raw))
    assert got == [ref % n for _, ref in recs]


@pytest.mark.parametrize("curve", CURVES)
def test_host_staging_is_cleared(ctx, curve):
    cv = ctx.curve(curve)
    n, _ = V.SCALAR_FIELDS[curve]
    rng = random.Random(3)
    cnt = 4099
    a = enc([rng.randrange(1, n) for _ in range(cnt)], cv.nb)
    b = enc([rng.randrange(1, n) for _ in range(cnt)], cv.nb)
    for code in range(7):
        cv.scalar_op(code, a, b if code in S.BINARY else None)
        for slot in (0, 1, 2, 3):
            assert not any(ctx.debug_workspace(16 + slot)), (curve, code, slot)
    cv.scalar_reduce(np.concatenate([a, b], axis=1), nonzero=True)
    for slot in (0, 2):
        assert not any(ctx.debug_workspace(16 + slot)), (curve, "reduce", slot)


def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.handle
    buf = np.zeros(4 * 96, dtype=np.uint8)
    p = ctypes.cast(buf.ctypes.data, ctypes.POINTER(ctypes.c_uint8))
    for curve, nb in ((0, 32), (1, 32), (2, 48)):
        assert lib.ecgpu_scalar_op_batch(h, curve, 7, p, p, p, p, 1, 0) == ERR_ARG
        assert lib.ecgpu_scalar_op_batch(h, curve, -1, p, p, p, p, 1, 0) == ERR_ARG
        for op in S.BINARY:
            assert lib.ecgpu_scalar_op_batch(h, curve, op, p, None, p, p, 1, 0) == ERR_ARG
        assert lib.ecgpu_scalar_reduce_batch(h, curve, p, 0, p, 1, 0, 0) == ERR_ARG
        assert lib.ecgpu_scalar_reduce_batch(h, curve, p, 2 * nb + 1, p, 1, 0, 0) == ERR_ARG
        assert lib.ecgpu_scalar_reduce_batch(h, curve, p, nb, p, 1, 0, 2) == ERR_ARG
        assert lib.ecgpu_scalar_reduce_batch(h, curve, p, nb, p, 1, 0, 0x101) == ERR_ARG
        # the unary ops take b = NULL, ok = NULL
        assert lib.ecgpu_scalar_op_batch(h, curve, S.NEG, p, None, p, None, 1, 0) == 0
        assert lib.ecgpu_scalar_reduce_batch(h, curve, p, 2 * nb, p, 1, 0, 1) == 0
