"""Scalar-field ops of csrc/scalar_ops.hpp (the per-element code of ecgpu_scalar_op_batch / ecgpu_scalar_reduce_batch), host build of
the device templates (tests/hosttwin), against Python integers on the edges and on random values, for the three group orders."""
import ctypes
import random

import numpy as np
import pytest

import field_edge_vectors as V
import scalar_ops_model as S
from hosttwin_util import lib

CURVES = ["k256", "p256", "p384"]
BATCHES = [1, 8, 16, 32]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_op(curve, op, a, b):
    n, L = V.SCALAR_FIELDS[curve]
    wa, wb = V.to_words(a, L), V.to_words(b, L)
    out = np.zeros((len(a), L), dtype=np.uint32)
    ok = np.zeros(len(a), dtype=np.uint8)
    assert lib().ht_sc_op(S.CURVE_INDEX[curve], op, _p(wa), _p(wb), _p(out), _p(ok), len(a)) == 0
    return V.from_words(out), list(ok)


def run_inv_lane(curve, batch, vals):
    n, L = V.SCALAR_FIELDS[curve]
    w = V.to_words(vals, L)
    out = np.zeros((len(vals), L), dtype=np.uint32)
    ok = np.zeros(len(vals), dtype=np.uint8)
    assert lib().ht_sc_inv_lane(S.CURVE_INDEX[curve], batch, _p(w), len(vals), _p(out), _p(ok)) == 0
    return V.from_words(out), list(ok)


def run_reduce(curve, vals, in_bytes, nonzero):
    n, L = V.SCALAR_FIELDS[curve]
    raw = np.frombuffer(b"".join(v.to_bytes(in_bytes, "big") for v in vals), dtype=np.uint8).copy()
    out = np.zeros((len(vals), L), dtype=np.uint32)
    assert lib().ht_sc_reduce(S.CURVE_INDEX[curve], int(nonzero), _p(raw), in_bytes, _p(out), len(vals)) == 0
    return V.from_words(out)


def check_ops(curve, op, pairs):
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    got, ok = run_op(curve, op, a, b)
    for x, y, g, k in zip(a, b, got, ok):
        assert (g, k) == S.expected(curve, op, x, y), (curve, op, hex(x), hex(y), hex(g), k)


@pytest.mark.parametrize("op", ["mul", "sqr", "add", "sub", "neg", "sqrt"])
@pytest.mark.parametrize("curve", CURVES)
def test_elementwise_op(curve, op):
    n, L = V.SCALAR_FIELDS[curve]
    code = S.OPS[op]
    rng = random.Random(len(curve) * 31 + code)
    if code in S.BINARY:
        pairs = S.edge_pairs(curve)
    else:
        pairs = [(x, 0) for x in S.edge_values(curve)] + [(a, 0) for a, _ in V.quotient_digit_pairs(n, L)]
    count = 300 if code == S.SQRT else 3000
    pairs += [(rng.randrange(n), rng.randrange(n)) for _ in range(count)]
    if code == S.SQRT:   # squares, so that the root path runs as often as the rejection
        pairs += [(rng.randrange(n) ** 2 % n, 0) for _ in range(count)]
    check_ops(curve, code, pairs)


@pytest.mark.parametrize("curve", CURVES)
def test_rejected_operands(curve):
    n, L = V.SCALAR_FIELDS[curve]
    bad = [n, n + 1, 2**(32 * L) - 1]
    for op in (S.MUL, S.SQR, S.ADD, S.SUB, S.NEG, S.SQRT):
        pairs = [(x, 1) for x in bad] + ([(1, x) for x in bad] if op in S.BINARY else [])
        got, ok = run_op(curve, op, [p[0] for p in pairs], [p[1] for p in pairs])
        assert got == [0] * len(pairs) and ok == [0] * len(pairs), (curve, op)


def test_root_of_unity_and_sqrt_model():
    """the model's constants come from the generator; the roots it returns are roots"""
    for curve in CURVES:
        n, _ = V.SCALAR_FIELDS[curve]
        s, t = S.two_adicity(n)
        z = S.root_of_unity(curve)
        assert pow(z, 2**s, n) == 1 and (s == 0 or pow(z, 2**(s - 1), n) != 1)
        rng = random.Random(s)
        for _ in range(50):
            a = rng.randrange(n)
            r, ok = S.sqrt_ref(curve, a)
            assert ok == (pow(a, (n - 1) // 2, n) in (0, 1)) and (not ok or r * r % n == a)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("curve", CURVES)
def test_inv_lane_every_count(curve, batch):
    n, L = V.SCALAR_FIELDS[curve]
    rng = random.Random(batch * 7 + L)
    edges = S.edge_values(curve)
    for cnt in range(1, batch + 1):
        vals = [rng.choice(edges) if rng.random() < 0.3 else rng.randrange(n) for _ in range(cnt)]
        got, ok = run_inv_lane(curve, batch, vals)
        for x, g, k in zip(vals, got, ok):
            assert (g, k) == S.expected(curve, S.INV, x), (curve, batch, cnt, hex(x))


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("curve", CURVES)
def test_inv_lane_zero_positions(curve, batch):
    """a zero (or an invalid value) at the first, a middle and the last position, and a lane of zeros, leave the others exact"""
    n, L = V.SCALAR_FIELDS[curve]
    rng = random.Random(batch + 100 * L)
    cases = [[0] * batch]
    for pos in sorted({0, batch // 2, batch - 1}):
        for bad in (0, n, 2**(32 * L) - 1):
            v = [rng.randrange(1, n) for _ in range(batch)]
            v[pos] = bad
            cases.append(v)
    for vals in cases:
        got, ok = run_inv_lane(curve, batch, vals)
        for x, g, k in zip(vals, got, ok):
            assert (g, k) == S.expected(curve, S.INV, x), (curve, batch, hex(x))


def test_default_batch_is_measured_variant():
    assert lib().ht_sc_inv_default_batch() in BATCHES


@pytest.mark.parametrize("nonzero", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_reduce_every_width(curve, nonzero):
    n, L = V.SCALAR_FIELDS[curve]
    for in_bytes in range(1, 8 * L + 1):
        vals = S.wide_inputs(curve, in_bytes, 40, seed=in_bytes * 3 + nonzero)
        got = run_reduce(curve, vals, in_bytes, nonzero)
        for x, g in zip(vals, got):
            assert g == S.expected_reduce(curve, x, nonzero), (curve, in_bytes, nonzero, hex(x), hex(g))


@pytest.mark.parametrize("curve", CURVES)
def test_reduce_nonzero_residues(curve):
    """inputs = 0 and = n - 2 (mod n - 1) at every width: the results 1 and n - 1 at both ends of the range"""
    n, L = V.SCALAR_FIELDS[curve]
    m = n - 1
    for in_bytes in range(1, 8 * L + 1):
        top = 2**(8 * in_bytes)
        qs = [0, 1, 2, (top - 1) // m, (top - 1) // m - 1]
        vals = sorted({q * m + r for q in qs for r in (0, m - 1) if 0 <= q * m + r < top})
        if not vals:
            continue
        got = run_reduce(curve, vals, in_bytes, True)
        for x, g in zip(vals, got):
            assert g == x % m + 1 and g in (1, n - 1), (curve, in_bytes, hex(x))


@pytest.mark.parametrize("curve", CURVES)
def test_from_okm_reduction(curve):
    width, recs = S.okm_inputs(curve, 200, seed=7)
    n, _ = V.SCALAR_FIELDS[curve]
    got = run_reduce(curve, [int.from_bytes(r, "big") for r, _ in recs], width, False)
    for (raw, ref), g in zip(recs, got):
        assert g == ref % n


@pytest.mark.parametrize("curve", CURVES)
def test_fold_constants_and_bound(curve):
    """C = 2^(32 L) mod (n - 1), and NF folds take every value below 2^(64 L) below 2^(32 L), with a tight bound per fold"""
    n, L = V.SCALAR_FIELDS[curve]
    c = np.zeros(8, dtype=np.uint32)
    cw, nf = ctypes.c_int(), ctypes.c_int()
    assert lib().ht_sc_fold_params(S.CURVE_INDEX[curve], _p(c), ctypes.byref(cw), ctypes.byref(nf)) == 0
    R, m = 2**(32 * L), n - 1
    assert V.from_words(c[:cw.value].reshape(1, -1))[0] == R % m and R % m < 2**(32 * cw.value)
    M = 2**(64 * L) - 1                     # largest value before a fold
    for _ in range(nf.value):
        H = M // R
        M = max((H - 1) * (R % m) + R - 1 if H else 0, H * (R % m) + M - H * R)
    assert M < R

