"""The field and scalar primitives as the kernels run them (tests/devtwin: gfx950 build with the inline-asm column forms of
mp32_cols.inc), in the three configurations the product compiles: the throughput build, the branch-free build of the secret-scalar
kernels (ECGPU_K256_BRANCHFREE: the rare carry blocks run on every call) and the grouped instruction order (ECGPU_MAC_GROUPED).
Inputs: the edges of tests/field_edge_vectors.py (carry extremes, quotient digits 0 / 2^32 - 1, P-384's negative accumulator,
every k256 rare carry path) plus 2^16 random inputs per op.

- k256: every raw output is below 2^256 and congruent to the exact result mod p, bit-identical to the host twin (the portable
  fallback of the same templates) and, in the other two builds, to the throughput build.
- Montgomery and scalar fields: every output equals the exact Python-integer result and is below the modulus.
- mac_cols<M, FRESH, NC>: every form gives (c_in + sum pa pb) mod 2^96 exactly."""
import random

import numpy as np
import pytest

import field_edge_vectors as V
import devtwin_util as D

pytestmark = pytest.mark.gpu

NRAND = 2**16
BUILDS = ["default", "bf", "grouped"]
P = V.K256_P
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ---- k256 -------------------------------------------------------------------------------------------------------------------
def random_raw(g, n):
    """n x 8 words: uniform words, or words drawn from the extremes"""
    w = g.integers(0, 2**32, (n, 8), dtype=np.uint64)
    ext = np.array(V.WORDS, dtype=np.uint64)
    pick = g.random((n, 1)) < 0.4
    w = np.where(pick & (g.random((n, 8)) < 0.8), ext[g.integers(0, len(ext), (n, 8))], w)
    return w.astype(np.uint32)


def k256_inputs():
    rows = list(V.quads())
    rows += [(x, y, y, x) for x, y in V.pairs()]
    for ts in V.k256_rare_inputs().values():
        rows += [tuple(t) + (0,) * (4 - len(t)) for t in ts]
    edge = [V.to_words([r[k] for r in rows], 8) for k in range(4)]
    g = np.random.default_rng(2024)
    rnd = [random_raw(g, NRAND) for _ in range(4)]
    return [np.concatenate([e, r]) for e, r in zip(edge, rnd)]


def k256_ints():
    return cached("k256_ints", lambda: [V.from_words(x) for x in cached("k256_in", k256_inputs)])


def run_k256(side, op):
    fn = D.host()["k256"] if side == "host" else D.device(side)["k256"]
    return cached(("k256", side, op), lambda: D.k256_op(fn, op, *cached("k256_in", k256_inputs)))


K256_EXPECT = {
    "mul": lambda a, b, e, f: a * b, "sqr": lambda a, b, e, f: a * a, "add": lambda a, b, e, f: a + b,
    "sub": lambda a, b, e, f: a - b, "neg": lambda a, b, e, f: -a, "mul_small": lambda a, b, e, f: a * (b & V.MASK32),
    "shl1": lambda a, b, e, f: 2 * a, "shl2": lambda a, b, e, f: 4 * a, "shl3": lambda a, b, e, f: 8 * a,
    "mul_add2": lambda a, b, e, f: a * b + e * f, "mul_add_sqr": lambda a, b, e, f: a * b + e * e,
    "sub2": lambda a, b, e, f: a - b - e, "fold_top_fast": lambda a, b, e, f: a + V.fold_t(b) * V.K256_C,
    "normalize": lambda a, b, e, f: a, "is_zero_fast": lambda a, b, e, f: a,
}


@pytest.mark.parametrize("op", D.K256_OPS)
def test_k256_device_is_exact(op):
    out = run_k256("default", op)
    got = V.from_words(out[:, :8])
    flags = out[:, 8]
    a, b, e, f = k256_ints()
    for i, g in enumerate(got):
        x = a[i]
        if op == "inv":
            ok = g * x % P == 1 if x % P else g % P == 0
        elif op == "half":
            ok = (2 * g - x) % P == 0
        elif op == "sqrt":
            sq = g * g % P
            ok = sq == x % P if flags[i] else (sq == -x % P and x % P != 0)
        elif op == "normalize":
            ok = g == x % P
        elif op == "is_zero_fast":
            ok = g == x and bool(flags[i]) == (x % P == 0)
        else:
            ok = (g - K256_EXPECT[op](x, b[i], e[i], f[i])) % P == 0
        assert ok, (op, i, hex(x), hex(b[i]), hex(e[i]), hex(f[i]), hex(g), int(flags[i]))
    if op not in ("sqrt", "is_zero_fast"):
        assert not flags.any(), op


@pytest.mark.parametrize("op", D.K256_OPS)
def test_k256_device_matches_host_twin(op):
    dev, hst = run_k256("default", op), run_k256("host", op)
    bad = np.nonzero((dev != hst).any(axis=1))[0]
    assert bad.size == 0, (op, bad.size, int(bad[0]), dev[bad[0]].tolist(), hst[bad[0]].tolist())


@pytest.mark.parametrize("build", ["bf", "grouped"])
@pytest.mark.parametrize("op", D.K256_OPS)
def test_k256_builds_agree(op, build):
    dev, other = run_k256("default", op), run_k256(build, op)
    bad = np.nonzero((dev != other).any(axis=1))[0]
    assert bad.size == 0, (op, build, bad.size, int(bad[0]), dev[bad[0]].tolist(), other[bad[0]].tolist())


# ---- Montgomery fields ------------------------------------------------------------------------------------------------------
def mont_inputs(curve):
    m, L = V.MONT_FIELDS[curve]
    rows = V.edge_pairs(m, L) + V.quotient_digit_pairs(m, L) + [(s, s) for s in V.quotient_digit_squares(m, L)]
    rng = random.Random(len(curve))
    rows += [(rng.randrange(m), rng.randrange(m)) for _ in range(NRAND)]
    return [x for x, _ in rows], [y for _, y in rows]


def mont_expected_ok(op, x, y, g, flag, m, R, Ri):
    if op == "mul":
        return g == x * y * Ri % m
    if op == "sqr":
        return g == x * x * Ri % m
    if op == "add":
        return g == (x + y) % m
    if op == "sub":
        return g == (x - y) % m
    if op == "neg":
        return g == -x % m
    if op == "dbl":
        return g == 2 * x % m
    if op == "half":
        return g < m and 2 * g % m == x
    if op == "to_mont":
        return g == x * R % m
    if op == "from_mont":
        return g == x * Ri % m
    if op == "inv":                                   # Montgomery form of (x R^-1)^-1: g x = R^2
        return g < m and (g * x % m == R * R % m if x else g == 0)
    if op == "sqrt":                                  # g^2 R^-1 = x for a square, = -x for a non-square (p = 3 mod 4)
        sq = g * g * Ri % m
        return g < m and (sq == x if flag else (sq == -x % m and x != 0))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("op", D.MONT_OPS)
@pytest.mark.parametrize("curve", D.MONT_CURVES)
def test_mont_field_is_exact(curve, op, build):
    m, L = V.MONT_FIELDS[curve]
    R = 2**(32 * L)
    Ri = pow(R, -1, m)
    xs, ys = cached(("mont_in", curve), lambda: mont_inputs(curve))
    aw, bw = cached(("mont_w", curve), lambda: (V.to_words(xs, L), V.to_words(ys, L)))
    out = D.mont_op(D.device(build)["mont"], curve, op, aw, bw)
    if build != "default":
        ref = cached(("mont", curve, op), lambda: D.mont_op(D.device("default")["mont"], curve, op, aw, bw))
        bad = np.nonzero((out != ref).any(axis=1))[0]
        assert bad.size == 0, (curve, op, build, bad.size, hex(xs[bad[0]]), hex(ys[bad[0]]))
        return
    _CACHE[("mont", curve, op)] = out
    got = V.from_words(out[:, :L])
    flags = out[:, L]
    for x, y, g, fl in zip(xs, ys, got, flags):
        assert mont_expected_ok(op, x, y, g, fl, m, R, Ri), (curve, op, hex(x), hex(y), hex(g), int(fl))
    if op != "sqrt":
        assert not flags.any()
    else:                                                 # a non-residue gets no root, and there are non-residues here
        assert 0 < int(flags.sum()) < len(flags)


# ---- scalar fields ----------------------------------------------------------------------------------------------------------
def scalar_inputs(curve, op):
    n, L = V.SCALAR_FIELDS[curve]
    rows = V.edge_pairs(n, L)
    rng = random.Random(len(curve) * 31 + len(op))
    rows += [(rng.randrange(n), rng.randrange(n)) for _ in range(NRAND)]
    if op == "reduce_once":                               # domain [0, min(2n, 2^(32 L)))
        top = min(2 * n, 2**(32 * L))
        rows += [(n + x, 0) for x in V.edges(n, L) if n + x < top]
        rows += [(top - 1 - rng.getrandbits(rng.choice([8, 64, 200])), 0) for _ in range(NRAND)]
    return [x for x, _ in rows], [y for _, y in rows]


def scalar_expected(op, x, y, n, R, Ri):
    return {"mul": lambda: x * y * Ri, "add": lambda: x + y, "reduce_once": lambda: x, "to_mont": lambda: x * R,
            "from_mont": lambda: x * Ri}[op]() % n


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("op", D.SCALAR_OPS)
@pytest.mark.parametrize("curve", D.SCALAR_CURVES)
def test_scalar_field_is_exact(curve, op, build):
    n, L = V.SCALAR_FIELDS[curve]
    R = 2**(32 * L)
    Ri = pow(R, -1, n)
    xs, ys = cached(("scalar_in", curve, op), lambda: scalar_inputs(curve, op))
    aw, bw = cached(("scalar_w", curve, op), lambda: (V.to_words(xs, L), V.to_words(ys, L)))
    out = D.scalar_op(D.device(build)["scalar"], curve, op, aw, bw)
    if build != "default":
        ref = cached(("scalar", curve, op), lambda: D.scalar_op(D.device("default")["scalar"], curve, op, aw, bw))
        bad = np.nonzero((out != ref).any(axis=1))[0]
        assert bad.size == 0, (curve, op, build, bad.size, hex(xs[bad[0]]), hex(ys[bad[0]]))
        return
    _CACHE[("scalar", curve, op)] = out
    for x, y, g in zip(xs, ys, V.from_words(out)):
        if op == "inv":                                   # Montgomery form of (x R^-1)^-1: g x = R^2, and inv(0) = 0
            ok = g < n and (g * x % n == R * R % n if x else g == 0)
        else:
            ok = g < n and g == scalar_expected(op, x, y, n, R, Ri)
        assert ok, (curve, op, hex(x), hex(y), hex(g))


# ---- column forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_mac_cols_every_form_is_exact(build):
    fn = D.device(build)["mac"]
    for M, fresh, nc in V.mac_forms():
        c, pa, pb = V.mac_inputs(M, fresh, nc, NRAND)
        want, _ = V.mac_expected(c, pa, pb, M)
        got = D.mac_cols(fn, M, fresh, nc, c, pa, pb)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (build, M, fresh, nc, bad.size, c[bad[0]].tolist(), pa[bad[0], :M].tolist(), pb[bad[0], :M].tolist(),
                               got[bad[0]].tolist(), want[bad[0]].tolist())
