"""The edge vectors of tests/field_edge_vectors.py do what they are for: enough inputs take every rare carry path of the k256
field, the Montgomery quotient digits come out 0 and 2^32 - 1 and P-384's signed accumulator goes negative in the product and
in the separate squaring, the column-form inputs carry out of c.lo and wrap c.hi and keep the NC bound of the call sites.  A
change to the vectors that silently stops covering a path fails here, on the CPU."""
import numpy as np
import pytest

import field_edge_vectors as V

MIN_HITS = 8


@pytest.mark.parametrize("path", sorted(V.k256_rare_predicates()))
def test_k256_rare_path_is_taken(path):
    pred, arity = V.k256_rare_predicates()[path]
    hits = sum(bool(pred(*t[:arity])) for t in V.k256_rare_inputs()[path])
    assert hits >= MIN_HITS, (path, hits)


def test_k256_rare_inputs_are_in_range():
    for path, ts in V.k256_rare_inputs().items():
        for t in ts:
            assert all(0 <= x < 2**256 for x in t), path


def test_k256_shl_edges_take_the_second_wrap():
    """2^256 - 1 and 2^256 - 2 take the rare block of every shift and wrap past 2^256 a second time"""
    edges = [a for (a,) in V.k256_rare_inputs()["shl_edges"]]
    for K in (1, 2, 3):
        for a in (V.TOP, V.TOP - 1):
            assert a in edges and V.shl_rare(a, K) and V.shl_second_wrap(a, K), (K, hex(a))


@pytest.mark.parametrize("curve", sorted(V.MONT_FIELDS))
def test_mont_model_is_the_montgomery_product(curve):
    """the column model behind the predicates below computes (a b + q p) / R with a b + q p = 0 mod R"""
    m, L = V.MONT_FIELDS[curve]
    R = 2**(32 * L)
    for a, b in V.quotient_digit_pairs(m, L)[:64] + V.edge_pairs(m, L)[:64]:
        q, res, _ = V.mont_trace(V.product_columns(a, b, L), m, L)
        Q = sum(x << (32 * i) for i, x in enumerate(q))
        assert (a * b + Q * m) % R == 0 and res == (a * b + Q * m) // R and res < 2 * m


@pytest.mark.parametrize("curve", sorted(V.MONT_FIELDS))
def test_mont_quotient_digits_reach_the_extremes(curve):
    m, L = V.MONT_FIELDS[curve]
    ps = V.quotient_digit_pairs(m, L)
    assert all(a < m and b < m for a, b in ps)
    first = [V.mont_first_digit(a, b, m, L) for a, b in ps]
    assert sum(d == V.MASK32 for d in first) >= MIN_HITS
    assert sum(d == 0 and a != 0 and b != 0 for d, (a, b) in zip(first, ps)) >= MIN_HITS
    all_ones = sum(V.mont_trace(V.product_columns(a, b, L), m, L)[0] == [V.MASK32] * L for a, b in ps)
    assert all_ones >= MIN_HITS
    sq = V.quotient_digit_squares(m, L)
    assert all(a < m for a in sq) and len(sq) >= MIN_HITS
    assert sum(V.mont_trace(V.square_words(a, L), m, L)[0][0] == V.MASK32 - 6 for a in sq) >= MIN_HITS


def test_p384_signed_accumulator_goes_negative():
    m, L = V.MONT_FIELDS["p384"]
    ps = V.quotient_digit_pairs(m, L)
    assert sum(V.mont_mul_min_acc(a, b, m, L) < 0 for a, b in ps) >= MIN_HITS
    assert sum(V.mont_sqr_min_acc(a, m, L) < 0 for a in V.quotient_digit_squares(m, L)) >= MIN_HITS


@pytest.mark.parametrize("curve", sorted(V.MONT_FIELDS) + ["n_" + c for c in sorted(V.SCALAR_FIELDS)])
def test_edges_are_below_the_modulus(curve):
    m, L = V.SCALAR_FIELDS[curve[2:]] if curve.startswith("n_") else V.MONT_FIELDS[curve]
    e = V.edges(m, L)
    assert all(0 <= x < m for x in e) and {0, 1, 2, m - 1, m - 2} <= set(e)
    words = V.word_extreme_values(m, L, 32, __import__("random").Random(1))
    assert all(((x >> (32 * k)) & V.MASK32) in V.WORD_EXTREMES for x in words for k in range(L))
    near = [a * b for a, b in V.edge_pairs(m, L)]
    assert sum((m - 1)**2 - p < (m - 1)**2 >> 100 for p in near) >= MIN_HITS


@pytest.mark.parametrize("form", V.mac_forms(), ids=lambda f: "M%d_f%d_nc%d" % f)
def test_mac_inputs_keep_the_preconditions_and_carry(form):
    M, fresh, nc = form
    c, pa, pb = V.mac_inputs(M, fresh, nc, 4096)
    if fresh:
        assert not c[:, 2].any()
    assert V.mac_nc_bound_holds(c, pa, pb, nc)
    want, carried = V.mac_expected(c, pa, pb, M)
    # the vectorised reference against Python integers on a sample
    for i in range(0, 4096, 97):
        s = int(c[i, 0]) + (int(c[i, 1]) << 32) + (int(c[i, 2]) << 64) + sum(int(pa[i, k]) * int(pb[i, k]) for k in range(M))
        assert V.from_words(want[i:i + 1])[0] == s % 2**96
    if M > nc:                      # a product that may carry exists: the inputs make it carry, and wrap c.hi
        assert int(carried.sum()) >= MIN_HITS
        if not fresh:
            wrapped = sum((int(c[i, 2]) + ((int(c[i, 0]) + (int(c[i, 1]) << 32) + sum(int(pa[i, k]) * int(pb[i, k]) for k in range(M))) >> 64)) >> 32
                          for i in range(4096))
            assert wrapped >= MIN_HITS
    assert int((pa[:, :M] == V.MASK32).all(axis=1).sum()) >= 4
