"""The speculative products of the k256 field products (csrc/fe_k256.hpp, csrc/mp32.hpp mac_cols with SPEC) on the host twin
(tests/hosttwin/hosttwin_spec_carry.cpp), whose ECGPU_SPEC_NOTE hook reports per site whether the carry flag was raised.

A column's speculative product is issued without its carry addition; a rare branch adds the carry when the flag is raised.  For mul,
sqr, mul_add2 and mul_add_sqr on raw 256-bit operands (values >= p included):
- (a) all ones and the column-maximising pairs / quads of field_edge_vectors;
- (b) for every speculative site of mul an input that raises that site and no other (exactly one flag);
- (c) for the other forms the same where the seeded search (k256_spec_carry_vectors.isolating, 4 x 10^5 trials, the bound is 10^6)
  finds one: at most a quarter of a form's sites may be left without, and every site is raised by some input of the set;
- (d) 10^5 uniform random operands raise no flag.
Every flag equals the model's (k256_spec_carry_vectors.raised), every result is below 2^256, congruent to the Python integers mod p
and word for word the exact columns' result."""
import ctypes

import numpy as np
import pytest

import k256_spec_carry_vectors as S
from hosttwin_util import lib

P = S.P
_PTR = ctypes.POINTER(ctypes.c_uint32)


def _p(a):
    return a.ctypes.data_as(_PTR)


def run(form, ops):
    a, b, e, f = (np.ascontiguousarray(x, dtype=np.uint32) for x in ops)
    n = a.shape[0]
    out = np.zeros((n, 8), dtype=np.uint32)
    exact = np.zeros((n, 8), dtype=np.uint32)
    masks = np.zeros(n, dtype=np.uint32)
    seen = np.zeros(1, dtype=np.uint32)
    L = lib()
    op = S.FORMS.index(form)
    assert L.ht_k256_spec_carry_op(op, _p(a), _p(b), _p(e), _p(f), _p(out), _p(masks), _p(seen), n) == 0
    assert L.ht_k256_exact_op(op, _p(a), _p(b), _p(e), _p(f), _p(exact), n) == 0
    assert int(seen[0]) == sum(1 << K for K in S.SITES[form]), (form, hex(int(seen[0])))
    return out, exact, masks


def check_values(form, ops, out, exact):
    assert np.array_equal(out, exact), form
    ints = [S.from_words(x) for x in ops]
    for i, g in enumerate(S.from_words(out)):
        want = S.EXPECT[form](ints[0][i], ints[1][i], ints[2][i], ints[3][i])
        assert g % P == want % P, (form, i)


@pytest.mark.parametrize("form", S.FORMS)
def test_edges_and_isolating_inputs(form):
    ops = S.vector_set(form)
    out, exact, masks = run(form, ops)
    check_values(form, ops, out, exact)
    assert np.array_equal(masks, S.flag_mask(form, *ops)), form
    assert masks[0] != 0, "all ones raises a site of every form"
    iso, anyhit = S.isolating(form)
    print(form, "isolated sites", sorted(iso), "raised only with others", sorted(set(anyhit) - set(iso)))
    for K in S.SITES[form]:
        row = iso.get(K) or anyhit.get(K)
        print("  column", K, [hex(v) for v in (S.from_words(x[None, :])[0] for x in row)] if row else None)
    # every site is raised by some input of the set
    hit = 0
    for m in masks:
        hit |= int(m)
    assert hit == sum(1 << K for K in S.SITES[form]), (form, hex(hit))
    missing = [K for K in S.SITES[form] if K not in iso]
    if form == "mul":
        assert not missing, missing
    else:
        assert 4 * len(missing) <= len(S.SITES[form]), (form, missing)
    # an isolating input raises exactly its own flag, on the twin as in the model
    for K, row in iso.items():
        _, _, m = run(form, [x[None, :] for x in row])
        assert int(m[0]) == 1 << K, (form, K, hex(int(m[0])))


@pytest.mark.parametrize("form", S.FORMS)
def test_uniform_operands_raise_nothing(form):
    g = np.random.default_rng(77 + S.FORMS.index(form))
    ops = [g.integers(0, 2**32, (100_000, 8), dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    out, exact, masks = run(form, ops)
    assert not masks.any(), form
    assert np.array_equal(out, exact)
    sub = [x[:2000] for x in ops]
    check_values(form, sub, out[:2000], exact[:2000])
