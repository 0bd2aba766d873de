"""The tail of the k256 reductions (csrc/fe_k256.hpp: the overflow count T on the carry chains, add_high_chain, and the fold of
T C, fold_top_words) on the host twin (tests/hosttwin/hosttwin_k256_tails.cpp), whose ECGPU_TAIL_NOTE hook reports per input which
paths the tail took.

For mul, sqr, mul_add2 and mul_add_sqr, through the speculative and through the exact columns, on raw 256-bit operands:
- T at its largest (all-ones operands), and for the two-product forms word 16 set (h8 = 1) and clear;
- both chain carries set, exactly one, and neither;
- the carry of the fold's first multiply set and clear;
- solved rows whose fold carries out of word 2 (the rare ripple), and solved rows whose ripple crosses 2^256 (the second fold).
Every hook mask equals the model's (k256_tail_vectors.tail), every path is entered at least once, and every result is below 2^256
and congruent to the Python integers mod p."""
import ctypes

import numpy as np
import pytest

import k256_tail_vectors as S
from hosttwin_util import lib

P = S.P
_PTR = ctypes.POINTER(ctypes.c_uint32)


def _p(a):
    return a.ctypes.data_as(_PTR)


def run(form, ops, exact):
    a, b, e, f = (np.ascontiguousarray(x, dtype=np.uint32) for x in ops)
    n = a.shape[0]
    out = np.zeros((n, 8), dtype=np.uint32)
    masks = np.zeros(n, dtype=np.uint32)
    assert lib().ht_k256_tail_op(S.FORMS.index(form), int(exact), _p(a), _p(b), _p(e), _p(f), _p(out), _p(masks), n) == 0
    return out, masks


def count(masks, want, dont=0):
    return int((((masks & want) == want) & ((masks & dont) == 0)).sum())


@pytest.mark.parametrize("exact", [False, True], ids=["spec", "exact"])
@pytest.mark.parametrize("form", S.FORMS)
def test_tail_paths_and_values(form, exact):
    ops = S.vector_set(form)
    out, masks = run(form, ops, exact)
    ints = [S.V.from_words(x) for x in ops]
    for i, g in enumerate(S.V.from_words(out)):
        assert g % P == S.EXPECT[form](ints[0][i], ints[1][i], ints[2][i], ints[3][i]) % P, (form, i)
    model = S.masks(form, ops)
    assert np.array_equal(masks, model), (form, np.nonzero(masks != model)[0][:8])
    B = S.BIT
    n_rip, n_sec = 12, 12
    # the solved rows take the path they were solved for
    rip = masks[-(n_rip + n_sec):-n_sec]
    sec = masks[-n_sec:]
    assert ((rip & B["fold:ripple"]) != 0).all() and ((rip & B["fold:second"]) == 0).all(), form
    assert ((sec & B["fold:second"]) != 0).all() and ((sec & B["fold:ripple"]) != 0).all(), form
    # row 0 is all ones: the largest T of the form, with word 16 set in the two-product forms
    T0 = S.tail(form, *[x[0] for x in ints])[0]
    assert T0 == S.t_max(form) and T0 == max(S.tail(form, *row)[0] for row in zip(*[x[:64] for x in ints]))
    first = "sqr:c1" if form == "sqr" else "chain:t0"
    second = "chain:word7"
    paths = {
        "both chain carries": count(masks, B[first] | B[second]),
        "first chain carry only": count(masks, B[first], B[second]),
        "second chain carry only": count(masks, B[second], B[first]),
        "no chain carry": count(masks, 0, B[first] | B[second]),
        "fold multiply carries": count(masks, B["fold:k1"]),
        "fold multiply does not carry": count(masks, 0, B["fold:k1"]),
        "ripple": count(masks, B["fold:ripple"], B["fold:second"]),
        "second fold": count(masks, B["fold:second"]),
        "no ripple": count(masks, 0, B["fold:ripple"]),
    }
    if form in ("mul_add2", "mul_add_sqr"):
        assert masks[0] & B["mul:h8"]
        paths["word 16 set"] = count(masks, B["mul:h8"])
        paths["word 16 clear"] = count(masks, 0, B["mul:h8"])
    else:
        assert not (masks & B["mul:h8"]).any()
    if form == "sqr":
        paths["carry into t1"] = count(masks, B["chain:t0"])
    print(form, "exact" if exact else "spec", "T max", hex(T0), paths)
    missing = [k for k, v in paths.items() if v == 0]
    assert not missing, (form, missing)
