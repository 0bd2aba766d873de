"""GPU side of tests/test_hosttwin_k256_tails.py: the tails of the k256 reductions as the kernels run them (tests/devtwin: the
throughput build, where the ripple behind the fold is a wave-level branch, and the branch-free build, which executes it on every
call), on the same vectors.  The inputs are arranged four ways, at most 4 096 elements per launch: every lane of every wave taking
the ripple (solved rows, half of them crossing 2^256 into the second fold), exactly one lane of each 64-lane wave taking it among
random operands, no lane taking it, and the edge rows (largest T, word 16, the chain carries).  Results are bit-exact against Python
integers, and the branch-free build's words equal the throughput build's.  Then one variable-base scalar multiplication of
4 096 + 37 units against the C oracle."""
import numpy as np
import pytest

import k256_tail_vectors as S
import devtwin_util as D

pytestmark = pytest.mark.gpu

P = S.P
N = 4096
_CACHE = {}


def arrangements(form):
    """{name: four (n, 8) operand arrays}, n <= 4096"""
    if form in _CACHE:
        return _CACHE[form]
    B = S.BIT
    vec = S.vector_set(form)
    mask = S.masks(form, vec)
    hot = [x[(mask & B["fold:ripple"]) != 0] for x in vec]                 # every row ripples; the solved second-fold rows among them
    assert hot[0].shape[0] >= 24 and ((mask & B["fold:second"]) != 0).sum() >= 12
    g = np.random.default_rng(11 + S.FORMS.index(form))
    rnd = [g.integers(0, 2**32, (N, 8), dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    assert not (S.masks(form, rnd) & B["fold:ripple"]).any()
    rep = np.arange(N) % hot[0].shape[0]
    all_lanes = [h[rep] for h in hot]
    one_lane = [r.copy() for r in rnd]
    lanes = (np.arange(N // 64) * 64 + (np.arange(N // 64) * 37 + 5) % 64)      # one lane per wave, a different one each
    for k in range(4):
        one_lane[k][lanes] = hot[k][np.arange(N // 64) % hot[0].shape[0]]
    m1 = (S.masks(form, one_lane) & B["fold:ripple"]).reshape(-1, 64)
    assert ((m1 != 0).sum(axis=1) == 1).all()
    edges = [x[:N] for x in vec]
    _CACHE[form] = {"all_lanes": all_lanes, "one_lane": one_lane, "none": rnd, "edges": edges}
    return _CACHE[form]


def expect(form, ops):
    ints = [S.V.from_words(x) for x in ops]
    return [S.EXPECT[form](a, b, e, f) % P for a, b, e, f in zip(*ints)]


@pytest.mark.parametrize("form", S.FORMS)
def test_tails_exact_in_every_arrangement(form):
    dflt, bf = D.device("default")["k256"], D.device("bf")["k256"]
    for name, ops in arrangements(form).items():
        assert ops[0].shape[0] <= N
        out = D.k256_op(dflt, form, *ops)
        got = S.V.from_words(out[:, :8])
        want = expect(form, ops)
        bad = [i for i in range(len(got)) if got[i] % P != want[i]]
        print(form, name, len(got), "elements, mismatches", len(bad))
        assert not bad, (form, name, bad[:8])
        out_bf = D.k256_op(bf, form, *ops)
        assert np.array_equal(out_bf[:, :8], out[:, :8]), (form, name)


def test_scalar_mul_against_oracle():
    import ecgpu
    from oracle import ecmodel as M
    from oracle import synth
    from oracle import coracle as CO
    C = M.K256
    n = 4096 + 37
    sb = CO.synth_scalars(0, n, synth.SEED, 7711)               # curve id 0: k256
    pb = CO.synth_points(0, n, synth.SEED, 7711)
    ks = [C.n - 1, C.n - 2, 2**255, 2**256 - 2**128 - 1, 1, 2, 3, 2**32 - 1]
    for i, k in enumerate(ks):
        sb[i] = np.frombuffer(M.i2b(C, k % C.n or 1), dtype=np.uint8)
    ctx = ecgpu.Context(0)
    try:
        xy, inf = ctx.curve("k256").mul(sb, pb)
    finally:
        ctx.close()
    want = CO.lincomb_batch(0, sb, pb, threads=8)
    assert bytes(np.ascontiguousarray(want[:, :64])) == bytes(xy)
    assert np.array_equal(want[:, 64], np.asarray(inf).astype(np.uint8))
