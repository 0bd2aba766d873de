"""BIP340 batch verification on the GPU (include/ecgpu.h "batch verification"): ecgpu_schnorr_batch_verify,
ecgpu_schnorr_batch_verify_prehash and ecgpu_schnorr_batch_verify_msg.  The specification is the per-signature verifier: ok is byte for
byte what ecgpu_schnorr_verify_prehash_batch writes.  Valid signatures come from schnorr_sign_prehash on the device (checked against
the oracle by test_gpu_signing.py); the terms and coefficients come from tests/schnorr_batch_model.py."""
import ctypes
import hashlib

import numpy as np
import pytest

import schnorr_batch_model as B

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4
N = B.N
POOL = 40960            # 2 * 40960 + 1 = 81 921 terms: the first size the MSM's bucket method takes by itself
SEEDS = [bytes(range(32)), hashlib.sha256(b"seed two").digest(), b"\xa5" * 32]
SHAPES = [1, 2, 63, 257, 1000]


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cv(ctx):
    return ctx.curve("k256")


def _keys(rng, n):
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d[:, 0] &= 0x7F          # below n
    d[:, 31] |= 1            # not zero
    return d


@pytest.fixture(scope="module")
def pool(cv):
    """POOL valid (key, signature, prehash) rows, signed on the device once; read-only"""
    rng = np.random.default_rng(0xB340)
    d, m, aux = _keys(rng, POOL), rng.integers(0, 256, (POOL, 32), dtype=np.uint8), rng.integers(0, 256, (POOL, 32), dtype=np.uint8)
    sig, px, ok = cv.schnorr_sign_prehash(d, m, aux)
    assert ok.all()
    for a in (px, sig, m):
        a.setflags(write=False)
    return px, sig, m


@pytest.fixture(params=[1, 0], ids=["small-path", "buckets"])
def msm_path(ctx, request):
    """the MSM under the equation: its small-sum path (one multiplication per term), or the bucket method with 16-bit windows"""
    import ecgpu
    before = ctx.get_option(ecgpu.OPT_MSM_SMALL_PATH)
    ctx.set_option(ecgpu.OPT_MSM_SMALL_PATH, request.param)
    yield request.param
    ctx.set_option(ecgpu.OPT_MSM_SMALL_PATH, before)


def _flip_s(sig, i, bit=3):
    out = np.array(sig)
    out[i, 63] ^= 1 << bit
    return out


def _add_to_s(sig, i, delta):
    s = (int.from_bytes(bytes(sig[i, 32:]), "big") + delta) % N
    assert s != 0
    sig[i, 32:] = np.frombuffer(s.to_bytes(32, "big"), dtype=np.uint8)


@pytest.mark.parametrize("n", SHAPES)
def test_valid_batches_and_one_bad_signature(cv, pool, msm_path, n):
    import ecgpu
    px, sig, m = (a[:n] for a in pool)
    always = ecgpu.BATCH_EQUATION_ALWAYS
    ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, seed=SEEDS[0], flags=always)
    assert ok.tolist() == [1] * n and all_valid is True
    # the equation itself held (a failed one leaves zeros with VERDICT_ONLY)
    ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, seed=SEEDS[1], flags=always | ecgpu.BATCH_VERDICT_ONLY)
    assert ok.tolist() == [1] * n and all_valid is True
    for i in sorted({0, n // 2, n - 1}):
        bad = _flip_s(sig, i)
        want = [1] * n
        want[i] = 0
        ok, all_valid = cv.schnorr_batch_verify_prehash(px, bad, m, seed=SEEDS[0], flags=always)
        assert ok.tolist() == want and all_valid is False, i
        ok, all_valid = cv.schnorr_batch_verify_prehash(px, bad, m, seed=SEEDS[0], flags=always | ecgpu.BATCH_VERDICT_ONLY)
        assert ok.tolist() == [0] * n and all_valid is False, i


def test_default_routes_at_40960(ctx, cv, pool):
    """81 921 terms: the MSM takes the bucket method by itself (every option at its default).  The call's own default routing
    (per-signature below 2^18 signatures) and the equation must give the same bytes."""
    import ecgpu
    assert ctx.get_option(ecgpu.OPT_MSM_SMALL_PATH) == 1
    px, sig, m = pool
    n = POOL
    bad = _flip_s(sig, n // 2)
    want = cv.schnorr_verify_prehash(px, bad, m)
    assert np.nonzero(want == 0)[0].tolist() == [n // 2]
    for flags in (ecgpu.BATCH_EQUATION_ALWAYS, 0):
        ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, flags=flags | ecgpu.BATCH_VERDICT_ONLY)
        assert int(ok.sum()) == n and all_valid is True
        ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, flags=flags)
        assert int(ok.sum()) == n and all_valid is True
        ok, all_valid = cv.schnorr_batch_verify_prehash(px, bad, m, flags=flags)
        assert bytes(ok) == bytes(want) and all_valid is False
    ok, all_valid = cv.schnorr_batch_verify_prehash(px, bad, m, flags=ecgpu.BATCH_EQUATION_ALWAYS | ecgpu.BATCH_VERDICT_ONLY)
    assert not ok.any() and all_valid is False


def _vectors(ref_vectors):
    vs = ref_vectors["k256"]["bip340"]["verify"]
    assert [v["index"] for v in vs] == list(range(4, 15))
    u8 = lambda k: np.array([list(bytes.fromhex(v[k])) for v in vs], dtype=np.uint8)
    return u8("public_key"), u8("signature"), u8("message"), [v["valid"] for v in vs]


def test_reference_vectors_mixed_into_valid_ones(cv, pool, msm_path, ref_vectors):
    """vectors 4-14 at scattered places among 53 valid signatures: ok is the per-signature verifier's, byte for byte"""
    import ecgpu
    vpx, vsig, vm, valid = _vectors(ref_vectors)
    n = 64
    px, sig, m = (np.array(a[:n]) for a in pool)
    at = [0, 5, 6, 17, 31, 32, 33, 40, 50, 62, 63]
    px[at], sig[at], m[at] = vpx, vsig, vm
    want = cv.schnorr_verify_prehash(px, sig, m)
    assert [int(want[i]) for i in at] == [int(v) for v in valid] and int(want.sum()) == n - 10
    ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, seed=SEEDS[2], flags=ecgpu.BATCH_EQUATION_ALWAYS)
    assert bytes(ok) == bytes(want) and all_valid is False
    # only undecodable elements among valid ones: the equation holds without them, no fallback - with VERDICT_ONLY ok is the decode flags
    dec = np.array([1 if B.decodes(bytes(px[i]), bytes(sig[i])) else 0 for i in range(n)], dtype=np.uint8)
    keep = np.nonzero((want == 1) | (dec == 0))[0]
    assert 0 < int((dec[keep] == 0).sum()) < len(at)
    ok, all_valid = cv.schnorr_batch_verify_prehash(px[keep], sig[keep], m[keep], seed=SEEDS[2], flags=ecgpu.BATCH_EQUATION_ALWAYS | ecgpu.BATCH_VERDICT_ONLY)
    assert bytes(ok) == bytes(dec[keep]) == bytes(want[keep]) and all_valid is False
    # all of them: the decodable invalid vectors fail the equation, VERDICT_ONLY leaves zeros
    ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, seed=SEEDS[2], flags=ecgpu.BATCH_EQUATION_ALWAYS | ecgpu.BATCH_VERDICT_ONLY)
    assert not ok.any() and all_valid is False


@pytest.mark.parametrize("seed", SEEDS, ids=["seed0", "seed1", "seed2"])
def test_cancelling_pair(cv, pool, msm_path, seed):
    """s1 + d, s2 - d satisfies the equation when every coefficient is 1; with the real coefficients it must fail"""
    import ecgpu
    n, i, j, delta = 63, 5, 40, 0x1234567
    px, sig, m = (np.array(a[:n]) for a in pool)
    _add_to_s(sig, i, delta)
    _add_to_s(sig, j, -delta)
    ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, seed=seed, flags=ecgpu.BATCH_EQUATION_ALWAYS | ecgpu.BATCH_VERDICT_ONLY)
    assert not ok.any() and all_valid is False
    ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, seed=seed, flags=ecgpu.BATCH_EQUATION_ALWAYS)
    assert np.nonzero(ok == 0)[0].tolist() == [i, j] and all_valid is False


def test_workspace_holds_the_model_terms(ctx, cv, pool):
    """after a VERDICT_ONLY call workspace 1 starts with the 2n + 1 scalars, then (256-byte aligned) the points: a_i, a_i e_i, R_i, P_i
    and the generator term of the model"""
    import ecgpu
    n, first = 63, 0
    px, sig, m = (a[:n] for a in pool)
    ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, seed=SEEDS[1], flags=ecgpu.BATCH_EQUATION_ALWAYS | ecgpu.BATCH_VERDICT_ONLY)
    assert ok.all() and all_valid
    ws = ctx.debug_workspace(1)
    cnt = 2 * n + 1
    pts_at = (32 * cnt + 255) // 256 * 256
    got = B.parse_terms(ws[:32 * cnt], ws[pts_at:pts_at + 64 * cnt])
    keys, sigs = [bytes(r) for r in px], [bytes(r) for r in sig]
    es = [B.challenge(k, bytes(mm), s) for k, mm, s in zip(keys, m, sigs)]
    dec, want = B.terms(keys, sigs, es, SEEDS[1], first)
    assert dec == [1] * n and got == want
    assert [k for k, _ in got[0:2 * n:2]] == [B.coefficient(SEEDS[1], i) for i in range(n)]
    assert len({k for k, _ in got}) == cnt


def test_repeated_signature_and_one_key(cv, pool, msm_path):
    import ecgpu
    n = 1000
    px, sig, m = pool
    rep = lambda a: np.ascontiguousarray(np.repeat(a[7:8], n, axis=0))
    ok, all_valid = cv.schnorr_batch_verify_prehash(rep(px), rep(sig), rep(m), seed=SEEDS[0], flags=ecgpu.BATCH_EQUATION_ALWAYS | ecgpu.BATCH_VERDICT_ONLY)
    assert ok.all() and all_valid is True
    rng = np.random.default_rng(0x1CE)
    d = np.ascontiguousarray(np.repeat(_keys(rng, 1), n, axis=0))
    mm, aux = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s1, p1, good = cv.schnorr_sign_prehash(d, mm, aux)
    assert good.all() and len({bytes(r) for r in p1}) == 1
    ok, all_valid = cv.schnorr_batch_verify_prehash(p1, s1, mm, seed=SEEDS[0], flags=ecgpu.BATCH_EQUATION_ALWAYS | ecgpu.BATCH_VERDICT_ONLY)
    assert ok.all() and all_valid is True


def test_seeds_do_not_change_the_answer(cv, pool):
    import ecgpu
    n = 257
    px, m = (a[:n] for a in (pool[0], pool[2]))
    sig = _flip_s(_flip_s(pool[1][:n], 100), 256, bit=0)
    want = cv.schnorr_verify_prehash(px, sig, m)
    assert np.nonzero(want == 0)[0].tolist() == [100, 256]
    for seed in (SEEDS[0], SEEDS[1], None):
        ok, all_valid = cv.schnorr_batch_verify_prehash(px, sig, m, seed=seed, flags=ecgpu.BATCH_EQUATION_ALWAYS)
        assert bytes(ok) == bytes(want) and all_valid is False
        ok, all_valid = cv.schnorr_batch_verify_prehash(px, pool[1][:n], m, seed=seed, flags=ecgpu.BATCH_EQUATION_ALWAYS | ecgpu.BATCH_VERDICT_ONLY)
        assert ok.all() and all_valid is True


def test_three_forms_agree_with_each_other_and_the_per_signature_calls(cv):
    import ecgpu
    from ecgpu import schnorr as S
    n = 257
    rng = np.random.default_rng(0xF0)
    d = _keys(rng, n)
    msgs = [bytes(rng.integers(0, 256, int(l), dtype=np.uint8)) for l in rng.integers(0, 120, n)]
    digests = np.array([list(hashlib.sha256(mm).digest()) for mm in msgs], dtype=np.uint8)
    sig, px, good = cv.schnorr_sign_msg(d, msgs)
    assert good.all()
    sig = _flip_s(sig, 200)
    sig[13, :32] = 0                                   # r = 0: does not decode
    e = np.frombuffer(S.challenges([bytes(r) for r in px], [bytes(r) for r in digests], [bytes(r) for r in sig]), dtype=np.uint8).reshape(n, 32)
    want = cv.schnorr_verify_prehash(px, sig, digests)
    assert np.nonzero(want == 0)[0].tolist() == [13, 200]
    assert bytes(cv.schnorr_verify(px, sig, e)) == bytes(want) == bytes(cv.schnorr_verify_msg(px, msgs, sig))
    for flags in (ecgpu.BATCH_EQUATION_ALWAYS, 0):     # 0: 515 terms route to the per-signature pipeline
        a = cv.schnorr_batch_verify(px, sig, e, seed=SEEDS[0], flags=flags)
        b = cv.schnorr_batch_verify_prehash(px, sig, digests, seed=SEEDS[0], flags=flags)
        c = cv.schnorr_batch_verify_msg(px, msgs, sig, seed=SEEDS[0], flags=flags)
        for ok, all_valid in (a, b, c):
            assert bytes(ok) == bytes(want) and all_valid is False
    ok, all_valid = S.batch_verify_device(cv, [bytes(r) for r in px[:12]], [bytes(r) for r in digests[:12]], [bytes(r) for r in sig[:12]])
    assert ok.all() and all_valid is True


def test_device_resident_batches_agree_with_host_ones(cv, pool):
    import ecgpu
    import torch
    n = 1000
    px, m = (a[:n] for a in (pool[0], pool[2]))
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    for sig in (pool[1][:n], _flip_s(pool[1][:n], 999)):
        host_ok, host_all = cv.schnorr_batch_verify_prehash(px, sig, m, seed=SEEDS[2], flags=ecgpu.BATCH_EQUATION_ALWAYS)
        d_ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        _, dev_all = cv.schnorr_batch_verify_prehash_device(dev(px), dev(sig), dev(m), d_ok, n, seed=SEEDS[2], flags=ecgpu.BATCH_EQUATION_ALWAYS)
        assert bytes(d_ok.cpu().numpy()) == bytes(host_ok) and dev_all == host_all
        # without ok: the verdict alone
        _, verdict = cv.schnorr_batch_verify_prehash_device(dev(px), dev(sig), dev(m), None, n, flags=ecgpu.BATCH_VERDICT_ONLY)
        assert verdict == host_all
        # default routing of a device batch this small: the per-signature pipeline, all_valid from ok
        d_ok.fill_(7)
        _, routed = cv.schnorr_batch_verify_prehash_device(dev(px), dev(sig), dev(m), d_ok, n)
        assert bytes(d_ok.cpu().numpy()) == bytes(host_ok) and routed == host_all


def test_argument_checks(ctx, cv, pool):
    import ecgpu
    px, sig, m = (np.array(a[:4]) for a in pool)
    ok, all_valid = cv.schnorr_batch_verify_prehash(px[:0], sig[:0], m[:0])
    assert len(ok) == 0 and all_valid is True
    with pytest.raises(ecgpu.EcgpuError, match="ecgpu error %d" % ERR_UNSUPPORTED):
        ctx.curve("p256").schnorr_batch_verify_prehash(px, sig, m)
    lib, p = ctx.lib, lambda a: ctypes.c_void_p(a.ctypes.data)
    verdict = ctypes.c_int(-1)
    for fn in (lib.ecgpu_schnorr_batch_verify, lib.ecgpu_schnorr_batch_verify_prehash):
        assert fn(ctx.handle, ecgpu.K256, p(px), p(sig), p(m), None, None, ctypes.byref(verdict), 4, ecgpu.HOST, 0) == ERR_ARG
        assert fn(ctx.handle, ecgpu.K256, p(px), p(sig), p(m), None, None, ctypes.byref(verdict), 4, ecgpu.HOST, ecgpu.BATCH_EQUATION_ALWAYS) == ERR_ARG
        assert fn(ctx.handle, ecgpu.K256, p(px), p(sig), None, None, p(np.zeros(4, np.uint8)), None, 4, ecgpu.HOST, 0) == ERR_ARG
        assert fn(ctx.handle, ecgpu.K256, p(px), p(sig), p(m), None, p(np.zeros(4, np.uint8)), None, 4, ecgpu.HOST, 64) == ERR_ARG
        assert fn(ctx.handle, ecgpu.P384, p(px), p(sig), p(m), None, None, None, 4, ecgpu.HOST, ecgpu.BATCH_VERDICT_ONLY) == ERR_UNSUPPORTED
        assert verdict.value == -1
        # NULL ok with VERDICT_ONLY, NULL all_valid with ok: both fine
        assert fn(ctx.handle, ecgpu.K256, p(px), p(sig), p(m), None, None, ctypes.byref(verdict), 0, ecgpu.HOST, ecgpu.BATCH_VERDICT_ONLY) == 0
        assert verdict.value == 1
        verdict.value = -1
    with pytest.raises(ValueError):
        cv.schnorr_batch_verify_prehash(px, sig, m, seed=b"short")
