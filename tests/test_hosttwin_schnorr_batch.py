"""BIP340 batch verification on the host twin (csrc/schnorr_batch_kernels.hpp compiled for the host by
tests/hosttwin/hosttwin_schnorr_batch.cpp): the coefficients against hashlib, the emitted terms against the model and - as a sum of
k_j Q_j in the oracle's arithmetic - against the identity, the wide modular sum at its carry extreme, and the decode flags of the
reference's verify vectors."""
import ctypes
import random

import schnorr_batch_model as B
from hosttwin_util import buf, lib, outbuf
from oracle import ecmodel as M

N = B.N
SEED = bytes(range(100, 132))


def _signatures(count, rng):
    keys, sigs, msgs = [], [], []
    for _ in range(count):
        d, m, aux = rng.randrange(1, N).to_bytes(32, "big"), rng.randbytes(32), rng.randbytes(32)
        sig, px = M.schnorr_sign_prehash(d, m, aux)
        assert M.schnorr_verify_prehash(px, m, sig)
        keys.append(px); sigs.append(sig); msgs.append(m)
    return keys, sigs, msgs


def _twin_terms(keys, sigs, es, seed, first_index=0, lanes=256):
    n = len(keys)
    sc, pts, dec = outbuf(32 * (2 * n + 1)), outbuf(64 * (2 * n + 1)), outbuf(n)
    bad = lib().ht_sb_terms(buf(b"".join(keys)), buf(b"".join(sigs)), buf(b"".join(es)), buf(seed), ctypes.c_uint64(first_index), ctypes.c_size_t(n), lanes,
                            sc, pts, dec)
    return bad, list(bytes(dec)), B.parse_terms(bytes(sc), bytes(pts))


def test_coefficients_equal_the_model():
    out = outbuf(16)
    for seed in (SEED, bytes(32), b"\xff" * 32):
        for index in (0, 1, (1 << 32) - 1, (1 << 32) + 5):
            assert lib().ht_sb_coefficient(buf(seed), ctypes.c_uint64(index), out) == 0
            assert int.from_bytes(bytes(out), "big") == B.coefficient(seed, index), (seed.hex(), index)
    assert len({B.coefficient(SEED, i) for i in range(64)}) == 64


def test_terms_of_valid_signatures_sum_to_the_identity():
    keys, sigs, msgs = _signatures(8, random.Random(0xba7c4))
    es = [B.challenge(px, m, s) for px, m, s in zip(keys, msgs, sigs)]
    for first in (0, (1 << 32) - 3):
        bad, dec, terms = _twin_terms(keys, sigs, es, SEED, first)
        assert bad == 0 and dec == [1] * 8
        assert (dec, terms) == B.terms(keys, sigs, es, SEED, first)
        assert all(M.on_curve(M.K256, q) and q[1] % 2 == 0 for _, q in terms[:-1])
        assert B.combination(terms) is None
    # one s altered: the same terms but the generator's scalar, and the sum is no longer the identity
    s5 = (int.from_bytes(sigs[5][32:], "big") ^ 4)
    assert 0 < s5 < N
    broken = list(sigs)
    broken[5] = sigs[5][:32] + s5.to_bytes(32, "big")
    bad, dec, terms2 = _twin_terms(keys, broken, es, SEED)
    assert bad == 0 and dec == [1] * 8
    assert terms2[:-1] == B.terms(keys, sigs, es, SEED)[1][:-1] and terms2 == B.terms(keys, broken, es, SEED)[1]
    assert B.combination(terms2) is not None


def test_sum_at_the_carry_extreme():
    """m scalars n - 1, and m scalars 2^256 - 1 (every limb full: the widest carries an accumulator sees), on one and two workgroups"""
    out = outbuf(32)
    for m in (1, 2, 255, 256, 257):
        for v in (N - 1, (1 << 256) - 1):
            for lanes in (256, 512):
                assert lib().ht_sb_sum(buf(v.to_bytes(32, "big") * m), ctypes.c_size_t(m), lanes, out) == 0
                assert int.from_bytes(bytes(out), "big") == (-(m * v)) % N, (m, hex(v), lanes)
    rng = random.Random(0x5a3)
    vals = [rng.randrange(N) for _ in range(777)]
    assert lib().ht_sb_sum(buf(b"".join(v.to_bytes(32, "big") for v in vals)), ctypes.c_size_t(len(vals)), 512, out) == 0
    assert int.from_bytes(bytes(out), "big") == (-sum(vals)) % N


def test_decode_flags_of_the_reference_vectors(ref_vectors):
    """verify vectors 4-14: dec is what the model predicts; an element with dec = 0 is invalid for the reference too, and is left out
    as two zero scalars on G"""
    vs = ref_vectors["k256"]["bip340"]["verify"]
    assert [v["index"] for v in vs] == list(range(4, 15))
    keys = [bytes.fromhex(v["public_key"]) for v in vs]
    sigs = [bytes.fromhex(v["signature"]) for v in vs]
    msgs = [bytes.fromhex(v["message"]) for v in vs]
    es = [B.challenge(px, m, s) for px, m, s in zip(keys, msgs, sigs)]
    bad, dec, terms = _twin_terms(keys, sigs, es, SEED)
    want = [1 if B.decodes(px, s) else 0 for px, s in zip(keys, sigs)]
    assert dec == want and bad == want.count(0) and 0 < bad < len(vs)
    assert (dec, terms) == B.terms(keys, sigs, es, SEED)
    for i, v in enumerate(vs):
        assert M.schnorr_verify_prehash(keys[i], msgs[i], sigs[i]) == v["valid"]
        if not dec[i]:
            assert not v["valid"] and terms[2 * i] == (0, B.G) and terms[2 * i + 1] == (0, B.G)
    # the decodable invalid ones break the equation; the valid one with the undecodable ones alone does not
    assert B.combination(terms) is not None
    keep = [i for i, v in enumerate(vs) if v["valid"] or not dec[i]]
    sub = _twin_terms([keys[i] for i in keep], [sigs[i] for i in keep], [es[i] for i in keep], SEED)
    assert sub[0] == len(keep) - 1 and B.combination(sub[2]) is None
