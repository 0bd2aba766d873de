"""The hash layer of hash to curve on the host twin (csrc/sha2.hpp, csrc/h2c_hash.hpp compiled for the host by
tests/hosttwin/hosttwin_h2c_hash.cpp): SHA-256 / SHA-384 against hashlib, expand_message_xmd against the oracle, FromOkm for
FieldElement against Python integers, the RFC 9380 vectors msg -> u_0, u_1 and the BIP340 challenges of the fixtures.
Everything is byte-exact."""
import ctypes
import hashlib
import random

import pytest

from hosttwin_util import buf, lib, outbuf
from oracle import ecmodel as M

HASHES = {0: "sha256", 1: "sha384"}
CURVES = [("k256", 0), ("p256", 1), ("p384", 2)]


def _sha2(h, msg):
    out = outbuf(hashlib.new(HASHES[h]).digest_size)
    assert lib().ht_sha2(h, buf(msg), ctypes.c_size_t(len(msg)), out) == 0
    return bytes(out)


def _xmd(h, msg, dst, length):
    out = outbuf(length)
    rc = lib().ht_expand_xmd(h, buf(msg), ctypes.c_size_t(len(msg)), buf(dst), ctypes.c_size_t(len(dst)), out, ctypes.c_size_t(length))
    assert rc == 0
    return bytes(out)


@pytest.mark.parametrize("h", [0, 1])
def test_sha2_every_length_to_300(h):
    """lengths 0 .. 300: each padding case (the 0x80 and the length field in one block / in two, a full block) twice per hash"""
    rng = random.Random(0x5a2 + h)
    block = hashlib.new(HASHES[h]).block_size
    lenfield = block // 8
    for n in range(301):
        msg = rng.randbytes(n)
        assert _sha2(h, msg) == hashlib.new(HASHES[h], msg).digest(), n
        if n % block in (block - lenfield - 1, block - lenfield, block - 1, 0):
            for fill in (b"\x00", b"\xff"):
                assert _sha2(h, fill * n) == hashlib.new(HASHES[h], fill * n).digest(), (n, fill)


@pytest.mark.parametrize("h", [0, 1])
def test_sha2_incremental_updates(h):
    """two updates cut at every position of a 300-byte message: the block buffer across word and block boundaries"""
    msg = random.Random(77).randbytes(300)
    want = hashlib.new(HASHES[h], msg).digest()
    out = outbuf(len(want))
    for cut in range(301):
        assert lib().ht_sha2_split(h, buf(msg), ctypes.c_size_t(len(msg)), cut, out) == 0
        assert bytes(out) == want, cut


@pytest.mark.parametrize("h,lengths", [(0, (1, 32, 48, 96, 144, 255 * 32)), (1, (72, 144, 255 * 48))])
def test_expand_message_xmd(h, lengths):
    rng = random.Random(0xd57 + h)
    dsts = [rng.randbytes(n) for n in (1, 49, 55, 255)]
    msgs = [rng.randbytes(n) for n in range(201)]
    for dst in dsts:
        for length in lengths:
            for msg in msgs:
                assert _xmd(h, msg, dst, length) == M.expand_message_xmd(HASHES[h], msg, dst, length), (len(msg), len(dst), length)


def test_expand_message_xmd_refuses_bad_lengths():
    out = outbuf(32)
    one = buf(b"x")
    assert lib().ht_expand_xmd(0, one, ctypes.c_size_t(1), one, ctypes.c_size_t(0), out, ctypes.c_size_t(32)) != 0
    assert lib().ht_expand_xmd(0, one, ctypes.c_size_t(1), buf(bytes(256)), ctypes.c_size_t(256), out, ctypes.c_size_t(32)) != 0
    assert lib().ht_expand_xmd(0, one, ctypes.c_size_t(1), one, ctypes.c_size_t(1), out, ctypes.c_size_t(255 * 32 + 1)) != 0
    assert lib().ht_expand_xmd(7, one, ctypes.c_size_t(1), one, ctypes.c_size_t(1), out, ctypes.c_size_t(32)) != 0


def okm_edge_values(c, L):
    """the inputs of FromOkm worth a look: around 0, p, the top of the range, both halves of the reference's split, and the
    largest multiple of p below 2^(8 L)"""
    p, nb = c.p, c.nbytes
    top = 1 << (8 * L)
    half = 8 * L // 2
    k = (top - 1) // p
    sh = p << (8 * (L - nb))
    v = [0, 1, p - 1, p, p + 1, top - 1, sh - 1, sh, sh + 1, ((1 << half) - 1) << half, (1 << half) - 1, k * p - 1, k * p, k * p + 1]
    assert all(0 <= x < top for x in v) and k * p < top <= (k + 1) * p
    return v


def _from_okm(cid, L, nb, values):
    data = b"".join(v.to_bytes(L, "big") for v in values)
    out = outbuf(nb * len(values))
    assert lib().ht_field_from_okm(cid, buf(data), out, len(values)) == 0
    return [int.from_bytes(bytes(out)[nb * i:nb * (i + 1)], "big") for i in range(len(values))]


@pytest.mark.parametrize("cn,cid", CURVES)
def test_field_from_okm(cn, cid):
    c = M.CURVES[cn]
    L = 72 if cn == "p384" else 48
    rng = random.Random(0xf0 + cid)
    values = okm_edge_values(c, L) + [rng.getrandbits(8 * L) for _ in range(1000)]
    got = _from_okm(cid, L, c.nbytes, values)
    for v, g in zip(values, got):
        assert g == v % c.p, hex(v)


@pytest.mark.parametrize("cn,cid", CURVES)
def test_rfc9380_hash_to_field_vectors(cn, cid, ref_vectors):
    c = M.CURVES[cn]
    L = 72 if cn == "p384" else 48
    h = 1 if cn == "p384" else 0
    vs = ref_vectors[cn]["hash2curve"]
    assert len(vs) == 5
    for v in vs:
        msg, dst = v["msg"].encode(), v["dst"].encode()
        okm = _xmd(h, msg, dst, 2 * L)
        u = _from_okm(cid, L, c.nbytes, [int.from_bytes(okm[:L], "big"), int.from_bytes(okm[L:], "big")])
        assert ["%0*x" % (2 * c.nbytes, x) for x in u] == [v["u_0"], v["u_1"]]
        # the fused form the device kernel runs (the okm never leaves the registers)
        out = outbuf(2 * c.nbytes)
        assert lib().ht_hash_to_field(cid, buf(msg), ctypes.c_size_t(len(msg)), buf(dst), ctypes.c_size_t(len(dst)), 2, out) == 0
        assert bytes(out).hex() == v["u_0"] + v["u_1"]
        assert lib().ht_hash_to_field(cid, buf(msg), ctypes.c_size_t(len(msg)), buf(dst), ctypes.c_size_t(len(dst)), 1, out) == 0
        assert int.from_bytes(bytes(out)[:c.nbytes], "big") == M.hash_to_field(c, msg, dst, 1)[0]


def test_bip340_challenges(ref_vectors):
    from ecgpu.schnorr import tagged_hash
    v = ref_vectors["k256"]["bip340"]
    cases = [(bytes.fromhex(x["public_key"]), bytes.fromhex(x["message"]), bytes.fromhex(x["signature"])) for x in v["sign"] + v["verify"]]
    cases = [x for x in cases if len(x[0]) == 32 and len(x[1]) == 32 and len(x[2]) == 64]
    assert len(cases) >= 5
    out = outbuf(32)
    for px, m, sig in cases:
        assert lib().ht_schnorr_challenge(buf(sig[:32]), buf(px), buf(m), out) == 0
        assert bytes(out) == tagged_hash(b"BIP0340/challenge", sig[:32], px, m)
