"""Pins tests/keccak_model.py before anything uses it: its SHA-3 instances against hashlib on every length 0 .. 300 (both rates,
every block and padding boundary), Keccak-256 - the same sponge with the other domain byte - against known answers, and the three
vectors of tests/golden/keccak_ecdsa.json (the reference's Ethereum example, k256/src/ecdsa.rs:84-143 and :312-342) through
oracle.ecmodel and tests/rfc6979_model.py: the signature and recovery id, the recovered keys, and the address."""
import hashlib
import json
import os
import random

import keccak_model as K
import rfc6979_model as R
from conftest import GOLDEN
from oracle import ecmodel as M


def test_sha3_against_hashlib_on_every_length():
    rng = random.Random(0x5A3)
    for n in range(301):
        msg = rng.randbytes(n)
        assert K.digest(K.SHA3_256, msg) == hashlib.sha3_256(msg).digest(), n
        assert K.digest(K.SHA3_384, msg) == hashlib.sha3_384(msg).digest(), n


def test_keccak256_known_answers():
    assert K.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert K.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert K.digest(K.KECCAK256, b"abc") == K.keccak256(b"abc") != hashlib.sha3_256(b"abc").digest()


def test_round_constants_and_offsets():
    assert K.RC[0] == 1 and K.RC[1] == 0x8082 and K.RC[23] == 0x8000000080008008 and len(set(K.RC)) == 22
    assert K.RHO[:5] == [0, 1, 62, 28, 27] and sorted(K.RHO)[:3] == [0, 1, 2] and 32 not in K.RHO


def test_ethereum_vectors():
    with open(os.path.join(GOLDEN, "keccak_ecdsa.json")) as f:
        fx = json.load(f)
    c = M.K256
    # sign_digest_recoverable: RFC 6979 on HMAC-SHA-256 over the Keccak-256 digest, low s
    s = fx["sign"]
    d = int(s["secret_key"], 16)
    z = K.keccak256(bytes.fromhex(s["message"]))
    k = R.nonce(c, d, z)
    r, sv, recid = M.ecdsa_sign_prehashed(c, d, k, z, normalize_s=True)
    assert (r.to_bytes(32, "big") + sv.to_bytes(32, "big")).hex() == s["signature"] and recid == s["recovery_id"]
    pub = M.affine_mul(c, d, (c.gx, c.gy))
    assert M.ecdsa_recover_prehashed(c, z, r, sv, recid, reject_high_s=True) == pub
    assert M.ecdsa_verify_prehashed(c, pub, z, r, sv, reject_high_s=True)
    assert K.eth_address(M.i2b(c, pub[0]) + M.i2b(c, pub[1])).hex() == s["address"]
    # recover_from_digest
    v = fx["recover"]
    sig = bytes.fromhex(v["signature"])
    z = K.keccak256(v["message_text"].encode())
    q = M.ecdsa_recover_prehashed(c, z, int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big"), v["recovery_id"], reject_high_s=True)
    assert M.group_to_bytes(c, q).hex() == v["public_key_sec1"]
