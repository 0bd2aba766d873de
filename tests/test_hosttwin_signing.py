"""Deterministic signing on the host twin (csrc/sha2.hpp word placement, csrc/hmac_drbg.hpp, csrc/signing_kernels.hpp compiled for the
host by tests/hosttwin/hosttwin_signing.cpp): the RFC 6979 model against the reference's six signatures, HMAC against hmac, the
generator against the model on the real orders and on an order that rejects often, the BIP340 tag midstates and the nonce, accept
and finish steps.  Everything is byte-exact."""
import ctypes
import hashlib
import hmac
import json
import os
import random

import pytest

import rfc6979_model as R
from hosttwin_util import buf, lib, outbuf
from oracle import ecmodel as M

HERE = os.path.dirname(os.path.abspath(__file__))
HASHES = {0: "sha256", 1: "sha384"}
CURVES = [("k256", 0), ("p256", 1), ("p384", 2)]
N = M.K256.n


def test_model_reproduces_the_reference_signatures():
    """pins tests/rfc6979_model.py before anything else uses it: nonce from the model, signature from the oracle's sign_prehashed"""
    with open(os.path.join(HERE, "golden", "rfc6979_sign.json")) as f:
        fixture = json.load(f)
    count = 0
    for cn, entry in fixture.items():
        c, d = M.CURVES[cn], int(entry["secret_key"], 16)
        for v in entry["vectors"]:
            z = M.bits2field(c, hashlib.new(v["hash"], bytes.fromhex(v["message"])).digest())
            r, s, _ = M.ecdsa_sign_prehashed(c, d, R.nonce(c, d, z), z)
            assert (M.i2b(c, r) + M.i2b(c, s)).hex() == v["signature"], (cn, v["test"])
            count += 1
    assert count == 6


@pytest.mark.parametrize("h", [0, 1])
def test_hmac_every_length_to_300(h):
    """lengths 0 .. 300 through the word placement: every alignment of a word in its two slots, padding in the last block and in
    one of its own"""
    rng = random.Random(0x4d0 + h)
    dlen = hashlib.new(HASHES[h]).digest_size
    out = outbuf(dlen)
    for n in range(301):
        for key, msg in ((rng.randbytes(dlen), rng.randbytes(n)), (b"\xff" * dlen, b"\xff" * n), (bytes(dlen), bytes(n))):
            assert lib().ht_hmac(h, buf(key), buf(msg), ctypes.c_size_t(n), out) == 0
            assert bytes(out) == hmac.new(key, msg, HASHES[h]).digest(), n


def _twin_nonce(cid, nb, d, z, extra):
    out = outbuf(nb)
    rejected = lib().ht_ecdsa_nonce(cid, buf(d.to_bytes(nb, "big")), buf(z), buf(extra) if extra else None, out)
    return int.from_bytes(bytes(out), "big"), rejected


@pytest.mark.parametrize("cn,cid", CURVES)
def test_generate_k_on_the_real_orders(cn, cid):
    c = M.CURVES[cn]
    nb = c.nbytes
    rng = random.Random(0x6979 + cid)
    cases = [(rng.randrange(1, c.n), rng.randbytes(nb)) for _ in range(500)]
    top = (1 << (8 * nb)) - 1
    cases += [(x, z.to_bytes(nb, "big")) for x in (1, c.n - 1) for z in (0, c.n - 1, c.n, c.n + 1, top)]
    for d, z in cases:
        for extra in (b"", rng.randbytes(nb)):
            assert _twin_nonce(cid, nb, d, z, extra) == (R.nonce(c, d, z, extra), 0), (hex(d), z.hex(), extra.hex())
    # a key outside [1, n - 1]: the batched call's zero
    for d in (0, c.n, c.n + 1, top):
        assert _twin_nonce(cid, nb, d, rng.randbytes(nb), b"")[0] == 0


def test_generate_k_rejection_branch():
    """q = 2^255 + 0x1D with SHA-256: every candidate is rejected with probability near 1/2, so the retry path (K = HMAC(K, V || 0x00),
    V = HMAC(K, V)) runs 0 .. 9 times among 2 000 inputs; the twin must agree with the model on k AND on the count"""
    q = (1 << 255) + 0x1D
    rng = random.Random(0x7e1ec7)
    out = outbuf(32)
    seen = {}
    for i in range(2000):
        x, h1 = rng.randbytes(32), rng.randbytes(32)
        extra = rng.randbytes(32) if i % 4 == 3 else b""
        want_k, want_rejections = R.generate_k(q, "sha256", x, h1, extra)
        rejected = lib().ht_rfc6979_generate_k(0, buf(x), buf(h1), buf(extra) if extra else None, buf(q.to_bytes(32, "big")), out)
        assert (int.from_bytes(bytes(out), "big"), rejected) == (want_k, want_rejections), i
        seen[min(rejected, 3)] = seen.get(min(rejected, 3), 0) + 1
    assert all(seen.get(r, 0) > 0 for r in (0, 1, 2, 3)), seen
    assert 800 < seen[0] < 1200, seen


def test_generate_k_rejection_branch_sha384():
    """the same branch on the 64-bit hash: q = 2^383 + 0x1D"""
    q = (1 << 383) + 0x1D
    rng = random.Random(0x384)
    out = outbuf(48)
    most = 0
    for i in range(300):
        x, h1 = rng.randbytes(48), rng.randbytes(48)
        extra = rng.randbytes(48) if i % 2 else b""
        want = R.generate_k(q, "sha384", x, h1, extra)
        rejected = lib().ht_rfc6979_generate_k(1, buf(x), buf(h1), buf(extra) if extra else None, buf(q.to_bytes(48, "big")), out)
        assert (int.from_bytes(bytes(out), "big"), rejected) == want, i
        most = max(most, rejected)
    assert most >= 3


def test_bip340_midstates():
    out = outbuf(32)
    for which, tag in enumerate((b"BIP0340/challenge", b"BIP0340/aux", b"BIP0340/nonce")):
        t = hashlib.sha256(tag).digest()
        assert lib().ht_bip340_midstate_digest(which, out) == 0
        assert bytes(out) == hashlib.sha256(t + t).digest(), tag


def test_bip340_nonce_step():
    rng = random.Random(0xb340)
    dp_out, rand_out = outbuf(32), outbuf(32)
    for i in range(200):
        d = rng.choice((1, N - 1)) if i < 8 else rng.randrange(1, N)
        odd = i & 1
        px, aux, m = rng.randbytes(32), rng.randbytes(32), rng.randbytes(32)
        assert lib().ht_bip340_nonce(buf(d.to_bytes(32, "big")), odd, buf(px), buf(aux), buf(m), dp_out, rand_out) == 0
        dp = N - d if odd else d
        t = (dp ^ int.from_bytes(M._tagged_hash(b"BIP0340/aux", aux), "big")).to_bytes(32, "big")
        assert int.from_bytes(bytes(dp_out), "big") == dp
        assert bytes(rand_out) == M._tagged_hash(b"BIP0340/nonce", t, px, m)


def test_bip340_accept_step():
    """NonZeroScalar::try_from: a rand outside [1, n - 1] is refused, not reduced"""
    for cn, cid in CURVES:
        n, nb = M.CURVES[cn].n, M.CURVES[cn].nbytes
        for v, want in ((0, 0), (n, 0), (n + 1, 0), ((1 << (8 * nb)) - 1, 0), (n - 1, 1), (1, 1)):
            x = buf(v.to_bytes(nb, "big"))
            assert lib().ht_nonzero_scalar(cid, x) == want, (cn, hex(v))
            assert int.from_bytes(bytes(x), "big") == (v if want else 0)


def _finish(k, r_odd, dp, r, px, m):
    s = outbuf(32)
    ok = lib().ht_bip340_finish(buf(k.to_bytes(32, "big")), r_odd, buf(dp.to_bytes(32, "big")), buf(r), buf(px), buf(m), s)
    return ok, int.from_bytes(bytes(s), "big")


def test_bip340_finish_step():
    rng = random.Random(0xf1)
    for i in range(200):
        k, dp = rng.randrange(1, N), rng.randrange(1, N)
        r, px, m = rng.randbytes(32), rng.randbytes(32), rng.randbytes(32)
        e = int.from_bytes(M._tagged_hash(b"BIP0340/challenge", r, px, m), "big") % N
        odd = i & 1
        assert _finish(k, odd, dp, r, px, m) == (1, ((N - k if odd else k) + e * dp) % N)
        # k = -e d' (as the nonce after the parity flip): s = 0 is refused
        k0 = (-e * dp) % N
        if k0:
            assert _finish(N - k0 if odd else k0, odd, dp, r, px, m) == (0, 0)


def test_bip340_steps_compose_to_the_reference_vectors(ref_vectors):
    """nonce, accept and finish chained with the oracle's curve arithmetic give the reference's own signatures"""
    c = M.K256
    vs = [v for v in ref_vectors["k256"]["bip340"]["sign"]]
    assert vs
    dp_out, rand_out = outbuf(32), outbuf(32)
    for v in vs:
        d = int(v["secret_key"], 16)
        aux, m = bytes.fromhex(v["aux_rand"]), bytes.fromhex(v["message"])
        P = M.affine_mul(c, d, (c.gx, c.gy))
        px = P[0].to_bytes(32, "big")
        assert lib().ht_bip340_nonce(buf(d.to_bytes(32, "big")), P[1] & 1, buf(px), buf(aux), buf(m), dp_out, rand_out) == 0
        k = int.from_bytes(bytes(rand_out), "big")
        Rp = M.affine_mul(c, k, (c.gx, c.gy))
        r = Rp[0].to_bytes(32, "big")
        ok, s = _finish(k, Rp[1] & 1, int.from_bytes(bytes(dp_out), "big"), r, px, m)
        assert ok == 1 and (r + s.to_bytes(32, "big")).hex() == v["signature"].lower()
