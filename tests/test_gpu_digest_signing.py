"""ECDSA from message bytes on a chosen digest (include/ecgpu.h: ecgpu_ecdsa_sign_digest_batch, ecgpu_ecdsa_verify_digest_batch,
ecgpu_ecdsa_recover_digest_batch) on the GPU: the reference's Ethereum example (tests/golden/keccak_ecdsa.json, from
k256/src/ecdsa.rs:84-143 and :312-342), round trips of ragged batches against tests/keccak_model.py, hashlib and
tests/rfc6979_model.py - the nonce keeps the curve's own HMAC-DRBG hash whatever the digest - the equality with the *_msg_batch
calls where the hash is the curve's own, the refused pairings, and the clearing of the nonces.  Everything is byte-exact."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import keccak_model as K
import rfc6979_model as R
from conftest import GOLDEN
from oracle import ecmodel as M

pytestmark = pytest.mark.gpu

SHA256, SHA384, KECCAK256, SHA3_256, SHA3_384 = 0, 1, 16, 17, 18
LOW_S, PUBLIC_SCALARS = 2, 4
ERR_ARG = -1
N = 70
STRIDE = 301                                    # unaligned: record i starts i mod 4 bytes off a word boundary
PAIRS = [("k256", KECCAK256), ("k256", SHA3_256), ("p256", KECCAK256), ("p384", SHA3_384)]
OWN = {"k256": SHA256, "p256": SHA256, "p384": SHA384}


def _hash(h, msg):
    if h == KECCAK256:
        return K.keccak256(msg)
    return hashlib.new({SHA256: "sha256", SHA384: "sha384", SHA3_256: "sha3_256", SHA3_384: "sha3_384"}[h], msg).digest()


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "keccak_ecdsa.json")) as f:
        return json.load(f)


_BATCH = {}


def batch(cn):
    """70 seeded (key, message of 0 .. 300 bytes, additional data) per curve, keys 11 and 40 replaced by 0 and n; the records at
    the unaligned stride with 0xA5 behind each message: computed once, read-only"""
    if cn not in _BATCH:
        c = M.CURVES[cn]
        rng = random.Random(0xD16 + c.nbytes + len(cn))
        keys = [rng.randrange(1, c.n).to_bytes(c.nbytes, "big") for _ in range(N)]
        keys[11], keys[40] = bytes(c.nbytes), c.n.to_bytes(c.nbytes, "big")
        msgs = [rng.randbytes(rng.randrange(0, 301)) for _ in range(N)]
        msgs[0], msgs[1], msgs[2], msgs[3] = b"", rng.randbytes(300), rng.randbytes(135), rng.randbytes(103)
        extra = [rng.randbytes(c.nbytes) for _ in range(N)]
        rec = np.full(N * STRIDE, 0xA5, dtype=np.uint8)
        for k, m in enumerate(msgs):
            rec[k * STRIDE:k * STRIDE + len(m)] = np.frombuffer(m, dtype=np.uint8)
        lens = np.array([len(m) for m in msgs], dtype=np.uint32)
        _BATCH[cn] = (keys, msgs, extra, rec, lens)
    return _BATCH[cn]


_DIGESTS = {}


def digests(cn, h):
    if (cn, h) not in _DIGESTS:
        _DIGESTS[cn, h] = [_hash(h, m) for m in batch(cn)[1]]
    return _DIGESTS[cn, h]


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _dp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sign(ctx, curve, h, d, rec, stride, lens, x, n, nb, mem, flags, name="ecgpu_ecdsa_sign_digest_batch"):
    """the C call -> (rc, sig, recid, ok); outputs start as 0xA5.  name: the *_msg_batch twin takes no hash"""
    hash_arg = () if name.endswith("_msg_batch") else (h,)
    sig, rid, ok = np.full((n, 2 * nb), 0xA5, dtype=np.uint8), np.full(n, 0xA5, dtype=np.uint8), np.full(n, 0xA5, dtype=np.uint8)
    fn = getattr(ctx.lib, name)
    if mem == 0:
        rc = fn(ctx.handle, curve, *hash_arg, _vp(d), _vp(rec), stride, _vp(lens), _vp(x), _vp(sig), _vp(rid), _vp(ok), n, 0, flags)
        return rc, sig, rid, ok
    import torch
    t = [_dev(d), _dev(rec), _dev(lens.view(np.int32)), _dev(x), _dev(sig), _dev(rid), _dev(ok)]
    torch.cuda.synchronize()
    rc = fn(ctx.handle, curve, *hash_arg, _dp(t[0]), _dp(t[1]), stride, _dp(t[2]), _dp(t[3]), _dp(t[4]), _dp(t[5]), _dp(t[6]), n, 1, flags)
    ctx.synchronize()
    return rc, t[4].cpu().numpy(), t[5].cpu().numpy(), t[6].cpu().numpy()


def verify(ctx, curve, h, rec, stride, lens, sig, pub, n, mem, flags, name="ecgpu_ecdsa_verify_digest_batch"):
    hash_arg = () if name.endswith("_msg_batch") else (h,)
    ok = np.full(n, 0xA5, dtype=np.uint8)
    fn = getattr(ctx.lib, name)
    if mem == 0:
        return fn(ctx.handle, curve, *hash_arg, _vp(rec), stride, _vp(lens), _vp(sig), _vp(pub), _vp(ok), n, 0, flags), ok
    import torch
    t = [_dev(rec), _dev(lens.view(np.int32)), _dev(sig), _dev(pub), _dev(ok)]
    torch.cuda.synchronize()
    rc = fn(ctx.handle, curve, *hash_arg, _dp(t[0]), stride, _dp(t[1]), _dp(t[2]), _dp(t[3]), _dp(t[4]), n, 1, flags)
    ctx.synchronize()
    return rc, t[4].cpu().numpy()


def recover(ctx, curve, h, rec, stride, lens, sig, rid, n, nb, mem, flags, name="ecgpu_ecdsa_recover_digest_batch"):
    hash_arg = () if name.endswith("_msg_batch") else (h,)
    pub, ok = np.full((n, 2 * nb), 0xA5, dtype=np.uint8), np.full(n, 0xA5, dtype=np.uint8)
    fn = getattr(ctx.lib, name)
    if mem == 0:
        return fn(ctx.handle, curve, *hash_arg, _vp(rec), stride, _vp(lens), _vp(sig), _vp(rid), _vp(pub), _vp(ok), n, 0, flags), pub, ok
    import torch
    t = [_dev(rec), _dev(lens.view(np.int32)), _dev(sig), _dev(rid), _dev(pub), _dev(ok)]
    torch.cuda.synchronize()
    rc = fn(ctx.handle, curve, *hash_arg, _dp(t[0]), stride, _dp(t[1]), _dp(t[2]), _dp(t[3]), _dp(t[4]), _dp(t[5]), n, 1, flags)
    ctx.synchronize()
    return rc, t[4].cpu().numpy(), t[5].cpu().numpy()


def test_ethereum_example(ctx, fixture):
    """sign_digest_recoverable gives the signature and recovery id 0, recover_from_digest the signer's key and the key of the second
    vector, verify_digest accepts, and one flipped message byte is rejected"""
    c = M.K256
    s, v = fixture["sign"], fixture["recover"]
    msg = bytes.fromhex(s["message"])
    assert len(msg) == 42
    d = _u8(bytes.fromhex(s["secret_key"]))
    rec, lens = np.zeros(44, dtype=np.uint8), np.array([42], dtype=np.uint32)
    rec[:42] = _u8(msg)
    for mem in (0, 1):
        rc, sig, rid, ok = sign(ctx, 0, KECCAK256, d, rec, 44, lens, None, 1, 32, mem, LOW_S)
        assert rc == 0, ctx.last_error()
        assert ok[0] == 1 and bytes(sig[0]).hex() == s["signature"] and rid[0] == s["recovery_id"], mem
    # both vectors in one batch of recoveries: different lengths, one stride
    msgs = [msg, v["message_text"].encode()]
    rec2 = np.full(2 * 44, 0xA5, dtype=np.uint8)
    for k, m in enumerate(msgs):
        rec2[44 * k:44 * k + len(m)] = _u8(m)
    lens2 = np.array([len(m) for m in msgs], dtype=np.uint32)
    sig2 = _u8(bytes.fromhex(s["signature"]) + bytes.fromhex(v["signature"]))
    rid2 = np.array([s["recovery_id"], v["recovery_id"]], dtype=np.uint8)
    P = M.affine_mul(c, int(s["secret_key"], 16), (c.gx, c.gy))
    for mem in (0, 1):
        rc, pub, ok = recover(ctx, 0, KECCAK256, rec2, 44, lens2, sig2, rid2, 2, 32, mem, LOW_S)
        assert rc == 0, ctx.last_error()
        assert ok.all() and bytes(pub[0]) == M.i2b(c, P[0]) + M.i2b(c, P[1]), mem
        x, y = int.from_bytes(bytes(pub[1][:32]), "big"), int.from_bytes(bytes(pub[1][32:]), "big")
        assert M.group_to_bytes(c, (x, y)).hex() == v["public_key_sec1"], mem
        rc, vok = verify(ctx, 0, KECCAK256, rec2, 44, lens2, sig2, pub, 2, mem, LOW_S)
        assert rc == 0 and bytes(vok) == b"\x01\x01", mem
        bad = rec2.copy()
        bad[7] ^= 0x10
        bad[44 + 3] ^= 0x01
        rc, vok = verify(ctx, 0, KECCAK256, bad, 44, lens2, sig2, pub, 2, mem, LOW_S)
        assert rc == 0 and bytes(vok) == b"\x00\x00", mem
    # the same message under SHA3-256 or the curve's own SHA-256 signs differently: the hash argument is what is hashed with
    others = {bytes(sign(ctx, 0, h, d, rec, 44, lens, None, 1, 32, 0, LOW_S)[1]) for h in (SHA256, SHA3_256)}
    assert len(others) == 2 and bytes.fromhex(s["signature"]) not in others


@pytest.mark.parametrize("cn,h", PAIRS)
def test_round_trip_against_the_model(ctx, cn, h):
    """70 ragged messages of 0 .. 300 bytes at an unaligned stride, host and device memory, additional data absent and present:
    sign_digest = the model's signature over the model's digest with the RFC 6979 nonce of the CURVE's HMAC hash; keys 0 and n
    give ok = 0 and zeros; recover_digest returns d G; verify_digest accepts, and rejects after a flipped message bit"""
    c = M.CURVES[cn]
    cid, nb = M.CURVE_IDS[cn], c.nbytes
    flags = LOW_S if cn == "k256" else 0
    keys, msgs, extra, rec, lens = batch(cn)
    zs = digests(cn, h)
    good = [i for i in range(N) if i not in (11, 40)]
    pub = np.zeros((N, 2 * nb), dtype=np.uint8)
    for i in good:
        Q = M.affine_mul(c, int.from_bytes(keys[i], "big"), (c.gx, c.gy))
        pub[i] = _u8(M.i2b(c, Q[0]) + M.i2b(c, Q[1]))
    d = _u8(b"".join(keys))
    for x in (None, extra):
        want_sig, want_rid = np.zeros((N, 2 * nb), dtype=np.uint8), np.zeros(N, dtype=np.uint8)
        for i in good:
            di = int.from_bytes(keys[i], "big")
            k = R.nonce(c, di, zs[i], b"" if x is None else x[i])
            r, s, rid = M.ecdsa_sign_prehashed(c, di, k, zs[i], normalize_s=(cn == "k256"))
            want_sig[i], want_rid[i] = _u8(M.i2b(c, r) + M.i2b(c, s)), rid
        want_ok = np.ones(N, dtype=np.uint8)
        want_ok[[11, 40]] = 0
        xa = None if x is None else _u8(b"".join(x))
        for mem in (0, 1):
            rc, sig, rid, ok = sign(ctx, cid, h, d, rec, STRIDE, lens, xa, N, nb, mem, flags)
            assert rc == 0, ctx.last_error()
            assert bytes(ok) == bytes(want_ok) and bytes(sig) == bytes(want_sig) and bytes(rid) == bytes(want_rid), (x is None, mem)
            assert not sig[11].any() and not sig[40].any()
            rc, got, rok = recover(ctx, cid, h, rec, STRIDE, lens, sig, rid, N, nb, mem, flags)
            assert rc == 0, ctx.last_error()
            assert bytes(rok) == bytes(want_ok) and bytes(got) == bytes(pub), (x is None, mem)
            rc, vok = verify(ctx, cid, h, rec, STRIDE, lens, sig, pub, N, mem, flags)
            assert rc == 0 and bytes(vok) == bytes(want_ok), (x is None, mem)
            flipped = rec.copy()
            for i, m in enumerate(msgs):
                if m:
                    flipped[i * STRIDE + (7 * i) % len(m)] ^= 1 << (i % 8)
            fl_lens = np.where(lens == 0, 1, lens).astype(np.uint32)                       # the empty message grows by a byte instead
            rc, vok = verify(ctx, cid, h, flipped, STRIDE, fl_lens, sig, pub, N, mem, flags)
            assert rc == 0 and not vok.any(), (x is None, mem)


@pytest.mark.parametrize("cn", ["k256", "p256", "p384"])
def test_the_curves_own_hash_is_the_msg_call(ctx, cn):
    """with hash = the curve's own digest the three calls give byte for byte what ecgpu_ecdsa_{sign,verify,recover}_msg_batch give"""
    c = M.CURVES[cn]
    cid, nb, h = M.CURVE_IDS[cn], c.nbytes, OWN[cn]
    flags = LOW_S if cn == "k256" else 0
    keys, msgs, extra, rec, lens = batch(cn)
    d, xa = _u8(b"".join(keys)), _u8(b"".join(extra))
    for mem in (0, 1):
        for x in (None, xa):
            a = sign(ctx, cid, h, d, rec, STRIDE, lens, x, N, nb, mem, flags)
            b = sign(ctx, cid, h, d, rec, STRIDE, lens, x, N, nb, mem, flags, name="ecgpu_ecdsa_sign_msg_batch")
            assert a[0] == 0 and b[0] == 0, ctx.last_error()
            assert all(bytes(p) == bytes(q) for p, q in zip(a[1:], b[1:])), (mem, x is None)
            assert a[3].sum() == N - 2
        _, sig, rid, _ = a
        ra = recover(ctx, cid, h, rec, STRIDE, lens, sig, rid, N, nb, mem, flags)
        rb = recover(ctx, cid, h, rec, STRIDE, lens, sig, rid, N, nb, mem, flags, name="ecgpu_ecdsa_recover_msg_batch")
        assert ra[0] == 0 and rb[0] == 0 and bytes(ra[1]) == bytes(rb[1]) and bytes(ra[2]) == bytes(rb[2]) and ra[2].sum() == N - 2, mem
        va = verify(ctx, cid, h, rec, STRIDE, lens, sig, ra[1], N, mem, flags)
        vb = verify(ctx, cid, h, rec, STRIDE, lens, sig, ra[1], N, mem, flags, name="ecgpu_ecdsa_verify_msg_batch")
        assert va[0] == 0 and vb[0] == 0 and bytes(va[1]) == bytes(vb[1]) and va[1].sum() == N - 2, mem
    # and the digest is hashlib's: the signature is the prehash call's on it
    z = b"".join(_hash(h, m) for m in msgs)
    want = ctx.curve(cn).ecdsa_sign_prehash(bytes(d), z, bytes(xa), flags=flags)
    assert bytes(want[0]) == bytes(a[1]) and bytes(want[1]) == bytes(a[2]) and bytes(want[2]) == bytes(a[3])


def test_refusals(ctx):
    """a digest that does not fill the field, an unknown hash and ECGPU_PUBLIC_SCALARS on signing: ECGPU_ERR_ARG, the text names the
    hash and the curve, and no output byte is written"""
    keys, msgs, extra, rec, lens = batch("p384")
    d = _u8(b"".join(keys))
    pairs = [(0, SHA384, "SHA-384", "secp256k1"), (2, KECCAK256, "Keccak-256", "P-384"), (1, SHA3_384, "SHA3-384", "P-256"), (0, 2, "unknown hash 2", "")]
    for cid, h, hname, cname in pairs:
        nb = 48 if cid == 2 else 32
        rc, sig, rid, ok = sign(ctx, cid, h, d, rec, STRIDE, lens, None, N, nb, 0, 0)
        assert rc == ERR_ARG and hname in ctx.last_error() and cname in ctx.last_error() and "ecgpu_ecdsa_sign_digest_batch" in ctx.last_error()
        assert (sig == 0xA5).all() and (rid == 0xA5).all() and (ok == 0xA5).all()
        sig0, rid0 = np.zeros((N, 2 * nb), dtype=np.uint8), np.zeros(N, dtype=np.uint8)
        rc, vok = verify(ctx, cid, h, rec, STRIDE, lens, sig0, sig0, N, 0, 0)
        assert rc == ERR_ARG and hname in ctx.last_error() and cname in ctx.last_error() and (vok == 0xA5).all()
        rc, pub, rok = recover(ctx, cid, h, rec, STRIDE, lens, sig0, rid0, N, nb, 0, 0)
        assert rc == ERR_ARG and hname in ctx.last_error() and cname in ctx.last_error() and (pub == 0xA5).all() and (rok == 0xA5).all()
    rc, sig, rid, ok = sign(ctx, 0, KECCAK256, d, rec, STRIDE, lens, None, N, 32, 0, LOW_S | PUBLIC_SCALARS)
    assert rc == ERR_ARG and "ECGPU_PUBLIC_SCALARS is refused" in ctx.last_error() and (sig == 0xA5).all() and (ok == 0xA5).all()
    # the rules of the message arguments hold
    over = lens.copy()
    over[5] = STRIDE + 1
    rc, sig, rid, ok = sign(ctx, 0, KECCAK256, d, rec, STRIDE, over, None, N, 32, 0, LOW_S)
    assert rc == ERR_ARG and "msg_len[5] = 302" in ctx.last_error() and (sig == 0xA5).all()
    assert sign(ctx, 0, KECCAK256, d, rec, STRIDE, lens, None, 0, 32, 0, LOW_S)[0] == 0          # n = 0: nothing to do


def _limbs(b):
    """big-endian bytes -> little-endian 32-bit limbs, least significant first (the kernels' internal form)"""
    return b"".join(b[i:i + 4][::-1] for i in range(len(b) - 4, -1, -4))


def test_no_nonce_stays_behind(ctx):
    """after ecgpu_ecdsa_sign_digest_batch the pipeline workspace (ecgpu_debug_workspace 1) holds no nonce of the batch, as wire bytes
    or as limbs - nor a key or additional data - while the public Keccak digests are where the digest kernel left them (workspace 3)"""
    c = M.K256
    keys, msgs, extra, rec, lens = batch("k256")
    zs = digests("k256", KECCAK256)
    good = [i for i in range(N) if i not in (11, 40)]
    rc, sig, rid, ok = sign(ctx, 0, KECCAK256, _u8(b"".join(keys)), rec, STRIDE, lens, _u8(b"".join(extra)), N, 32, 0, LOW_S)
    assert rc == 0 and ok.sum() == N - 2
    nonces = [R.nonce(c, int.from_bytes(keys[i], "big"), zs[i], extra[i]).to_bytes(32, "big") for i in good]
    ws = ctx.debug_workspace(1)
    assert len(ws) > 0
    for i, sec in enumerate(nonces + [keys[i] for i in good] + [extra[i] for i in good]):
        assert sec not in ws and _limbs(sec) not in ws, i
    assert ctx.debug_workspace(3)[:N * 32] == b"".join(zs)
