"""The message-level entry points (include/ecgpu.h, "from message bytes") on the GPU: ecgpu_ecdsa_sign_msg_batch,
ecgpu_ecdsa_verify_msg_batch, ecgpu_ecdsa_recover_msg_batch, ecgpu_schnorr_sign_msg_batch and ecgpu_schnorr_verify_msg_batch.
Expected values come from hashlib, the committed fixtures (Wycheproof, the reference's RFC 6979 signatures and recovery vectors), the
prehash entry points fed hashlib digests, and the host model of ecgpu/schnorr.py.  Everything is byte-exact."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import rfc6979_model as R
from conftest import GOLDEN
from oracle import ecmodel as M

pytestmark = pytest.mark.gpu

CURVES = ["k256", "p256", "p384"]
DIGEST = {"k256": hashlib.sha256, "p256": hashlib.sha256, "p384": hashlib.sha384}
ERR_ARG, ERR_UNSUPPORTED = -1, -4
N_RAGGED = 300


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


def padded(c, hx):
    b = bytes.fromhex(hx)
    return b[len(b) - c.nbytes:] if len(b) >= c.nbytes else bytes(c.nbytes - len(b)) + b


_BATCH = {}


def ragged(cn):
    """300 seeded (key, message of 0 .. 200 bytes, additional data) per curve and the hashlib digests: computed once, read-only"""
    if cn not in _BATCH:
        c = M.CURVES[cn]
        rng = random.Random(0x5167 + c.nbytes + len(cn))
        keys = [rng.randrange(1, c.n).to_bytes(c.nbytes, "big") for _ in range(N_RAGGED)]
        msgs = [rng.randbytes(rng.randrange(0, 201)) for _ in range(N_RAGGED)]
        msgs[0], msgs[1], msgs[2] = b"", rng.randbytes(200), rng.randbytes(128)
        extra = [rng.randbytes(c.nbytes) for _ in range(N_RAGGED)]
        _BATCH[cn] = (keys, msgs, extra, [DIGEST[cn](m).digest() for m in msgs])
    return _BATCH[cn]


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


@pytest.mark.parametrize("cn", CURVES)
def test_verify_msg_wycheproof(ctx, cn):
    """every Wycheproof row through Verifier::verify with the message hashed on the device: the `pass` column, and byte for byte
    what ecgpu_ecdsa_verify_batch says on hashlib digests of the same rows"""
    import ecgpu
    from ecgpu import ecdsa as E
    from ecgpu.der import decode_signature
    c, cv = M.CURVES[cn], ctx.curve(cn)
    nb = c.nbytes
    with open(os.path.join(GOLDEN, f"wycheproof_{cn}.json")) as f:
        rows = json.load(f)["rows"]
    keys = [padded(c, wx) + padded(c, wy) for wx, wy, _, _, _ in rows]
    msgs = [bytes.fromhex(r[2]) for r in rows]
    ders = [bytes.fromhex(r[3]) for r in rows]
    want = np.array([r[4] for r in rows], dtype=np.uint8)
    got = E.verify_der_batch_device(cv, keys, msgs, ders, normalize_s=(cn == "k256"))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"rows {bad[:10]} differ"
    assert want.sum() > 100
    assert bytes(got) == bytes(E.verify_der_batch(cv, keys, msgs, ders, normalize_s=(cn == "k256")))
    # the raw flags of the two C calls on the same decoded signatures
    sig = bytearray(len(rows) * 2 * nb)
    for i, der in enumerate(ders):
        rs = decode_signature(der, nb)
        if rs is not None:
            r, s = rs
            if cn == "k256" and c.n // 2 < s < c.n:
                s = c.n - s
            sig[2 * nb * i:2 * nb * (i + 1)] = r.to_bytes(nb, "big") + s.to_bytes(nb, "big")
    z = b"".join(DIGEST[cn](m).digest() for m in msgs)
    assert bytes(cv.ecdsa_verify_msg(msgs, bytes(sig), b"".join(keys))) == bytes(cv.ecdsa_verify(z, bytes(sig), b"".join(keys)))
    assert max(len(m) for m in msgs) >= 20 and ecgpu.pack_messages_aligned(msgs)[2] % 16 == 0


def test_sign_msg_reference_vectors(ctx):
    """the reference's RFC 6979 signatures whose hash is the curve's own digest, from the key and the message alone (the cross-hash
    vectors of the fixture belong to the prehash call)"""
    from ecgpu import ecdsa as E
    with open(os.path.join(GOLDEN, "rfc6979_sign.json")) as f:
        fixture = json.load(f)
    count = 0
    for cn, entry in fixture.items():
        cv = ctx.curve(cn)
        key = bytes.fromhex(entry["secret_key"])
        own = [v for v in entry["vectors"] if v["hash"] == DIGEST[cn]().name]
        sig, _, ok = E.sign_msg(cv, [key] * len(own), [bytes.fromhex(v["message"]) for v in own])
        assert ok.all()
        for i, v in enumerate(own):
            assert bytes(sig[i]).hex() == v["signature"], (cn, v["test"])
            count += 1
    assert count == 4


@pytest.mark.parametrize("cn", CURVES)
def test_sign_msg_equals_sign_prehash_on_hashlib_digests(ctx, cn):
    """a ragged batch of 300 messages of 0 .. 200 bytes: sig_rs, recovery_id and ok of ecgpu_ecdsa_sign_msg_batch equal those of
    ecgpu_ecdsa_sign_prehash_batch on hashlib digests - additional data absent and present, under ECGPU_ECDSA_LOW_S and under
    ECGPU_EXACT_REFERENCE, host and device buffers; verify_msg accepts every signature and rejects it once a message bit is flipped"""
    import ecgpu
    import torch
    cv = ctx.curve(cn)
    nb, n = cv.nb, N_RAGGED
    keys, msgs, extra, digests = ragged(cn)
    d, z = b"".join(keys), b"".join(digests)
    pub, inf = cv.mul_by_generator(d)
    assert not inf.any()
    rec, lens, stride = ecgpu.pack_messages_aligned(msgs)
    assert stride == 208
    rec[:] = np.where(np.arange(stride)[None, :] < lens[:, None], rec, 0xA5)       # bytes behind a message must not count
    for x in (None, b"".join(extra)):
        for flags in (ecgpu.ECDSA_LOW_S, ecgpu.EXACT_REFERENCE):
            want_sig, want_rid, want_ok = cv.ecdsa_sign_prehash(d, z, x, flags=flags)
            assert want_ok.all()
            sig, rid, ok = cv.ecdsa_sign_msg(d, msgs, x, flags=flags)
            assert bytes(sig) == bytes(want_sig) and bytes(rid) == bytes(want_rid) and bytes(ok) == bytes(want_ok), (x is None, flags)
            t_sig = torch.full((n, 2 * nb), 0xA5, dtype=torch.uint8, device="cuda")
            t_rid = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
            t_ok = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
            t_d, t_rec, t_len, t_x = _dev(_u8(d)), _dev(rec), _dev(lens.view(np.int32)), (None if x is None else _dev(_u8(x)))
            torch.cuda.synchronize()
            cv.ecdsa_sign_msg_device(t_d, t_rec, stride, t_len, t_x, t_sig, t_rid, t_ok, n, flags=flags)
            ctx.synchronize()
            assert bytes(t_sig.cpu().numpy()) == bytes(want_sig) and bytes(t_rid.cpu().numpy()) == bytes(want_rid) and bytes(t_ok.cpu().numpy()) == bytes(want_ok)
            if flags == ecgpu.ECDSA_LOW_S:
                vflags = ecgpu.ECDSA_LOW_S if cn == "k256" else 0
                assert cv.ecdsa_verify_msg(msgs, sig, pub, flags=vflags).all()
                t_vok = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
                cv.ecdsa_verify_msg_device(t_rec, stride, t_len, t_sig, _dev(pub), t_vok, n, flags=vflags)
                ctx.synchronize()
                assert bytes(t_vok.cpu().numpy()) == b"\x01" * n
                flipped = []
                for i, m in enumerate(msgs):
                    if not m:
                        flipped.append(b"\x00")                                     # the empty message grows by a byte instead
                    else:
                        b = bytearray(m)
                        b[(7 * i) % len(m)] ^= 1 << (i % 8)
                        flipped.append(bytes(b))
                assert not cv.ecdsa_verify_msg(flipped, sig, pub, flags=vflags).any()


@pytest.mark.parametrize("cn", CURVES)
def test_sign_msg_invalid_keys_and_refused_flag(ctx, cn):
    import ecgpu
    c, cv = M.CURVES[cn], ctx.curve(cn)
    nb = c.nbytes
    keys, msgs, _, digests = ragged(cn)
    ks = list(keys[:40])
    ks[7], ks[20] = bytes(nb), c.n.to_bytes(nb, "big")
    sig, rid, ok = cv.ecdsa_sign_msg(b"".join(ks), msgs[:40])
    want = cv.ecdsa_sign_prehash(b"".join(ks), b"".join(digests[:40]))
    assert bytes(sig) == bytes(want[0]) and bytes(rid) == bytes(want[1]) and bytes(ok) == bytes(want[2])
    good = np.ones(40, dtype=bool)
    good[[7, 20]] = False
    assert ok[good].all() and not ok[~good].any() and not sig[~good].any() and not rid[~good].any()
    with pytest.raises(ecgpu.EcgpuError, match="ECGPU_PUBLIC_SCALARS is refused"):
        cv.ecdsa_sign_msg(b"".join(keys[:4]), msgs[:4], flags=ecgpu.PUBLIC_SCALARS)


@pytest.mark.parametrize("cn", CURVES)
def test_recover_msg(ctx, cn, ref_vectors):
    """the reference's secp256k1 vectors (message text, compressed key), then on every curve sign_msg -> recover_msg = d G, byte for
    byte what ecgpu_ecdsa_recover_batch gives on hashlib digests"""
    from ecgpu import ecdsa as E
    cv = ctx.curve(cn)
    if cn == "k256":
        vs = ref_vectors["k256"]["recovery"]
        out, ok = E.recover_from_msg(cv, [v["msg"].encode() for v in vs], [bytes.fromhex(v["sig"]) for v in vs], [v["recid"] for v in vs])
        assert ok.all()
        assert [bytes(g).hex() for g in cv.to_bytes(out)] == [v["pk"] for v in vs]
    keys, msgs, _, digests = ragged(cn)
    d = b"".join(keys)
    sig, rid, ok = cv.ecdsa_sign_msg(d, msgs)
    assert ok.all()
    pub, _ = cv.mul_by_generator(d)
    out, rok = cv.ecdsa_recover_msg(msgs, sig, rid)
    assert rok.all() and bytes(out) == bytes(pub)
    wrong = rid ^ 1
    got, want = cv.ecdsa_recover_msg(msgs, sig, wrong), cv.ecdsa_recover(b"".join(digests), sig, wrong)
    assert bytes(got[0]) == bytes(want[0]) and bytes(got[1]) == bytes(want[1]) and bytes(got[0]) != bytes(pub)


def _limbs(b):
    """big-endian bytes -> little-endian 32-bit limbs, least significant first (the kernels' internal form)"""
    return b"".join(b[i:i + 4][::-1] for i in range(len(b) - 4, -1, -4))


@pytest.mark.parametrize("cn", CURVES)
def test_no_key_nonce_or_additional_data_stays_behind(ctx, cn):
    """ecgpu_ecdsa_sign_msg_batch from host buffers stages four inputs, the fourth (the additional data, a secret) in the slot
    that call brought: afterwards no key, no additional data and no nonce - as wire bytes or as limbs - is in the table, pipeline or
    hash workspace or in any of the 28 staging slots, while the public digests are where the digest kernel left them"""
    c, cv = M.CURVES[cn], ctx.curve(cn)
    n = 40
    keys, msgs, extra, digests = ragged(cn)
    keys, msgs, extra, digests = keys[:n], msgs[:n], extra[:n], digests[:n]
    sig, rid, ok = cv.ecdsa_sign_msg(b"".join(keys), msgs, b"".join(extra))
    assert ok.all()
    nonces = [R.nonce(c, int.from_bytes(keys[i], "big"), digests[i], extra[i]).to_bytes(c.nbytes, "big") for i in range(n)]
    blobs = {w: ctx.debug_workspace(w) for w in (0, 1, 3)}
    for slot in range(28):
        blobs[16 + slot] = ctx.debug_workspace(16 + slot)
    assert len(blobs[16 + 24]) > 0                       # the fourth input's slot exists: the additional data went through it
    assert blobs[3][:n * c.nbytes] == b"".join(digests)
    for which, blob in blobs.items():
        for i, sec in enumerate(keys + extra + nonces):
            assert sec not in blob and _limbs(sec) not in blob, (which, i)


def test_schnorr_msg(ctx):
    """BIP340 over SHA256(msg): schnorr_sign_msg = ecgpu_schnorr_sign_prehash_batch on hashlib digests (aux_rand NULL = an explicit zero
    buffer; random aux) = the host model of ecgpu/schnorr.py; schnorr_verify_msg accepts and rejects a flipped message"""
    from ecgpu import schnorr as S
    cv = ctx.curve("k256")
    keys, msgs, extra, digests = ragged("k256")
    n = N_RAGGED
    d, m = b"".join(keys), b"".join(digests)
    for aux in (None, bytes(32 * n), b"".join(extra)):
        want = cv.schnorr_sign_prehash(d, m, bytes(32 * n) if aux is None else aux)
        sig, px, ok = cv.schnorr_sign_msg(d, msgs, aux)
        assert want[2].all()
        assert bytes(sig) == bytes(want[0]) and bytes(px) == bytes(want[1]) and bytes(ok) == bytes(want[2]), aux is None
    model_sigs, model_px = S.sign_batch(cv, keys[:64], digests[:64], extra[:64])
    assert [bytes(r) for r in sig[:64]] == model_sigs and [bytes(r) for r in px[:64]] == model_px
    sigs, pxs = S.sign_msg_batch_device(cv, keys, msgs, extra)
    assert b"".join(sigs) == bytes(sig) and b"".join(pxs) == bytes(px)
    assert S.verify_msg_batch_device(cv, pxs, msgs, sigs).all()
    assert bytes(cv.schnorr_verify_msg(px, msgs, sig)) == bytes(cv.schnorr_verify_prehash(px, sig, m))
    flipped = [bytes([m0[0] ^ 1]) + m0[1:] if m0 else b"\x01" for m0 in msgs]
    assert not cv.schnorr_verify_msg(px, flipped, sig).any()
    # an invalid key: ok = 0 and zeros, as the prehash call
    ks = list(keys[:8])
    ks[3] = bytes(32)
    sig8, px8, ok8 = cv.schnorr_sign_msg(b"".join(ks), msgs[:8])
    want8 = cv.schnorr_sign_prehash(b"".join(ks), b"".join(digests[:8]), bytes(32 * 8))
    assert bytes(sig8) == bytes(want8[0]) and bytes(ok8) == bytes(want8[2]) and ok8[3] == 0 and not sig8[3].any()


def test_schnorr_msg_other_curves_unsupported(ctx):
    z = np.zeros((4, 64), dtype=np.uint8)
    lens = np.full(4, 5, dtype=np.uint32)
    ok = np.zeros(4, dtype=np.uint8)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    for curve in (1, 2):
        assert ctx.lib.ecgpu_schnorr_sign_msg_batch(ctx.handle, curve, vp(z), vp(z), 64, vp(lens), None, vp(z), None, vp(ok), 4, 0) == ERR_UNSUPPORTED
        assert "secp256k1 only" in ctx.last_error()
        assert ctx.lib.ecgpu_schnorr_verify_msg_batch(ctx.handle, curve, vp(z), vp(z), 64, vp(lens), vp(z), vp(ok), 4, 0) == ERR_UNSUPPORTED
    assert ctx.lib.ecgpu_schnorr_sign_msg_batch(ctx.handle, 9, vp(z), vp(z), 64, vp(lens), None, vp(z), None, vp(ok), 4, 0) == ERR_UNSUPPORTED


def test_message_argument_checks(ctx):
    """the rules of the hash calls hold for every message-level call: a host msg_len[i] above the stride, a stride that does not fit
    32 bits and NULL records with a stride are refused; n = 0 is nothing to do; stride 0 signs and verifies the empty message"""
    z = np.zeros((4, 96), dtype=np.uint8)
    lens = np.array([5, 64, 65, 0], dtype=np.uint32)
    ok = np.zeros(4, dtype=np.uint8)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    L = ctx.lib
    calls = [
        lambda m, st, ln, n: L.ecgpu_ecdsa_sign_msg_batch(ctx.handle, 0, vp(z), m, st, ln, None, vp(z), None, vp(ok), n, 0, 0),
        lambda m, st, ln, n: L.ecgpu_ecdsa_verify_msg_batch(ctx.handle, 1, m, st, ln, vp(z), vp(z), vp(ok), n, 0, 0),
        lambda m, st, ln, n: L.ecgpu_ecdsa_recover_msg_batch(ctx.handle, 2, m, st, ln, vp(z), vp(ok), vp(z), vp(ok), n, 0, 0),
        lambda m, st, ln, n: L.ecgpu_schnorr_sign_msg_batch(ctx.handle, 0, vp(z), m, st, ln, None, vp(z), None, vp(ok), n, 0),
        lambda m, st, ln, n: L.ecgpu_schnorr_verify_msg_batch(ctx.handle, 0, vp(z), m, st, ln, vp(z), vp(ok), n, 0),
    ]
    for call in calls:
        assert call(vp(z), 64, vp(lens), 4) == ERR_ARG and "msg_len[2] = 65" in ctx.last_error()
        assert call(vp(z), 1 << 32, None, 0) == ERR_ARG
        assert call(None, 64, None, 2) == ERR_ARG
        assert call(vp(z), 64, vp(lens), 0) == 0
    assert L.ecgpu_ecdsa_sign_msg_batch(ctx.handle, 0, None, vp(z), 64, None, None, vp(z), None, vp(ok), 2, 0, 0) == ERR_ARG
    assert L.ecgpu_ecdsa_verify_msg_batch(ctx.handle, 0, vp(z), 64, None, None, vp(z), vp(ok), 2, 0, 0) == ERR_ARG
    cv = ctx.curve("p256")
    key = (12345).to_bytes(32, "big")
    sig, rid, sok = cv.ecdsa_sign_msg(key * 3, [b"", b"", b""])
    want = cv.ecdsa_sign_prehash(key * 3, hashlib.sha256(b"").digest() * 3)
    assert sok.all() and bytes(sig) == bytes(want[0]) and bytes(rid) == bytes(want[1])
    pub, _ = cv.mul_by_generator(key * 3)
    assert cv.ecdsa_verify_msg([b"", b"", b""], sig, pub).all()
