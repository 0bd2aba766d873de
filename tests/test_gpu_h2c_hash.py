"""The entry points that start from bytes (include/ecgpu.h, "hash to curve"): ecgpu_expand_message_xmd_batch,
ecgpu_field_from_okm_batch, ecgpu_hash_to_curve_batch, ecgpu_hash_to_scalar_batch and ecgpu_schnorr_verify_prehash_batch, on the
GPU against hashlib (through the oracle's expand_message_xmd), Python integers, the RFC 9380 / VOPRF / BIP340 vectors and the
entry points that were there before (ecgpu_map_to_curve_batch, ecgpu_schnorr_verify_batch).  Everything is byte-exact."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import ecmodel as M
from test_hosttwin_h2c_hash import okm_edge_values

pytestmark = pytest.mark.gpu

HASHES = {0: "sha256", 1: "sha384"}
CURVES = [("k256", 0), ("p256", 1), ("p384", 2)]
RFC_DST = b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_"       # 49 bytes


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


def _np(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _xmd_raw(ctx, h, rec, stride, lens, dst, out_bytes, n, mem=0):
    """ecgpu_expand_message_xmd_batch as the C caller sees it -> (rc, out); mem = 1 round-trips the buffers through torch tensors"""
    import torch
    d = _np(dst)
    out = np.zeros((n, out_bytes), dtype=np.uint8)
    if mem == 0:
        rc = ctx.lib.ecgpu_expand_message_xmd_batch(ctx.handle, h, _vp(rec), stride, _vp(lens), _vp(d), len(d), _vp(out), out_bytes, n, 0)
        return rc, out
    t_rec = torch.from_numpy(rec).cuda() if rec is not None and rec.size else None
    t_len = torch.from_numpy(lens.view(np.int32)).cuda() if lens is not None else None
    t_out = torch.zeros((n, out_bytes), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.ecgpu_expand_message_xmd_batch(ctx.handle, h, ctypes.c_void_p(t_rec.data_ptr()) if t_rec is not None else None, stride,
                                                ctypes.c_void_p(t_len.data_ptr()) if t_len is not None else None, _vp(d), len(d),
                                                ctypes.c_void_p(t_out.data_ptr()), out_bytes, n, 1)
    ctx.synchronize()
    return rc, t_out.cpu().numpy()


@pytest.mark.parametrize("h,out_bytes", [(0, 96), (1, 144)])
def test_xmd_ragged_batches(ctx, h, out_bytes):
    """one ragged call per hash and DST length (message lengths 0 .. 200 in records of 200 bytes), uniform calls with stride 0
    and 133, host and device buffers"""
    import ecgpu
    rng = random.Random(0x9380 + h)
    msgs = [rng.randbytes(k) for k in range(201)]
    rec, lens, stride = ecgpu.pack_messages(msgs, 200)
    rec[:] = np.where(np.arange(200)[None, :] < lens[:, None], rec, 0xA5)         # bytes behind a message must not count
    for dst_len, mem in ((1, 0), (49, 0), (255, 0), (49, 1)):
        dst = rng.randbytes(dst_len)
        rc, out = _xmd_raw(ctx, h, rec, 200, lens, dst, out_bytes, 201, mem)
        assert rc == 0, ctx.last_error()
        for k, m in enumerate(msgs):
            assert bytes(out[k]) == M.expand_message_xmd(HASHES[h], m, dst, out_bytes), (dst_len, mem, k)
    dst = rng.randbytes(49)
    for stride, mem in ((0, 0), (133, 0), (133, 1), (0, 1)):
        n = 70
        rec = np.frombuffer(rng.randbytes(n * stride), dtype=np.uint8).reshape(n, stride).copy()
        rc, out = _xmd_raw(ctx, h, rec, stride, None, dst, out_bytes, n, mem)
        assert rc == 0, ctx.last_error()
        for k in range(n):
            assert bytes(out[k]) == M.expand_message_xmd(HASHES[h], bytes(rec[k]), dst, out_bytes), (stride, mem, k)


@pytest.mark.parametrize("h", [0, 1])
def test_xmd_output_lengths(ctx, h):
    """one digest, a cut digest, and the longest output (255 digests)"""
    import ecgpu
    rng = random.Random(0x1e + h)
    msgs = [rng.randbytes(k) for k in (0, 1, 55, 64, 111, 128, 200)]
    db = 48 if h else 32
    for out_bytes in (1, db, db + 1, 255 * db):
        out = ecgpu.expand_message_xmd(ctx, h, msgs, RFC_DST, out_bytes)
        for k, m in enumerate(msgs):
            assert bytes(out[k]) == M.expand_message_xmd(HASHES[h], m, RFC_DST, out_bytes), (out_bytes, k)


@pytest.mark.parametrize("h", [0, 1])
def test_xmd_at_scale(ctx, h):
    """2^16 + 3 messages, lengths cycling 0 .. 70: more than one pass of the grid"""
    n = (1 << 16) + 3
    L = 32
    rng = np.random.default_rng(0xabc + h)
    rec = rng.integers(0, 256, size=(n, 70), dtype=np.uint8)
    lens = (np.arange(n) % 71).astype(np.uint32)
    rc, out = _xmd_raw(ctx, h, rec, 70, lens, RFC_DST, L, n)
    assert rc == 0, ctx.last_error()
    raw = rec.tobytes()
    want = b"".join(M.expand_message_xmd(HASHES[h], raw[70 * k:70 * k + int(lens[k])], RFC_DST, L) for k in range(n))
    assert out.tobytes() == want


@pytest.mark.parametrize("cn,cid", CURVES)
def test_field_from_okm(ctx, cn, cid):
    c = M.CURVES[cn]
    L = 72 if cn == "p384" else 48
    rng = random.Random(0x0c3 + cid)
    values = okm_edge_values(c, L) + [rng.getrandbits(8 * L) for _ in range(4096)]
    out = ctx.curve(cn).field_from_okm(b"".join(v.to_bytes(L, "big") for v in values))
    assert out.tobytes() == b"".join((v % c.p).to_bytes(c.nbytes, "big") for v in values)


def _ragged_messages(seed, n=256, longest=150):
    rng = random.Random(seed)
    return [rng.randbytes(rng.randrange(0, longest + 1)) for _ in range(n)]


@pytest.mark.parametrize("cn,cid", CURVES)
def test_hash_to_curve_rfc_vectors(ctx, cn, cid, ref_vectors):
    """msg -> P of the five RFC 9380 vectors per curve (the longest message has 517 bytes: stride 517 with lengths)"""
    import ecgpu
    c = M.CURVES[cn]
    vs = ref_vectors[cn]["hash2curve"]
    msgs = [v["msg"].encode() for v in vs]
    assert max(map(len, msgs)) == 517
    rec, lens, stride = ecgpu.pack_messages(msgs, 517)
    dst = _np(vs[0]["dst"].encode())
    assert all(v["dst"] == vs[0]["dst"] for v in vs)
    out, inf = np.zeros((5, 2 * c.nbytes), dtype=np.uint8), np.ones(5, dtype=np.uint8)
    rc = ctx.lib.ecgpu_hash_to_curve_batch(ctx.handle, cid, _vp(rec), 517, _vp(lens), _vp(dst), len(dst), ecgpu.H2C_RO, _vp(out), _vp(inf), 5, 0)
    assert rc == 0, ctx.last_error()
    assert [bytes(o).hex() for o in out] == [v["p_x"] + v["p_y"] for v in vs] and not inf.any()


@pytest.mark.parametrize("cn,cid", CURVES)
def test_hash_to_curve_random_messages(ctx, cn, cid):
    """RO and NU on 256 ragged messages against the map entry point fed with the oracle's hash_to_field, and a sample against the
    oracle's hash_to_curve"""
    import ecgpu
    from ecgpu import hash2curve
    c = M.CURVES[cn]
    cv = ctx.curve(cn)
    msgs = _ragged_messages(0x4a5 + cid)
    dst = b"ecgpu-test-" + cn.encode() + b"_XMD_SSWU_RO_"
    u2 = b"".join(x.to_bytes(c.nbytes, "big") for m in msgs for x in M.hash_to_field(c, m, dst, 2))
    want, want_inf = cv.map_to_curve(u2, count=2)
    got, got_inf = cv.hash_to_curve(msgs, dst, ecgpu.H2C_RO)
    assert got.tobytes() == want.tobytes() and (got_inf == want_inf).all()
    got_dev, inf_dev = hash2curve.hash_from_bytes_device(cv, msgs, dst)
    assert got_dev.tobytes() == want.tobytes() and (inf_dev == want_inf).all()
    for k in range(0, 256, 8):
        x, y = M.hash_to_curve(c, msgs[k], dst)
        assert bytes(got[k]) == x.to_bytes(c.nbytes, "big") + y.to_bytes(c.nbytes, "big"), k
    u1 = b"".join(M.hash_to_field(c, m, dst, 1)[0].to_bytes(c.nbytes, "big") for m in msgs)
    want, want_inf = cv.map_to_curve(u1, count=1)
    got, got_inf = cv.hash_to_curve(msgs, dst, ecgpu.H2C_NU)
    assert got.tobytes() == want.tobytes() and (got_inf == want_inf).all()


@pytest.mark.parametrize("cn,cid", CURVES)
def test_hash_to_scalar(ctx, cn, cid):
    c = M.CURVES[cn]
    L = 72 if cn == "p384" else 48
    msgs = _ragged_messages(0x5ca + cid)
    dst = b"ecgpu-test-" + cn.encode() + b"-hash_to_scalar"
    got = ctx.curve(cn).hash_to_scalar(msgs, dst)
    want = b"".join((int.from_bytes(M.expand_message_xmd(M.h2c_hash_name(c), m, dst, L), "big") % c.n).to_bytes(c.nbytes, "big") for m in msgs)
    assert got.tobytes() == want


@pytest.mark.parametrize("cn", ["p256", "p384"])
def test_hash_to_scalar_voprf_vectors(ctx, cn):
    """DeriveKeyPair of draft-irtf-cfrg-voprf as the reference's hash_to_scalar tests run it: msg = seed || I2OSP(len(key_info), 2)
    || key_info || I2OSP(counter, 1), the first counter whose scalar is not zero (counter 0 in every vector)"""
    with open(os.path.join(GOLDEN, "voprf_hash_to_scalar.json")) as f:
        vs = json.load(f)[cn]
    assert len(vs) == 3
    cv = ctx.curve(cn)
    for v in vs:
        ki = bytes.fromhex(v["key_info"])
        msgs = [bytes.fromhex(v["seed"]) + len(ki).to_bytes(2, "big") + ki + bytes([counter]) for counter in range(4)]
        out = cv.hash_to_scalar(msgs, bytes.fromhex(v["dst"]))
        first = next(k for k in range(4) if any(out[k]))
        assert bytes(out[first]).hex() == v["sk_sm"]


@pytest.mark.parametrize("cn,cid", CURVES)
def test_hash_to_scalar_leaves_nothing_behind(ctx, cn, cid):
    """after a call from host buffers neither the pipeline workspace (1) nor any staging slot holds a message, an okm or an
    output scalar (wire form or limb-reversed)"""
    c = M.CURVES[cn]
    L = 72 if cn == "p384" else 48
    rng = random.Random(0x4e6 + cid)
    n = 3000
    msgs = [rng.randbytes(64) for _ in range(n)]
    dst = b"ecgpu-test-hygiene"
    out = ctx.curve(cn).hash_to_scalar(msgs, dst)
    assert any(out[0])
    ws = ctx.debug_workspace(1)
    assert len(ws) >= n * L and not any(ws[:n * L]), "the uniform bytes were left in the workspace"
    slots = [ctx.debug_workspace(16 + k) for k in range(24)]
    assert sum(map(len, slots)) > 0
    assert not any(slots[0][:n * 64]) and not any(slots[2][:n * c.nbytes]), "staged messages / scalars were left behind"
    words = lambda b: b"".join(b[i:i + 4][::-1] for i in range(len(b) - 4, -1, -4))
    for k in (0, 1, 63, 64, 255, 256, n - 1):
        okm = M.expand_message_xmd(M.h2c_hash_name(c), msgs[k], dst, L)
        for name, blob in [("workspace 1", ws)] + [("staging slot %d" % j, s) for j, s in enumerate(slots)]:
            for what, secret in (("message", msgs[k]), ("okm", okm), ("scalar", bytes(out[k]))):
                assert secret not in blob and words(secret) not in blob, (name, k, what)


def test_schnorr_verify_prehash(ctx, ref_vectors):
    """every BIP340 vector of the fixtures: the same answers as ecgpu_schnorr_verify_batch on host-computed challenges, and the
    vectors' expected results; other curves are refused"""
    import ecgpu
    from ecgpu import schnorr
    cv = ctx.curve("k256")
    v = ref_vectors["k256"]["bip340"]
    keys = [bytes.fromhex(t["public_key"]) for t in v["verify"] + v["sign"]]
    msgs = [bytes.fromhex(t["message"]) for t in v["verify"] + v["sign"]]
    sigs = [bytes.fromhex(t["signature"]) for t in v["verify"] + v["sign"]]
    want = [t["valid"] for t in v["verify"]] + [True] * len(v["sign"])
    got = schnorr.verify_batch_device(cv, keys, msgs, sigs)
    assert list(map(bool, got)) == want
    assert (got == schnorr.verify_batch(cv, keys, msgs, sigs)).all()
    # a larger batch: the vectors repeated, every third message changed
    rep = 50
    keys, msgs, sigs = keys * rep, [bytes([m[0] ^ (k % 3 == 2)]) + m[1:] for k, m in enumerate(msgs * rep)], sigs * rep
    got = schnorr.verify_batch_device(cv, keys, msgs, sigs)
    assert (got == schnorr.verify_batch(cv, keys, msgs, sigs)).all() and got.any() and not got.all()
    for cn in ("p256", "p384"):
        o = ctx.curve(cn)
        ok = np.zeros(1, dtype=np.uint8)
        z = np.zeros(2 * o.nb, dtype=np.uint8)
        rc = ctx.lib.ecgpu_schnorr_verify_prehash_batch(ctx.handle, o.id, _vp(z), _vp(z), _vp(z), _vp(ok), 1, 0)
        assert rc == -4                                                # ECGPU_ERR_UNSUPPORTED
    with pytest.raises(ecgpu.EcgpuError):
        ctx.curve("p256").schnorr_verify_prehash(bytes(32), bytes(64), bytes(32))


def test_argument_errors(ctx):
    ERR_ARG = -1
    rec = np.zeros((4, 16), dtype=np.uint8)
    lens = np.array([0, 16, 3, 16], dtype=np.uint32)
    assert _xmd_raw(ctx, 0, rec, 16, lens, b"dst", 32, 4)[0] == 0
    assert _xmd_raw(ctx, 0, rec, 16, lens, b"", 32, 4)[0] == ERR_ARG                       # dst_len 0
    d256 = np.zeros(256, dtype=np.uint8)
    out = np.zeros((4, 32), dtype=np.uint8)
    lib, h = ctx.lib, ctx.handle
    assert lib.ecgpu_expand_message_xmd_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 0, _vp(out), 32, 4, 0) == ERR_ARG
    assert lib.ecgpu_expand_message_xmd_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 256, _vp(out), 32, 4, 0) == ERR_ARG
    assert "255" in ctx.last_error()
    big = np.zeros((4, 255 * 48 + 1), dtype=np.uint8)
    assert lib.ecgpu_expand_message_xmd_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 5, _vp(big), 255 * 32 + 1, 4, 0) == ERR_ARG
    assert lib.ecgpu_expand_message_xmd_batch(h, 1, _vp(rec), 16, _vp(lens), _vp(d256), 5, _vp(big), 255 * 48 + 1, 4, 0) == ERR_ARG
    assert lib.ecgpu_expand_message_xmd_batch(h, 1, _vp(rec), 16, _vp(lens), _vp(d256), 5, _vp(big), 255 * 48, 4, 0) == 0
    assert lib.ecgpu_expand_message_xmd_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 5, _vp(big), 0, 4, 0) == ERR_ARG
    assert lib.ecgpu_expand_message_xmd_batch(h, 2, _vp(rec), 16, _vp(lens), _vp(d256), 5, _vp(out), 32, 4, 0) == ERR_ARG      # unknown hash
    bad = np.array([0, 17, 3, 16], dtype=np.uint32)                                                                      # msg_len[1] > msg_stride
    assert lib.ecgpu_expand_message_xmd_batch(h, 0, _vp(rec), 16, _vp(bad), _vp(d256), 5, _vp(out), 32, 4, 0) == ERR_ARG
    xy, inf = np.zeros((4, 64), dtype=np.uint8), np.zeros(4, dtype=np.uint8)
    assert lib.ecgpu_hash_to_curve_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 5, 0, _vp(xy), _vp(inf), 4, 0) == 0
    assert lib.ecgpu_hash_to_curve_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 5, 2, _vp(xy), _vp(inf), 4, 0) == ERR_ARG   # unknown mode
    assert lib.ecgpu_hash_to_curve_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 0, 0, _vp(xy), _vp(inf), 4, 0) == ERR_ARG
    assert lib.ecgpu_hash_to_curve_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 256, 0, _vp(xy), _vp(inf), 4, 0) == ERR_ARG
    assert lib.ecgpu_hash_to_curve_batch(h, 0, _vp(rec), 16, _vp(bad), _vp(d256), 5, 0, _vp(xy), _vp(inf), 4, 0) == ERR_ARG
    sc = np.zeros((4, 32), dtype=np.uint8)
    assert lib.ecgpu_hash_to_scalar_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 5, _vp(sc), 4, 0) == 0
    assert lib.ecgpu_hash_to_scalar_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 0, _vp(sc), 4, 0) == ERR_ARG
    assert lib.ecgpu_hash_to_scalar_batch(h, 0, _vp(rec), 16, _vp(lens), _vp(d256), 256, _vp(sc), 4, 0) == ERR_ARG
    assert lib.ecgpu_hash_to_scalar_batch(h, 0, _vp(rec), 16, _vp(bad), _vp(d256), 5, _vp(sc), 4, 0) == ERR_ARG
    assert lib.ecgpu_hash_to_scalar_batch(h, 7, _vp(rec), 16, _vp(lens), _vp(d256), 5, _vp(sc), 4, 0) == -4                 # unknown curve
