"""ecgpu_digest_batch on the sponge ids (include/ecgpu.h: ECGPU_KECCAK256 = 16, ECGPU_SHA3_256 = 17, ECGPU_SHA3_384 = 18; csrc/keccak.hpp)
on the GPU: SHA3-256 and SHA3-384 against hashlib, Keccak-256 against tests/keccak_model.py (pinned by tests/test_keccak_model.py).
One message per lane, whole blocks of a 4-byte aligned record read by words and everything else by bytes.  The every-length sweeps
put the block and padding boundaries (134/135/136/137, 271/272/273; 102/103/104/105, 207/208/209) on both paths, among them the
lengths rate - 1 mod rate where the domain byte and the final 0x80 share a byte."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import keccak_model as K
from conftest import GOLDEN
from oracle import ecmodel as M

pytestmark = pytest.mark.gpu

HASHES = {16: "keccak256", 17: "sha3_256", 18: "sha3_384"}
DB = {16: 32, 17: 32, 18: 48}
ERR_ARG = -1


def _want(h, msg):
    return K.digest(h, msg) if h == 16 else hashlib.new(HASHES[h], msg).digest()


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sweep():
    """the 301 messages of length 0 .. 300 and their digests, computed once"""
    rng = random.Random(0xCECCAC)
    msgs = [rng.randbytes(k) for k in range(301)]
    return msgs, {h: b"".join(_want(h, m) for m in msgs) for h in HASHES}


def _records(msgs, stride, lead=0):
    """records of `stride` bytes with 0xA5 behind each message, `lead` bytes into a larger array of 0xA5 -> (view, lengths)"""
    big = np.full(lead + len(msgs) * stride + 8, 0xA5, dtype=np.uint8)
    for k, m in enumerate(msgs):
        big[lead + k * stride:lead + k * stride + len(m)] = np.frombuffer(m, dtype=np.uint8)
    return big[lead:lead + len(msgs) * stride], np.array([len(m) for m in msgs], dtype=np.uint32)


def _digest(ctx, h, rec, stride, lens, n, mem, lead=0):
    """the C call -> (rc, digests).  mem = 1: the buffers are torch tensors, the records `lead` bytes into their allocation"""
    out = np.zeros((n, DB.get(h, 48)), dtype=np.uint8)
    if mem == 0:
        rc = ctx.lib.ecgpu_digest_batch(ctx.handle, h, ctypes.c_void_p(rec.ctypes.data) if rec is not None and rec.size else None, stride,
                                        ctypes.c_void_p(lens.ctypes.data) if lens is not None else None, ctypes.c_void_p(out.ctypes.data), n, 0)
        return rc, out
    import torch
    t_rec = None
    if rec is not None and rec.size:
        t_big = torch.full((lead + rec.size,), 0xA5, dtype=torch.uint8, device="cuda")
        t_big[lead:] = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
        t_rec = t_big[lead:]
        assert t_rec.data_ptr() % 4 == (t_big.data_ptr() + lead) % 4 and t_big.data_ptr() % 16 == 0
    t_len = torch.from_numpy(lens.view(np.int32)).cuda() if lens is not None else None
    t_out = torch.zeros(out.shape, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.ecgpu_digest_batch(ctx.handle, h, ctypes.c_void_p(t_rec.data_ptr()) if t_rec is not None else None, stride,
                                    ctypes.c_void_p(t_len.data_ptr()) if t_len is not None else None, ctypes.c_void_p(t_out.data_ptr()), n, 1)
    ctx.synchronize()
    return rc, t_out.cpu().numpy()


def _first_difference(out, want, width):
    got = out.tobytes()
    return next((k for k in range(len(want) // width) if got[k * width:(k + 1) * width] != want[k * width:(k + 1) * width]), None)


@pytest.mark.parametrize("h", [16, 17, 18])
@pytest.mark.parametrize("mem", [0, 1])
def test_every_length_in_aligned_records(ctx, sweep, h, mem):
    msgs, want = sweep
    rec, lens = _records(msgs, 304)
    rc, out = _digest(ctx, h, rec, 304, lens, 301, mem)
    assert rc == 0, ctx.last_error()
    assert out.tobytes() == want[h], _first_difference(out, want[h], DB[h])


@pytest.mark.parametrize("h", [16, 17, 18])
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_length_on_all_four_alignments(ctx, sweep, h, lead):
    """stride 301: record i starts i mod 4 bytes (plus the lead) off a word boundary, so every length meets both paths"""
    msgs, want = sweep
    rec, lens = _records(msgs, 301, lead)
    for mem in (1, 0):
        rc, out = _digest(ctx, h, rec, 301, lens, 301, mem, lead)
        assert rc == 0, ctx.last_error()
        assert out.tobytes() == want[h], (mem, lead, _first_difference(out, want[h], DB[h]))


@pytest.mark.parametrize("h", [16, 17, 18])
def test_uniform_batches(ctx, h):
    rng = random.Random(0x51 + h)
    n = 70
    for stride in (0, 135, 136, 137, 272):
        rec = np.frombuffer(rng.randbytes(n * stride), dtype=np.uint8).copy()
        want = b"".join(_want(h, rec[k * stride:(k + 1) * stride].tobytes()) for k in range(n))
        for mem in (0, 1):
            rc, out = _digest(ctx, h, rec, stride, None, n, mem)
            assert rc == 0, ctx.last_error()
            assert out.tobytes() == want, (stride, mem)


@pytest.mark.parametrize("h", [16, 17, 18])
def test_more_messages_than_lanes(ctx, h):
    """200 003 messages of 5 .. 70 bytes: the grid-stride loop.  Contents and lengths repeat with period 66, so the 66 digests the
    model (Keccak-256) or hashlib computes are the whole expectation, tiled"""
    n, stride, period = 200003, 72, 66
    rng = np.random.default_rng(0xabc + h)
    base = rng.integers(0, 256, size=(period, stride), dtype=np.uint8)
    rec = np.ascontiguousarray(np.tile(base, (n // period + 1, 1))[:n]).reshape(-1)
    lens = (5 + np.arange(n) % period).astype(np.uint32)
    rc, out = _digest(ctx, h, rec, stride, lens, n, 0)
    assert rc == 0, ctx.last_error()
    one = [_want(h, base[k, :5 + k].tobytes()) for k in range(period)]
    want = (b"".join(one) * (n // period + 1))[:n * DB[h]]
    assert out.tobytes() == want, _first_difference(out, want, DB[h])


_LONG = {}


def _long(h):
    if h not in _LONG:
        rng = random.Random(0x10000 + h)
        msgs = [rng.randbytes(k) for k in (3, 136, 10000, 0, 273, 700, 1)]
        _LONG[h] = (msgs, b"".join(_want(h, m) for m in msgs))
    return _LONG[h]


@pytest.mark.parametrize("h", [16, 17, 18])
@pytest.mark.parametrize("stride", [10000, 10001])
def test_one_long_message_among_short_ones(ctx, h, stride):
    msgs, want = _long(h)
    rec, lens = _records(msgs, stride)
    for mem in (0, 1):
        rc, out = _digest(ctx, h, rec, stride, lens, len(msgs), mem)
        assert rc == 0, ctx.last_error()
        assert out.tobytes() == want, mem


def test_python_wrappers(ctx):
    import ecgpu
    assert (ecgpu.KECCAK256, ecgpu.SHA3_256, ecgpu.SHA3_384) == (16, 17, 18)
    assert [ctx.lib.ecgpu_hash_bytes(h) for h in (0, 1, 2, 15, 16, 17, 18, 19)] == [32, 48, 0, 0, 32, 32, 48, 0]
    rng = random.Random(7)
    msgs = [rng.randbytes(k) for k in (0, 1, 135, 136, 137, 200)]
    for h in (16, 17, 18):
        assert ecgpu.digest(ctx, h, msgs).tobytes() == b"".join(_want(h, m) for m in msgs)
        assert ecgpu.digest(ctx, h, []).shape == (0, DB[h]) and ecgpu.DIGEST_BYTES[h] == DB[h]
    assert ecgpu.digest(ctx, ecgpu.KECCAK256, [b"", b"abc"]).tobytes().hex() == (
        "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470" "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45")
    import torch
    rec, lens = _records(msgs, 200)
    t_out = torch.zeros((len(msgs), 32), dtype=torch.uint8, device="cuda")
    ecgpu.digest_device(ctx, ecgpu.SHA3_256, torch.from_numpy(rec.copy()).cuda(), 200, torch.from_numpy(lens.view(np.int32)).cuda(), t_out, len(msgs))
    ctx.synchronize()
    assert t_out.cpu().numpy().tobytes() == b"".join(hashlib.sha3_256(m).digest() for m in msgs)


def test_eth_addresses(ctx):
    """Keccak-256 over the 64-byte x || y records (stride 64, 4-byte aligned), last 20 bytes: the fixture's key
    (k256/src/ecdsa.rs:312-342) and 70 random keys against the model"""
    from ecgpu import ecdsa as E
    with open(os.path.join(GOLDEN, "keccak_ecdsa.json")) as f:
        fx = json.load(f)["sign"]
    c, cv = M.K256, ctx.curve("k256")
    rng = random.Random(0xE7)
    keys = [bytes.fromhex(fx["secret_key"])] + [rng.randrange(1, c.n).to_bytes(32, "big") for _ in range(70)]
    pub, inf = cv.mul_by_generator(b"".join(keys))
    assert not inf.any()
    got = E.eth_addresses(ctx, pub)
    assert got.shape == (71, 20) and bytes(got[0]).hex() == fx["address"]
    assert got.tobytes() == b"".join(K.eth_address(bytes(q)) for q in pub)
    assert E.eth_addresses(ctx, np.zeros((0, 64), dtype=np.uint8)).shape == (0, 20)


def test_refusals(ctx):
    rec = np.zeros(4 * 16, dtype=np.uint8)
    lens = np.array([1, 16, 17, 0], dtype=np.uint32)
    out = np.zeros((4, 48), dtype=np.uint8)
    call = ctx.lib.ecgpu_digest_batch
    rp, lp, op = ctypes.c_void_p(rec.ctypes.data), ctypes.c_void_p(lens.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    for h in (2, 15, 19):
        assert call(ctx.handle, h, rp, 16, lp, op, 2, 0) == ERR_ARG and "unknown hash %d" % h in ctx.last_error()
    for h in (16, 17, 18):
        assert call(ctx.handle, h, rp, 16, lp, None, 2, 0) == ERR_ARG
        assert call(ctx.handle, h, None, 16, lp, op, 2, 0) == ERR_ARG
        assert call(ctx.handle, h, rp, 16, lp, op, 4, 0) == ERR_ARG and "msg_len[2] = 17" in ctx.last_error()
        assert call(ctx.handle, h, rp, 1 << 32, None, op, 0, 0) == ERR_ARG
        assert not out.any()
        assert call(ctx.handle, h, rp, 16, lp, op, 0, 0) == 0                 # n = 0: nothing to do
    assert call(ctx.handle, 17, rp, 16, lp, op, 2, 0) == 0
    assert out.tobytes()[:64] == hashlib.sha3_256(b"\0").digest() + hashlib.sha3_256(bytes(16)).digest()
    # device-resident digests are rows of words
    import torch
    t = torch.zeros(128, dtype=torch.uint8, device="cuda")
    for h in (16, 18):
        assert call(ctx.handle, h, None, 0, None, ctypes.c_void_p(t.data_ptr() + 1), 2, 1) == ERR_ARG and "4-byte aligned" in ctx.last_error()
    # XMD is the Merkle-Damgard expander: the sponge ids stay refused
    dst = np.frombuffer(b"QUUX-V01-CS02", dtype=np.uint8).copy()
    okm = np.zeros((2, 32), dtype=np.uint8)
    assert ctx.lib.ecgpu_expand_message_xmd_batch(ctx.handle, 16, rp, 16, lp, ctypes.c_void_p(dst.ctypes.data), len(dst), ctypes.c_void_p(okm.ctypes.data), 32, 2, 0) == ERR_ARG
    assert "unknown hash 16" in ctx.last_error() and not okm.any()
