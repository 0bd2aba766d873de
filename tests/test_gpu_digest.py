"""ecgpu_digest_batch (include/ecgpu.h, "from message bytes") on the GPU against hashlib: SHA-256 and SHA-384 of whole messages, one
message per lane, whole blocks of a 4-byte aligned record read by words (csrc/sha2.hpp update_aligned) and everything else by
bytes.  The every-length sweeps put the block and padding boundaries (55/56/63/64/65, 111/112/127/128/129) on both paths."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HASHES = {0: "sha256", 1: "sha384"}
DB = {0: 32, 1: 48}
ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sweep():
    """the 301 messages of length 0 .. 300 and their digests, computed once"""
    rng = random.Random(0xD16E57)
    msgs = [rng.randbytes(k) for k in range(301)]
    return msgs, {h: b"".join(hashlib.new(HASHES[h], m).digest() for m in msgs) for h in HASHES}


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


@pytest.mark.parametrize("h", [0, 1])
@pytest.mark.parametrize("mem", [0, 1])
def test_every_length_in_aligned_records(ctx, sweep, h, mem):
    msgs, want = sweep
    rec, lens = _records(msgs, 304)
    rc, out = _digest(ctx, h, rec, 304, lens, 301, mem)
    assert rc == 0, ctx.last_error()
    assert out.tobytes() == want[h]


@pytest.mark.parametrize("h", [0, 1])
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_length_on_all_four_alignments(ctx, sweep, h, lead):
    """stride 301: record i starts i mod 4 bytes (plus the lead) off a word boundary, so every length meets both paths"""
    msgs, want = sweep
    rec, lens = _records(msgs, 301, lead)
    for mem in (1, 0):
        rc, out = _digest(ctx, h, rec, 301, lens, 301, mem, lead)
        assert rc == 0, ctx.last_error()
        assert out.tobytes() == want[h], (mem, lead)


@pytest.mark.parametrize("h", [0, 1])
def test_uniform_batches(ctx, h):
    rng = random.Random(0x51 + h)
    n = 70
    for stride in (0, 64, 128, 133):
        rec = np.frombuffer(rng.randbytes(n * stride), dtype=np.uint8).copy()
        want = b"".join(hashlib.new(HASHES[h], rec[k * stride:(k + 1) * stride].tobytes()).digest() for k in range(n))
        for mem in (0, 1):
            rc, out = _digest(ctx, h, rec, stride, None, n, mem)
            assert rc == 0, ctx.last_error()
            assert out.tobytes() == want, (stride, mem)


@pytest.mark.parametrize("h", [0, 1])
def test_more_messages_than_lanes(ctx, h):
    """200 003 messages of 5 .. 70 bytes: the grid-stride loop"""
    n, stride = 200003, 72
    rng = np.random.default_rng(0xabc + h)
    rec = rng.integers(0, 256, size=n * stride, dtype=np.uint8)
    lens = (5 + np.arange(n) % 66).astype(np.uint32)
    rc, out = _digest(ctx, h, rec, stride, lens, n, 0)
    assert rc == 0, ctx.last_error()
    raw = rec.tobytes()
    new = hashlib.sha384 if h else hashlib.sha256
    assert out.tobytes() == b"".join(new(raw[stride * k:stride * k + int(lens[k])]).digest() for k in range(n))


@pytest.mark.parametrize("h", [0, 1])
@pytest.mark.parametrize("stride", [10000, 10001])
def test_one_long_message_among_short_ones(ctx, h, stride):
    rng = random.Random(0x10000 + h)
    msgs = [rng.randbytes(k) for k in (3, 64, 10000, 0, 129, 700, 1)]
    rec, lens = _records(msgs, stride)
    for mem in (0, 1):
        rc, out = _digest(ctx, h, rec, stride, lens, len(msgs), mem)
        assert rc == 0, ctx.last_error()
        assert out.tobytes() == b"".join(hashlib.new(HASHES[h], m).digest() for m in msgs), mem


def test_python_wrappers(ctx):
    import ecgpu
    rng = random.Random(7)
    msgs = [rng.randbytes(k) for k in (0, 1, 63, 64, 65, 200)]
    for h in (0, 1):
        assert ecgpu.digest(ctx, h, msgs).tobytes() == b"".join(hashlib.new(HASHES[h], m).digest() for m in msgs)
    assert ecgpu.digest(ctx, 0, []).shape == (0, 32)
    assert ctx.curve("p384").digest(msgs).tobytes() == b"".join(hashlib.sha384(m).digest() for m in msgs)
    assert ctx.curve("k256").digest([b"", b""]).tobytes() == 2 * hashlib.sha256(b"").digest()


def test_refusals(ctx):
    rec = np.zeros(4 * 16, dtype=np.uint8)
    lens = np.array([1, 16, 17, 0], dtype=np.uint32)
    out = np.zeros((4, 48), dtype=np.uint8)
    call = ctx.lib.ecgpu_digest_batch
    rp, lp, op = ctypes.c_void_p(rec.ctypes.data), ctypes.c_void_p(lens.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert call(ctx.handle, 2, rp, 16, lp, op, 2, 0) == ERR_ARG and "unknown hash" in ctx.last_error()
    assert call(ctx.handle, 0, rp, 16, lp, None, 2, 0) == ERR_ARG
    assert call(ctx.handle, 0, None, 16, lp, op, 2, 0) == ERR_ARG
    assert call(ctx.handle, 0, rp, 16, lp, op, 4, 0) == ERR_ARG and "msg_len[2] = 17" in ctx.last_error()
    assert call(ctx.handle, 0, rp, 1 << 32, None, op, 0, 0) == ERR_ARG
    assert not out.any()
    assert call(ctx.handle, 0, rp, 16, lp, op, 0, 0) == 0                 # n = 0: nothing to do
    assert call(ctx.handle, 1, None, 0, None, op, 0, 0) == 0
    assert call(ctx.handle, 0, rp, 16, lp, op, 2, 0) == 0
    assert out.tobytes()[:64] == hashlib.sha256(b"\0").digest() + hashlib.sha256(bytes(16)).digest()
    # device-resident digests are rows of words
    import torch
    t = torch.zeros(128, dtype=torch.uint8, device="cuda")
    assert call(ctx.handle, 0, None, 0, None, ctypes.c_void_p(t.data_ptr() + 1), 2, 1) == ERR_ARG
