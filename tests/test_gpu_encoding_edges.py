"""The rows of tests/encoding_edge_vectors.py through the C ABI: ecgpu_batch_normalize, ecgpu_to_bytes_batch / ecgpu_sec1_encode_batch
and ecgpu_from_bytes_batch / ecgpu_sec1_decode_batch at the sizes that enter every loop of their kernels (full batches of 16 with
identities in every slot, two and three workgroups, full and ragged tiles with byte tails of 0 .. 3 bytes, unaligned record buffers,
a second pass of the grid-stride loops).  Every byte is compared with Python-integer arithmetic (oracle.ecmodel and the models of the
vectors module); tests/test_encoding_edge_coverage.py shows on the CPU that the rows are what they claim."""
import ctypes
import functools

import numpy as np
import pytest

import encoding_edge_vectors as V
from oracle import ecmodel as M

pytestmark = pytest.mark.gpu
CURVES = list(V.CURVES)
AFFINE, PROJECTIVE, HOST, DEVICE = 0, 1, 0, 1
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


def _arr(data: bytes, width: int) -> np.ndarray:
    return np.frombuffer(data, dtype=np.uint8).reshape(-1, width).copy()


def _first_bad_row(got, want):
    """index of the first row in which two (n, width) arrays or tensors differ, None if there is none"""
    got, want = got.reshape(len(want), -1), want.reshape(len(want), -1)
    bad = (got != want).any(1).nonzero()
    bad = bad[0] if isinstance(bad, tuple) else bad[:, 0]
    return int(bad[0]) if len(bad) else None


def _assert_rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    got, want = got.reshape(len(want), -1), want.reshape(len(want), -1)
    i = _first_bad_row(got, want)
    assert i is None, "%s: first differing row %d: got %s, want %s" % (what, i, bytes(got[i]).hex(), bytes(want[i]).hex())


# ---------------------------------------------------------------------------------------------------------------------------------
# expected values, computed once
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _normalize_case(cn, n):
    """(input X || Y || Z, expected x || y, expected infinity bytes) as read-only arrays"""
    c = M.CURVES[cn]
    nb = c.nbytes
    want = V.proj_affine(cn, n)
    out = (_arr(V.proj_bytes(cn, V.proj_rows(cn, n)), 3 * nb), _arr(b"".join(M.i2b(c, x) + M.i2b(c, y) for x, y, _ in want), 2 * nb),
           np.array([inf for _, _, inf in want], dtype=np.uint8))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _records(cn, n, compress):
    c = M.CURVES[cn]
    a = _arr(b"".join(V.sec1_encode_model(c, P, compress) for P in V.affine_rows(cn, n)), 1 + (1 if compress else 2) * c.nbytes)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _decode_case(cn, wide):
    """(records, expected x || y, expected ok) of the class matrix"""
    c = M.CURVES[cn]
    rows = V.decode_rows(cn, wide)
    want = [V.decoded_bytes(c, r.record) for r in rows]
    out = (_arr(b"".join(r.record for r in rows), len(rows[0].record)), _arr(b"".join(w[0] for w in want), 2 * c.nbytes),
           np.array([w[1] for w in want], dtype=np.uint8))
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# batch_normalize
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", V.NORMALIZE_SIZES)
@pytest.mark.parametrize("cn", CURVES)
def test_batch_normalize(ctx, cn, n):
    p, want_xy, want_inf = _normalize_case(cn, n)
    xy, inf = ctx.curve(cn).batch_normalize(p)
    _assert_rows(xy, want_xy, "%s normalize n=%d" % (cn, n))
    _assert_rows(inf, want_inf, "%s normalize n=%d: infinity" % (cn, n))
    if n >= V.IDENTITY_EVERY:
        assert 0 < int(inf.sum()) < n


@pytest.mark.parametrize("cn", CURVES)
def test_batch_normalize_without_infinity_bytes(ctx, cn):
    """out_inf = NULL through the raw entry point, on the constructed 4096-row layout"""
    p, want_xy, _ = _normalize_case(cn, 4096)
    xy = np.full(want_xy.shape, 0xA5, dtype=np.uint8)
    rc = ctx.lib.ecgpu_batch_normalize(ctx.handle, M.CURVE_IDS[cn], ctypes.c_void_p(p.ctypes.data), ctypes.c_void_p(xy.ctypes.data), None, 4096, HOST)
    assert rc == 0, ctx.last_error()
    _assert_rows(xy, want_xy, "%s normalize without out_inf" % cn)


# ---------------------------------------------------------------------------------------------------------------------------------
# to_bytes / sec1_encode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", V.ENCODE_SIZES)
@pytest.mark.parametrize("cn", CURVES)
def test_encode(ctx, cn, n):
    c = M.CURVES[cn]
    nb = c.nbytes
    # pure arithmetic, also in the coverage test: over these sizes the last tile's byte count takes every value mod 4
    assert {V.last_tile_tail(m, w) for m in V.ENCODE_SIZES for w in V.record_widths()} == {0, 1, 2, 3}
    assert all({V.last_tile_tail(m, w) for m in V.ENCODE_SIZES} == {0, 1, 2, 3} for w in (1 + nb, 1 + 2 * nb))
    cv = ctx.curve(cn)
    proj = _normalize_case(cn, 8197)[0][:n]
    aff = _arr(b"".join(V.affine_bytes(c, P) for P in V.affine_rows(cn, n)), 2 * nb)
    for pts, fmt, name in ((aff, AFFINE, "affine"), (proj, PROJECTIVE, "projective")):
        what = "%s %s n=%d " % (cn, name, n)
        _assert_rows(cv.to_bytes(pts, point_format=fmt), _records(cn, n, True), what + "to_bytes")
        _assert_rows(cv.sec1_encode(pts, compress=True, point_format=fmt), _records(cn, n, True), what + "sec1_encode compressed")
        _assert_rows(cv.sec1_encode(pts, compress=False, point_format=fmt), _records(cn, n, False), what + "sec1_encode uncompressed")


# ---------------------------------------------------------------------------------------------------------------------------------
# from_bytes / sec1_decode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [0, 1, 97])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("cn", CURVES)
def test_decode_class_matrix(ctx, cn, wide, rot):
    """the whole matrix in one batch, then rotated: a class lands on other lanes and next to other neighbours, its output goes with it"""
    cv = ctx.curve(cn)
    rows = V.rotate(V.decode_rows(cn, wide), rot)
    rec, want_xy, want_ok = (np.ascontiguousarray(np.roll(a, -rot, axis=0)) for a in _decode_case(cn, wide))
    assert bytes(rec[0]) == rows[0].record and bytes(rec[-1]) == rows[-1].record
    calls = [("sec1_decode", lambda: cv.sec1_decode(rec, record_bytes=rec.shape[1]))]
    if not wide:
        calls.append(("from_bytes", lambda: cv.from_bytes(rec)))
    for name, call in calls:
        xy, ok = call()
        bad = [(i, rows[i].cls, int(ok[i]), int(want_ok[i])) for i in range(len(rows)) if ok[i] != want_ok[i]][:10]
        assert not bad, (cn, name, wide, rot, bad)
        i = _first_bad_row(xy, want_xy)
        assert i is None, (cn, name, wide, rot, i, rows[i].cls, bytes(xy[i]).hex(), bytes(want_xy[i]).hex())
    assert 0 < int(want_ok.sum()) < len(rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# round trips
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", CURVES)
def test_round_trips(ctx, cn):
    c = M.CURVES[cn]
    nb = c.nbytes
    cv = ctx.curve(cn)
    n = V.ROUND_TRIP_N
    pts = V.affine_rows(cn, n)
    assert set(V.pool(cn)) <= set(pts) and None in pts
    aff = _arr(b"".join(V.affine_bytes(c, P) for P in pts), 2 * nb)
    for compress in (True, False):
        rec = cv.sec1_encode(aff, compress=compress)
        _assert_rows(rec, _records(cn, n, compress), "%s encode compress=%d" % (cn, compress))
        back, ok = cv.sec1_decode(rec, record_bytes=rec.shape[1])
        assert ok.tolist() == [1] * n
        _assert_rows(back, aff, "%s decode(encode(P)) compress=%d" % (cn, compress))
    # the records of the class matrix that decode and carry the tags 2, 3, 4 come back from the encoder byte for byte
    for wide in (False, True):
        rec, want_xy, want_ok = _decode_case(cn, wide)
        keep = [i for i in range(len(rec)) if want_ok[i] and rec[i][0] in (2, 3, 4)]
        assert {int(rec[i][0]) for i in keep} == ({2, 3, 4} if wide else {2, 3})
        xy, ok = cv.sec1_decode(np.ascontiguousarray(rec[keep]), record_bytes=rec.shape[1])
        assert ok.all()
        _assert_rows(xy, want_xy[keep], "%s decode of the valid matrix rows" % cn)
        for tag4 in (False, True):
            sel = [k for k, i in enumerate(keep) if (rec[i][0] == 4) == tag4]
            if sel:
                again = cv.sec1_encode(np.ascontiguousarray(xy[sel]), compress=not tag4)
                _assert_rows(again, np.ascontiguousarray(rec[keep][sel][:, :again.shape[1]]), "%s encode(decode(record)) tag4=%d" % (cn, tag4))


# ---------------------------------------------------------------------------------------------------------------------------------
# device-resident buffers: record buffers at any byte offset
# ---------------------------------------------------------------------------------------------------------------------------------
def _dptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("cn", CURVES)
def test_device_record_buffers_at_any_byte_offset(ctx, cn, off):
    """the encoders' `out` and the decoders' `in` hold byte records and may start at any address (include/ecgpu.h); the word-typed
    buffers stay aligned.  The result equals the model's and the host-memory call's, and the bytes around the output slice are untouched."""
    import torch
    c = M.CURVES[cn]
    nb, cid = c.nbytes, M.CURVE_IDS[cn]
    cv = ctx.curve(cn)
    n = V.DEVICE_N
    lib, h = ctx.lib, ctx.handle
    aff = _arr(b"".join(V.affine_bytes(c, P) for P in V.affine_rows(cn, n)), 2 * nb)
    proj = _normalize_case(cn, 8197)[0][:n]
    d_aff, d_proj = torch.from_numpy(aff).cuda(), torch.from_numpy(proj.copy()).cuda()
    for compress in (True, False):
        width = 1 + (1 if compress else 2) * nb
        want = _records(cn, n, compress)
        for d_pts, fmt, host_pts in ((d_aff, AFFINE, aff), (d_proj, PROJECTIVE, proj)):
            buf = torch.full((GUARD + off + n * width + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            out = buf[GUARD + off:GUARD + off + n * width]
            assert out.data_ptr() % 4 == off
            torch.cuda.synchronize()
            if compress:
                rc = lib.ecgpu_to_bytes_batch(h, cid, _dptr(d_pts), fmt, _dptr(out), n, DEVICE)
            else:
                rc = lib.ecgpu_sec1_encode_batch(h, cid, _dptr(d_pts), fmt, 0, _dptr(out), n, DEVICE)
            assert rc == 0, ctx.last_error()
            ctx.synchronize()
            got = buf.cpu().numpy()
            what = "%s device encode compress=%d fmt=%d off=%d" % (cn, compress, fmt, off)
            _assert_rows(got[GUARD + off:GUARD + off + n * width].reshape(n, width), want, what)
            assert (got[:GUARD + off] == 0xA5).all() and (got[GUARD + off + n * width:] == 0xA5).all(), what + ": guard bytes"
            host = cv.sec1_encode(host_pts, compress=compress, point_format=fmt)
            assert bytes(host) == bytes(got[GUARD + off:GUARD + off + n * width]), what + ": host-memory result"
    # decode from a record buffer at the same offsets: the class matrix, filled up with valid records
    for wide in (False, True):
        rec, want_xy, want_ok = _decode_case(cn, wide)
        width = rec.shape[1]
        fill = _records(cn, n, not wide)
        recs = np.concatenate([rec, fill[:n - len(rec)]])
        want_xy = np.concatenate([want_xy, aff[:n - len(rec)]])
        want_ok = np.concatenate([want_ok, np.ones(n - len(rec), dtype=np.uint8)])
        buf = torch.zeros(GUARD + off + n * width + GUARD, dtype=torch.uint8, device="cuda")
        src = buf[GUARD + off:GUARD + off + n * width]
        src.copy_(torch.from_numpy(recs.reshape(-1)))
        d_xy = torch.full((n, 2 * nb), 0xA5, dtype=torch.uint8, device="cuda")
        d_ok = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        assert src.data_ptr() % 4 == off
        torch.cuda.synchronize()
        if wide:
            rc = lib.ecgpu_sec1_decode_batch(h, cid, _dptr(src), width, _dptr(d_xy), _dptr(d_ok), n, DEVICE)
        else:
            rc = lib.ecgpu_from_bytes_batch(h, cid, _dptr(src), _dptr(d_xy), _dptr(d_ok), n, DEVICE)
        assert rc == 0, ctx.last_error()
        ctx.synchronize()
        what = "%s device decode wide=%d off=%d" % (cn, wide, off)
        _assert_rows(d_xy.cpu().numpy(), want_xy, what)
        _assert_rows(d_ok.cpu().numpy(), want_ok, what + ": ok")
        h_xy, h_ok = cv.sec1_decode(recs, record_bytes=width)
        assert bytes(h_xy) == bytes(d_xy.cpu().numpy()) and bytes(h_ok) == bytes(d_ok.cpu().numpy()), what + ": host-memory result"


# ---------------------------------------------------------------------------------------------------------------------------------
# the loops whose trip count depends on the device
# ---------------------------------------------------------------------------------------------------------------------------------
def _tile(pool_rows: np.ndarray, n: int):
    """(n, width) device tensor: row i is row i mod len(pool_rows) of the pool"""
    import torch
    d_pool = torch.from_numpy(np.array(pool_rows)).cuda()
    idx = torch.arange(n, device="cuda") % len(pool_rows)
    return torch.index_select(d_pool.reshape(len(pool_rows), -1), 0, idx).contiguous()


def _assert_device_rows(got, want, what):
    import torch
    if not torch.equal(got, want):
        i = _first_bad_row(got, want)
        raise AssertionError("%s: first differing row %d (pool row %d): got %s, want %s" % (
            what, i, i % V.DEVICE_POOL, bytes(got[i].reshape(-1).cpu().numpy()).hex(), bytes(want[i].reshape(-1).cpu().numpy()).hex()))


@pytest.mark.parametrize("cn", ["k256", "p384"])
def test_encode_and_decode_enter_a_second_grid_stride_pass(ctx, cn):
    """n = 8 cus 256 + 256 + 3, uncompressed: the grid of 8 cus workgroups takes its tiles, two of them a second one, the last tile has
    three records.  The rows are a pool of 4099 tiled on the device; the expected values are the model's for the pool, tiled the same way."""
    import torch
    c = M.CURVES[cn]
    nb, cid = c.nbytes, M.CURVE_IDS[cn]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = V.encode_pass_rows(cus)
    g = V.geometry(n, cus)
    assert g.grid == 8 * cus and g.tile_passes == 2 and n % 256 == 3
    width = 1 + 2 * nb
    pool_pts = V.affine_rows(cn, V.DEVICE_POOL)
    d_aff = _tile(_arr(b"".join(V.affine_bytes(c, P) for P in pool_pts), 2 * nb), n)
    want = _tile(_arr(b"".join(V.sec1_encode_model(c, P, False) for P in pool_pts), width), n)
    d_out = torch.full((n, width), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.ecgpu_sec1_encode_batch(ctx.handle, cid, _dptr(d_aff), AFFINE, 0, _dptr(d_out), n, DEVICE)
    assert rc == 0, ctx.last_error()
    ctx.synchronize()
    _assert_device_rows(d_out, want, "%s encode n=%d" % (cn, n))
    recs = V.device_decode_pool(cn)
    dec = [V.decoded_bytes(c, r) for r in recs]
    d_rec = _tile(_arr(b"".join(recs), width), n)
    want_xy = _tile(_arr(b"".join(d[0] for d in dec), 2 * nb), n)
    want_ok = _tile(np.array([d[1] for d in dec], dtype=np.uint8).reshape(-1, 1), n)
    d_xy = torch.full((n, 2 * nb), 0xA5, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n, 1), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.ecgpu_sec1_decode_batch(ctx.handle, cid, _dptr(d_rec), width, _dptr(d_xy), _dptr(d_ok), n, DEVICE)
    assert rc == 0, ctx.last_error()
    ctx.synchronize()
    _assert_device_rows(d_xy, want_xy, "%s decode n=%d" % (cn, n))
    _assert_device_rows(d_ok, want_ok, "%s decode n=%d: ok" % (cn, n))
    assert 0 < int(want_ok.sum()) < n


def test_batch_normalize_enters_a_second_pass(ctx):
    """n = 8 cus 256 16 + 3 256 + 5 on secp256k1 (the loop does not depend on the curve), device-resident: every lane of the largest grid
    normalises a full batch of 16, then the lanes 0 .. 772 come round for a ragged second one of a single row.  About 8.4 M rows and
    1.35 GB at 256 compute units, tiled on the device from 4099 rows with identities of both forms every 37."""
    import torch
    cn = "k256"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = V.normalize_pass_rows(cus)
    g = V.geometry(n, cus)
    assert g.blocks == 8 * cus and g.passes == 2 and n - 16 * g.T == 773
    p, xy, inf = (a[:V.DEVICE_POOL] for a in _normalize_case(cn, 8197))
    d_p, want_xy, want_inf = _tile(p, n), _tile(xy, n), _tile(inf.reshape(-1, 1), n)
    d_xy = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((n, 1), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.curve(cn).batch_normalize_device(d_p, d_xy, d_inf, n)
    ctx.synchronize()
    _assert_device_rows(d_xy, want_xy, "normalize n=%d" % n)
    _assert_device_rows(d_inf, want_inf, "normalize n=%d: infinity" % n)
    assert 0 < int(want_inf.sum()) < n
    del d_p, d_xy, d_inf, want_xy, want_inf
    torch.cuda.empty_cache()
