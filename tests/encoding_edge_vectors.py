"""Points as bytes at the edges of the three kernels behind ecgpu_batch_normalize, ecgpu_to_bytes_batch / ecgpu_sec1_encode_batch and
ecgpu_from_bytes_batch / ecgpu_sec1_decode_batch.  Pure Python on oracle.ecmodel; every expected value is Python-integer arithmetic.

Layout rules restated here (layout(n, cus)):
  normalize_kernel<C, 16>   csrc/kernels.hpp:138-180, launched at csrc/curve_ops.hpp:66 with
                            blocks = min(ceil(ceil(n / 16) / 256), 8 cus) (csrc/ecgpu_internal.hpp:139-145), T = 256 blocks lanes.
                            A pass covers 16 T rows (the `base += T * BATCH` loop, kernels.hpp:145); inside pass q lane l holds the rows
                            16 T q + l + T s in its slots s = 0 .. 15 and shares ONE inversion among them: prefix products forwards,
                            a zero Z replaced by one, unwound backwards (kernels.hpp:149-178).
  sec1::to_bytes_kernel     csrc/sec1_kernels.hpp:16-49, launched at csrc/curve_ops.hpp:351 with min(ceil(n / 256), 8 cus) workgroups.
                            Tile t = rows 256 t .. 256 t + 255, laid out in LDS and copied out as dwords plus a byte tail of
                            (records of the tile x record bytes) & 3 bytes (sec1_kernels.hpp:42-43), or byte by byte when the
                            destination is not 4-byte aligned (:45); workgroup g takes the tiles g, g + grid, .. (:20).
  sec1::from_bytes_kernel   csrc/sec1_kernels.hpp:56-109: one record per lane; sec1_decode_model is its model, written from
                            include/ecgpu.h:318-324 and the reference's from_encoded_point (k256 affine.rs:241-270, primeorder
                            affine.rs:164-195; compact: k256 affine.rs:207-211 the even root, primeorder affine.rs:66-77, 157-159
                            the numerically smaller root).

Rows
  pool(cn)            64 multiples of G, the two points of the smallest x >= 1 with a root (leading zero bytes in x), and on
                      P-256 / P-384 the two points with x = 0 (a tagged record with a zero x, NOT the identity; secp256k1 has none:
                      7 is not a square).
  proj_rows(cn, n)    the pool cycled with a stride coprime to 256 and to its length, Z of the classes 1, 2, p - 1, random; every
                      37th row an identity, alternately (0 : 1 : 0) and (X : Y : 0) with random non-zero X, Y.
  normalize_4096(cn)  n = 4096 is one workgroup whose every lane holds 16 rows: SPECIAL names the lanes built on purpose.
  decode_rows(cn, wide)  the tag x x-class matrix (TAGS, X_CLASSES, UNCOMPRESSED_CLASSES, TAIL_POSITIONS).  Near misses: x = p + x0 with x0 the smallest x >= 1 that has
                      a root (on the NIST curves x = p itself is one as well, x0 = 0), so "reduces, then checks the curve" would
                      accept what "checks canonical" rejects.  y >= p on secp256k1 is p + y0 with (x, y0) on the curve (y0 = 1, x a
                      cube root of y0^2 - 7: p = 7 mod 9, so a^((p + 2) / 9)); on the NIST curves 2^(8 NB) - p is far above any
                      y we can construct, the row is y = p + 1 and does NOT separate "reduce, then check" from "check canonical"."""
import functools
import json
import math
import os
import random
from collections import namedtuple

from oracle import ecmodel as M

CURVES = ("k256", "p256", "p384")
BATCH, LANES, TILE = 16, 256, 256

Geometry = namedtuple("Geometry", "blocks T passes tiles grid tile_passes")
Layout = namedtuple("Layout", "geo norm enc")


def geometry(n, cus):
    """grids and loop counts of the two kernels for an n-row batch on a device with `cus` compute units"""
    units = -(-n // BATCH)
    blocks = max(1, min(-(-units // LANES), 8 * cus))
    T = LANES * blocks
    tiles = -(-n // TILE)
    grid = max(1, min(tiles, 8 * cus))
    return Geometry(blocks, T, -(-n // (T * BATCH)), tiles, grid, -(-tiles // grid))


def norm_place(i, T):
    """(pass, lane, slot) of row i in normalize_kernel"""
    return i // (T * BATCH), i % (T * BATCH) % T, i % (T * BATCH) // T


def layout(n, cus):
    """norm[i] = (lane, slot) of row i in normalize_kernel (in pass i // (16 T)), enc[i] = (tile, record) in to_bytes_kernel"""
    geo = geometry(n, cus)
    return Layout(geo, [norm_place(i, geo.T)[1:] for i in range(n)], [(i // TILE, i % TILE) for i in range(n)])


def last_tile_tail(n, record_bytes):
    """bytes & 3 of the last tile of an n-row encode"""
    return ((n - 1) % TILE + 1) * record_bytes & 3


NORMALIZE_SIZES = (1, 255, 256, 257, 4089, 4096, 4097, 8197)
ENCODE_SIZES = (1, 2, 3, 255, 256, 257, 511, 513, 771)
ROUND_TRIP_N = 771
DEVICE_N = 513
DEVICE_POOL = 4099


def record_widths():
    return sorted({1 + k * M.CURVES[cn].nbytes for cn in CURVES for k in (1, 2)})       # 33, 49, 65, 97


def normalize_pass_rows(cus):
    """one full pass of normalize_kernel at its largest grid, three more workgroup-widths of rows and five"""
    return 8 * cus * LANES * BATCH + 3 * LANES + 5


def encode_pass_rows(cus):
    """one full grid of tiles, one more tile and three records"""
    return 8 * cus * TILE + TILE + 3


# ---------------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------------
def sec1_decode_model(c, record: bytes):
    """(ok, point | None) of one record of 1 + NB or 1 + 2 NB bytes; ok = False goes with zero output"""
    nb = c.nbytes
    wide = len(record) == 1 + 2 * nb
    assert wide or len(record) == 1 + nb
    tag, x, tail = record[0], M.b2i(record[1:1 + nb]), record[1 + nb:]
    if tag == 4:
        if not wide:
            return False, None
        y = M.b2i(tail)
        good = x < c.p and y < c.p and (y * y - (x * x * x + c.a * x + c.b)) % c.p == 0
        return (True, (x, y)) if good else (False, None)
    if tag in (2, 3, 5):
        if any(tail):
            return False, None
        P = M.decompress(c, x, 1 if tag == 3 else 0)
        if P is None:
            return False, None
        if tag == 5 and c.name != "k256":
            P = (P[0], min(P[1], c.p - P[1]))
        return True, P
    if tag == 0 and not any(record[1:]):
        return True, None
    return False, None


def sec1_encode_model(c, P, compress: bool) -> bytes:
    """ToEncodedPoint in fixed-width records; P = (x, y) or None"""
    if compress:
        return M.group_to_bytes(c, P)
    if P is None:
        return bytes(1 + 2 * c.nbytes)
    return b"\x04" + M.i2b(c, P[0]) + M.i2b(c, P[1])


def affine_bytes(c, P) -> bytes:
    return bytes(2 * c.nbytes) if P is None else M.i2b(c, P[0]) + M.i2b(c, P[1])


def decoded_bytes(c, record: bytes):
    """(out_xy bytes, ok byte) the decoders must produce for a record"""
    ok, P = sec1_decode_model(c, record)
    return affine_bytes(c, P if ok else None), 1 if ok else 0


# ---------------------------------------------------------------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------------------------------------------------------------
def smallest_x_with_root(c, start=1):
    return next(x for x in range(start, 1000) if M.decompress(c, x, 0) is not None)


@functools.lru_cache(maxsize=None)
def pool(cn):
    c = M.CURVES[cn]
    G = (c.gx, c.gy)
    pts, P = [], None
    for _ in range(64):
        P = M.affine_add(c, P, G)
        pts.append(P)
    x1 = smallest_x_with_root(c)
    pts += [M.decompress(c, x1, 0), M.decompress(c, x1, 1)]
    if M.decompress(c, 0, 0) is not None:
        pts += [M.decompress(c, 0, 0), M.decompress(c, 0, 1)]
    assert all(M.on_curve(c, P) for P in pts) and len(set(pts)) == len(pts)
    return tuple(pts)


def even_root_is_larger(c, P):
    """the even one of y, p - y is the larger: 'even' (tag 2, secp256k1's compact rule) and 'smaller' (the NIST compact rule) differ"""
    even = P[1] if P[1] % 2 == 0 else c.p - P[1]
    return even > c.p - even


Z_CLASSES = ("one", "two", "p_minus_1", "random")
IDENTITY_FORMS = ("canonical", "xy0")
ProjRow = namedtuple("ProjRow", "zcls xyz")          # zcls: a Z class, or an identity form


def _proj(c, rng, P, zcls):
    z = {"one": 1, "two": 2, "p_minus_1": c.p - 1}.get(zcls) or rng.randrange(3, c.p - 1)
    return ProjRow(zcls, (P[0] * z % c.p, P[1] * z % c.p, z))


def _identity(c, rng, form):
    return ProjRow(form, (0, 1, 0) if form == "canonical" else (rng.randrange(1, c.p), rng.randrange(1, c.p), 0))


POOL_STRIDE = 29
IDENTITY_EVERY = 37


@functools.lru_cache(maxsize=None)
def _proj_rows_all(cn):
    c = M.CURVES[cn]
    pts = pool(cn)
    assert math.gcd(POOL_STRIDE, 256) == 1 and math.gcd(POOL_STRIDE, len(pts)) == 1
    rng = random.Random("encoding-edges-proj-" + cn)
    rows = []
    for i in range(max(NORMALIZE_SIZES)):
        if i % IDENTITY_EVERY == IDENTITY_EVERY - 1:
            rows.append(_identity(c, rng, IDENTITY_FORMS[(i // IDENTITY_EVERY) % 2]))
        else:
            rows.append(_proj(c, rng, pts[i * POOL_STRIDE % len(pts)], Z_CLASSES[rng.randrange(4)]))
    return tuple(rows)


# the lanes of the 4096-row batch built on purpose: lane l < 16 has its one identity in slot l
SPECIAL = {"all_identity": 70, "only_slot0_finite": 133, "only_slot15_finite": 200, "alternating": 97, "alternating_odd": 255}


def normalize_4096_is_identity(lane, slot):
    if lane < 16:
        return slot == lane
    if lane == SPECIAL["all_identity"]:
        return True
    if lane == SPECIAL["only_slot0_finite"]:
        return slot != 0
    if lane == SPECIAL["only_slot15_finite"]:
        return slot != 15
    if lane == SPECIAL["alternating"]:
        return slot % 2 == 0
    if lane == SPECIAL["alternating_odd"]:
        return slot % 2 == 1
    return False


@functools.lru_cache(maxsize=None)
def normalize_4096(cn):
    c = M.CURVES[cn]
    pts = pool(cn)
    rng = random.Random("encoding-edges-4096-" + cn)
    rows = []
    for i in range(4096):
        lane, slot = i % 256, i // 256
        if normalize_4096_is_identity(lane, slot):
            rows.append(_identity(c, rng, IDENTITY_FORMS[(lane + slot) % 2]))
        else:
            rows.append(_proj(c, rng, pts[i * POOL_STRIDE % len(pts)], Z_CLASSES[(lane // 16 + slot) % 4]))
    return tuple(rows)


def proj_rows(cn, n):
    """the projective rows of an n-row batch: the constructed layout at 4096, a prefix of one cycled list otherwise"""
    return normalize_4096(cn) if n == 4096 else _proj_rows_all(cn)[:n]


@functools.lru_cache(maxsize=None)
def _affine_all(cn):
    c = M.CURVES[cn]
    return tuple(M.to_affine(c, r.xyz) for r in _proj_rows_all(cn))


@functools.lru_cache(maxsize=None)
def _affine_4096(cn):
    c = M.CURVES[cn]
    return tuple(M.to_affine(c, r.xyz) for r in normalize_4096(cn))


def proj_affine(cn, n):
    """M.to_affine of proj_rows(cn, n): (x, y, infinity) per row, computed once"""
    return _affine_4096(cn) if n == 4096 else _affine_all(cn)[:n]


def proj_bytes(cn, rows) -> bytes:
    c = M.CURVES[cn]
    return b"".join(M.proj_bytes(c, r.xyz) for r in rows)


def affine_rows(cn, n):
    """affine input of an n-row encode: the points of proj_rows, None for the identity"""
    return [None if inf else (x, y) for x, y, inf in proj_affine(cn, n)]


# ---------------------------------------------------------------------------------------------------------------------------------
# decode rows
# ---------------------------------------------------------------------------------------------------------------------------------
DecRow = namedtuple("DecRow", "cls record")
X_CLASSES = ("valid", "no_root", "p_minus_1", "p", "p_plus_x0", "all_ones")
TAGS = (0, 1, 2, 3, 4, 5, 6, 7, 0x82, 0xFF)
UNCOMPRESSED_CLASSES = ("xy", "x_negy", "y_plus_1", "y_minus_1", "p_plus_x0_y", "y_ge_p")
TAIL_POSITIONS = ("first", "middle", "last")


def x_of_class(c, xcls):
    top = 1 << (8 * c.nbytes)
    if xcls == "valid":
        return pool(c.name)[10][0]
    if xcls == "no_root":
        return next(x for x in range(1, 1000) if M.decompress(c, x, 0) is None)
    if xcls == "p_plus_x0":
        x = c.p + smallest_x_with_root(c)
        assert x < top
        return x
    return {"p_minus_1": c.p - 1, "p": c.p, "all_ones": top - 1}[xcls]


@functools.lru_cache(maxsize=None)
def k256_alias_y_point():
    """(x, y0) on secp256k1 with the smallest y0 >= 1 for which y0^2 - 7 is a cube: p + y0 fits in 32 bytes"""
    c = M.K256
    assert c.p % 9 == 7
    for y0 in range(1, 1000):
        a = (y0 * y0 - 7) % c.p
        x = pow(a, (c.p + 2) // 9, c.p)
        if pow(x, 3, c.p) == a:
            assert M.on_curve(c, (x, y0)) and c.p + y0 < 1 << 256
            return x, y0
    raise AssertionError


def golden_encodings(cn):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.json")) as f:
        return json.load(f)[cn]["encoding"]


@functools.lru_cache(maxsize=None)
def decode_rows(cn, wide):
    c = M.CURVES[cn]
    nb = c.nbytes
    width = 1 + (2 if wide else 1) * nb
    ib = lambda v: int(v).to_bytes(nb, "big")
    pad = lambda b: b + bytes(width - len(b))
    rows = []
    vx, vy = pool(cn)[10]
    # every tag over a valid x: the uncompressed and the hybrid tags with y behind it, where a record has room
    for tag in TAGS:
        body = ib(vx) + (ib(vy) if wide and tag in (4, 6, 7) else b"")
        rows.append(DecRow(("tag", tag), pad(bytes([tag]) + body)))
    for tag in (2, 3, 5):
        for xcls in X_CLASSES:
            rows.append(DecRow(("x", tag, xcls), pad(bytes([tag]) + ib(x_of_class(c, xcls)))))
    # the compact rule on every point of the pool, and the leading-zero and zero abscissas under the compressed tags
    for k, P in enumerate(pool(cn)):
        rows.append(DecRow(("compact_pool", k), pad(b"\x05" + ib(P[0]))))
    for k, P in enumerate(pool(cn)[64:]):
        rows.append(DecRow(("small_x", k), pad(bytes([2 + P[1] % 2]) + ib(P[0]))))
    rows.append(DecRow(("zero_x", 2), pad(b"\x02" + ib(0))))
    rows.append(DecRow(("zero_x", 3), pad(b"\x03" + ib(0))))
    rows.append(DecRow(("identity",), bytes(width)))
    body_byte = bytearray(width)
    body_byte[1 + nb // 2] = 1
    rows.append(DecRow(("identity_body_byte",), bytes(body_byte)))
    enc = golden_encodings(cn)
    if wide:
        x0 = smallest_x_with_root(c)
        y_of_x0 = M.decompress(c, x0, 0)[1]
        if cn == "k256":
            ax, ay0 = k256_alias_y_point()
            big_y = (ax, c.p + ay0)
        else:
            big_y = (vx, c.p + 1)
        unc = {"xy": (vx, vy), "x_negy": (vx, c.p - vy), "y_plus_1": (vx, vy + 1), "y_minus_1": (vx, vy - 1),
               "p_plus_x0_y": (c.p + x0, y_of_x0), "y_ge_p": big_y}
        for ucls in UNCOMPRESSED_CLASSES:
            rows.append(DecRow(("uncompressed", ucls), b"\x04" + ib(unc[ucls][0]) + ib(unc[ucls][1])))
        for pos, off in zip(TAIL_POSITIONS, (1 + nb, 1 + nb + nb // 2, 2 * nb)):
            r = bytearray(pad(b"\x02" + ib(vx)))
            r[off] = 0x80 if pos == "first" else 1
            rows.append(DecRow(("tail", pos), bytes(r)))
        tail_byte = bytearray(width)
        tail_byte[width - 1] = 1
        rows.append(DecRow(("identity_tail_byte",), bytes(tail_byte)))
        if "uncompact_basepoint" in enc:
            rows.append(DecRow(("golden", "uncompact"), bytes.fromhex(enc["uncompact_basepoint"])))
        rows.append(DecRow(("golden", "uncompressed"), bytes.fromhex(enc["uncompressed_basepoint"])))
    if "compact_basepoint" in enc:
        rows.append(DecRow(("golden", "compact"), pad(bytes.fromhex(enc["compact_basepoint"]))))
    rows.append(DecRow(("golden", "compressed"), pad(bytes.fromhex(enc["compressed_basepoint"]))))
    assert all(len(r.record) == width for r in rows)
    return tuple(rows)


def rotate(seq, k):
    k %= len(seq)
    return list(seq[k:]) + list(seq[:k])


# ---------------------------------------------------------------------------------------------------------------------------------
# pools of DEVICE_POOL rows that the device-sized tests tile
# ---------------------------------------------------------------------------------------------------------------------------------
def device_decode_pool(cn):
    """DEVICE_POOL wide records: the uncompressed encodings of affine_rows with every 41st row taken from the class matrix"""
    c = M.CURVES[cn]
    matrix = decode_rows(cn, True)
    recs = [sec1_encode_model(c, P, False) for P in affine_rows(cn, DEVICE_POOL)]
    for k, i in enumerate(range(5, DEVICE_POOL, 41)):
        recs[i] = matrix[k % len(matrix)].record
    return recs
