"""The rows of tests/encoding_edge_vectors.py are what they claim (CPU only): the layout rule puts the planted identities into the
slots and lanes it names, every Z class, identity form and decode class occurs, the near misses are near misses, and the model of the
wide decoder agrees with oracle.ecmodel on every narrow record.  tests/test_gpu_encoding_edges.py runs the same rows through the C ABI."""
import pytest

import encoding_edge_vectors as V
from oracle import ecmodel as M

CURVES = list(V.CURVES)
CUS = [256, 4]


@pytest.mark.parametrize("cus", CUS)
def test_layout_rule(cus):
    for n in V.NORMALIZE_SIZES:
        L = V.layout(n, cus)
        g = L.geo
        assert g.T == 256 * g.blocks and 1 <= g.blocks <= 8 * cus
        assert (g.blocks - 1) * 256 * 16 < n or g.blocks == 1         # no workgroup without a row
        assert g.blocks * 256 * 16 >= n or g.blocks == 8 * cus        # one pass, unless the grid is at its cap
        # a (pass, lane, slot) holds one row, and the rows a lane holds in one pass are T apart
        seen = {(i // (16 * g.T),) + ls: i for i, ls in enumerate(L.norm)}
        assert len(seen) == n and all(0 <= lane < g.T and 0 <= slot < 16 for lane, slot in L.norm)
        assert all(i == 16 * g.T * q + lane + g.T * slot for (q, lane, slot), i in seen.items())
    assert [V.geometry(n, cus).T for n in (4096, 4097, 8197)] == [256, 512, 768]
    full = V.layout(4096, cus)
    assert full.geo.passes == 1 and sorted(full.norm) == [(l, s) for l in range(256) for s in range(16)]
    # the ragged last batch: at 4089 the lanes 249 .. 255 hold 15 rows, at 257 lane 0 holds two and the others one
    assert max(s for l, s in V.layout(4089, cus).norm if l >= 249) == 14 and (248, 15) in V.layout(4089, cus).norm
    assert V.layout(257, cus).norm[256] == (0, 1)
    # the device-sized batches enter the outer loops a second time and end ragged
    n = V.normalize_pass_rows(cus)
    g = V.geometry(n, cus)
    assert g.blocks == 8 * cus and g.passes == 2 and n - 16 * g.T == 3 * 256 + 5
    assert V.norm_place(16 * g.T - 1, g.T) == (0, g.T - 1, 15) and V.norm_place(16 * g.T, g.T) == (1, 0, 0)
    assert V.norm_place(n - 1, g.T) == (1, 3 * 256 + 4, 0)
    n = V.encode_pass_rows(cus)
    g = V.geometry(n, cus)
    assert g.grid == 8 * cus and g.tiles == g.grid + 2 and g.tile_passes == 2 and n - 256 * (g.tiles - 1) == 3
    for n in V.ENCODE_SIZES:
        L = V.layout(n, cus)
        assert L.geo.tiles == -(-n // 256) and L.geo.grid == min(L.geo.tiles, 8 * cus) and L.enc[-1] == ((n - 1) // 256, (n - 1) % 256)
    assert max(V.geometry(n, cus).tiles for n in V.ENCODE_SIZES) == 4 and V.layout(771, cus).enc[-1] == (3, 2)


def test_last_tile_byte_counts_cover_every_tail():
    """records are 33, 49, 65 or 97 bytes: over the encode sizes the last tile's byte count takes every value of bytes & 3, so the
    byte tail of to_bytes_kernel is empty, 1, 2 and 3 bytes long; full tiles (no tail) and last tiles of 1, 2 and 3 records occur"""
    assert V.record_widths() == [33, 49, 65, 97]
    for w in V.record_widths():
        assert {V.last_tile_tail(n, w) for n in V.ENCODE_SIZES} == {0, 1, 2, 3}, w
    assert {(n - 1) % 256 + 1 for n in V.ENCODE_SIZES} >= {1, 2, 3, 255, 256}
    assert V.last_tile_tail(V.DEVICE_N, 65) != 0 and V.last_tile_tail(V.ROUND_TRIP_N, 33) != 0


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("cn", CURVES)
def test_normalize_4096_layout(cn, cus):
    c = M.CURVES[cn]
    rows = V.proj_rows(cn, 4096)
    L = V.layout(4096, cus)
    lanes = {}
    for r, (lane, slot) in zip(rows, L.norm):
        lanes.setdefault(lane, [None] * 16)[slot] = r
    ident = lambda r: r.xyz[2] == 0
    assert len(lanes) == 256 and all(None not in v for v in lanes.values())
    for l in range(16):                                      # the single identity of lane l sits in slot l
        assert [s for s in range(16) if ident(lanes[l][s])] == [l]
    S = V.SPECIAL
    assert all(ident(r) for r in lanes[S["all_identity"]])
    assert [ident(r) for r in lanes[S["only_slot0_finite"]]] == [False] + [True] * 15
    assert [ident(r) for r in lanes[S["only_slot15_finite"]]] == [True] * 15 + [False]
    assert [ident(r) for r in lanes[S["alternating"]]] == [True, False] * 8
    assert [ident(r) for r in lanes[S["alternating_odd"]]] == [False, True] * 8
    special = set(range(16)) | set(S.values())
    assert {l // 64 for l in special} == {0, 1, 2, 3}        # every wave of the workgroup has one
    assert all(not ident(r) for l, v in lanes.items() if l not in special for r in v)
    # both identity forms, and finite neighbours of every Z class in the lanes with a single identity
    assert {r.zcls for r in rows if ident(r)} == set(V.IDENTITY_FORMS)
    assert {r.zcls for l in range(16) for r in lanes[l] if not ident(r)} == set(V.Z_CLASSES)
    for r in rows:
        X, Y, Z = r.xyz
        if r.zcls == "canonical":
            assert (X, Y, Z) == (0, 1, 0)
        elif r.zcls == "xy0":
            assert X and Y and Z == 0
        else:
            assert Z == {"one": 1, "two": 2, "p_minus_1": c.p - 1}.get(r.zcls, Z) and 0 < Z < c.p
    want = V.proj_affine(cn, 4096)
    assert sum(a[2] for a in want) == sum(1 for r in rows if ident(r)) == 16 + 16 + 15 + 15 + 8 + 8
    assert all(M.on_curve(c, (x, y)) for x, y, inf in want if not inf)


@pytest.mark.parametrize("cn", CURVES)
def test_cycled_rows_and_pool(cn):
    c = M.CURVES[cn]
    pts = V.pool(cn)
    assert len(pts) == (66 if cn == "k256" else 68)
    assert {P[1] % 2 for P in pts} == {0, 1}
    x1 = V.smallest_x_with_root(c)
    assert {P[0] for P in pts[64:66]} == {x1} and M.i2b(c, x1)[:c.nbytes - 1] == bytes(c.nbytes - 1)
    assert all(M.decompress(c, x, 0) is None for x in range(1, x1))
    if cn == "k256":
        assert M.decompress(c, 0, 0) is None
    else:
        assert {P[0] for P in pts[66:]} == {0} and {P[1] % 2 for P in pts[66:]} == {0, 1}
        assert any(V.even_root_is_larger(c, P) for P in pts) and not all(V.even_root_is_larger(c, P) for P in pts)
    for n in V.NORMALIZE_SIZES:
        rows = V.proj_rows(cn, n)
        assert len(rows) == n
        ids = [i for i, r in enumerate(rows) if r.xyz[2] == 0]
        if n != 4096:
            assert ids == list(range(36, n, 37))
        if n >= 255:
            assert 0 < len(ids) < n and {rows[i].zcls for i in ids} == set(V.IDENTITY_FORMS)
            assert {r.zcls for r in rows} == set(V.Z_CLASSES) | set(V.IDENTITY_FORMS)
        assert sum(a[2] for a in V.proj_affine(cn, n)) == len(ids)
    # the cycled rows visit the whole pool, the points with a zero and a one-byte x among them
    assert {(a[0], a[1]) for a in V.proj_affine(cn, 255) if not a[2]} == set(pts)


@pytest.mark.parametrize("cn", CURVES)
def test_decode_classes(cn):
    c = M.CURVES[cn]
    nb = c.nbytes
    top = 1 << (8 * nb)
    for wide in (False, True):
        rows = V.decode_rows(cn, wide)
        cls = [r.cls for r in rows]
        assert len(set(cls)) == len(cls)
        assert {k[1] for k in cls if k[0] == "tag"} == set(V.TAGS)
        assert {k[1:] for k in cls if k[0] == "x"} == {(t, x) for t in (2, 3, 5) for x in V.X_CLASSES}
        if wide:
            assert {k[1] for k in cls if k[0] == "uncompressed"} == set(V.UNCOMPRESSED_CLASSES)
            assert {k[1] for k in cls if k[0] == "tail"} == set(V.TAIL_POSITIONS)
            assert ("identity_tail_byte",) in cls
        assert ("identity",) in cls and ("identity_body_byte",) in cls
        verdicts = {}
        for r in rows:
            verdicts.setdefault(r.record[0], set()).add(V.sec1_decode_model(c, r.record)[0])
        both = {0, 2, 3, 5} | ({4} if wide else set())
        for tag in V.TAGS:
            assert verdicts[tag] == ({True, False} if tag in both else {False}), (wide, tag)
        by = {r.cls: r for r in rows}
        model = lambda k: V.sec1_decode_model(c, by[k].record)
        for tag in (2, 3, 5):
            assert model(("x", tag, "valid"))[0] and not model(("x", tag, "no_root"))[0]
            for xcls in ("p", "p_plus_x0", "all_ones"):
                x = M.b2i(by[("x", tag, xcls)].record[1:1 + nb])
                assert c.p <= x < top and not model(("x", tag, xcls))[0]
            # the near miss: reduced, x is an abscissa of the curve
            x = M.b2i(by[("x", tag, "p_plus_x0")].record[1:1 + nb])
            assert x >= c.p and M.decompress(c, x % c.p, 0) is not None and x % c.p == V.smallest_x_with_root(c)
            assert model(("x", tag, "p_minus_1"))[0] == (M.decompress(c, c.p - 1, 0) is not None)
        # 02 00..00: the point with x = 0 on the NIST curves, whatever decompress says on secp256k1 (no such point)
        for tag in (2, 3):
            ok, P = model(("zero_x", tag))
            assert (ok, P) == ((True, M.decompress(c, 0, tag & 1)) if M.decompress(c, 0, 0) else (False, None))
            assert ok == (cn != "k256") and (not ok or (P[0] == 0 and P[1] % 2 == tag & 1))
        assert model(("identity",)) == (True, None) and not model(("identity_body_byte",))[0]
        # the compact rule: rows where the even root is the larger one exist on the NIST curves, and the model takes the smaller
        larger = [k for k, P in enumerate(V.pool(cn)) if V.even_root_is_larger(c, P)]
        assert larger and len(larger) < len(V.pool(cn))
        for k, P in enumerate(V.pool(cn)):
            ok, Q = model(("compact_pool", k))
            even = P[1] if P[1] % 2 == 0 else c.p - P[1]
            assert ok and Q == (P[0], even if cn == "k256" else min(P[1], c.p - P[1]))
            if cn != "k256" and k in larger:
                assert Q[1] % 2 == 1
        if wide:
            assert model(("uncompressed", "xy"))[0] and model(("uncompressed", "x_negy"))[0]
            for u in ("y_plus_1", "y_minus_1", "p_plus_x0_y", "y_ge_p"):
                assert not model(("uncompressed", u))[0]
            r = by[("uncompressed", "p_plus_x0_y")].record
            x, y = M.b2i(r[1:1 + nb]), M.b2i(r[1 + nb:])
            assert x >= c.p and y < c.p and M.on_curve(c, (x % c.p, y))
            r = by[("uncompressed", "y_ge_p")].record
            x, y = M.b2i(r[1:1 + nb]), M.b2i(r[1 + nb:])
            assert x < c.p and c.p <= y < top
            assert M.on_curve(c, (x, y % c.p)) == (cn == "k256")       # only secp256k1 has room for an alias of y on the curve
            for pos in V.TAIL_POSITIONS:
                r = by[("tail", pos)].record
                assert sum(1 for b in r[1 + nb:] if b) == 1 and not model(("tail", pos))[0]
                assert V.sec1_decode_model(c, r[:1 + nb])[0]
            assert by[("tail", "first")].record[1 + nb] != 0 and by[("tail", "last")].record[-1] != 0
            assert not model(("identity_tail_byte",))[0]
        golden = [k for k in cls if k[0] == "golden"]
        assert len(golden) == (2 if wide else 1) * (1 if cn == "k256" else 2 if cn == "p256" else 1)
        for k in golden:
            ok, P = model(k)
            assert ok and M.on_curve(c, P) and (P == (c.gx, c.gy)) == (k[1] in ("compressed", "uncompressed"))
        if wide and ("golden", "compact") in by:
            assert model(("golden", "compact")) == model(("golden", "uncompact"))


@pytest.mark.parametrize("cn", CURVES)
def test_model_agrees_with_the_oracle_and_round_trips(cn):
    c = M.CURVES[cn]
    nb = c.nbytes
    narrow = [r.record for r in V.decode_rows(cn, False)] + [r.record[:1 + nb] for r in V.decode_rows(cn, True)]
    for rec in narrow:
        assert V.sec1_decode_model(c, rec) == M.group_from_bytes(c, rec), rec.hex()
        if rec[0] != 4:                                      # zero padded in a wide record: the same verdict
            assert V.sec1_decode_model(c, rec + bytes(nb)) == V.sec1_decode_model(c, rec)
    for P in V.pool(cn) + (None,):
        for compress in (True, False):
            rec = V.sec1_encode_model(c, P, compress)
            assert len(rec) == 1 + (1 if compress else 2) * nb
            assert V.sec1_decode_model(c, rec) == (True, P)
        assert V.sec1_encode_model(c, P, True) == M.group_to_bytes(c, P)
        assert V.decoded_bytes(c, V.sec1_encode_model(c, P, False)) == (V.affine_bytes(c, P), 1)
    assert V.decoded_bytes(c, b"\x06" + bytes(nb)) == (bytes(2 * nb), 0)


@pytest.mark.parametrize("cn", ["k256", "p384"])
def test_device_pools(cn):
    c = M.CURVES[cn]
    recs = V.device_decode_pool(cn)
    assert len(recs) == V.DEVICE_POOL == len(V.affine_rows(cn, V.DEVICE_POOL)) and V.DEVICE_POOL % 256 != 0
    oks = [V.sec1_decode_model(c, r)[0] for r in recs]
    assert 10 < oks.count(False) < 100 and {r[0] for r in recs} >= {0, 2, 3, 4, 5, 6}
    assert sum(1 for P in V.affine_rows(cn, V.DEVICE_POOL) if P is None) == V.DEVICE_POOL // 37
