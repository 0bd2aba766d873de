"""Shared points on the GPU (ECGPU_SHARED_POINTS): one point, or `terms` points, for the whole batch, multiplied from tables cached in
the context.  Expected values come from the oracle - oracle/ecmodel.py for the planted edge cases, oracle/coracle.py for bulk - and,
as a second check, from the same call with the points replicated.  OPT_SHARED_MIN = 1 and OPT_SHARED_WINDOW pin the path under test;
every test restores both."""
import json
import os
import random

import numpy as np
import pytest

import shared_points_vectors as V
from oracle import coracle as CO
from oracle import ecmodel as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = ["k256", "p256", "p384"]
ERR_ARG, ERR_UNSUPPORTED = "error -1:", "error -4:"        # as Context.check and Group.check word an ecgpu_status


@pytest.fixture(scope="module")
def E():
    """The guard: on a tree without the feature the flag would be ignored and a short `points` buffer read as n points, so nothing is
    handed to the library before the flag and the options are known to exist."""
    import ecgpu
    assert getattr(ecgpu, "SHARED_POINTS", None) == 64
    probe = ecgpu.Context(0)
    try:
        assert probe.get_option(ecgpu.OPT_SHARED_MIN) == 0
    finally:
        probe.close()
    return ecgpu


@pytest.fixture(scope="module")
def ctx(E):
    c = E.Context(0)
    yield c
    c.close()


@pytest.fixture
def pin(E, ctx):
    """pin(wb, min_n=1): the table path at that width (0: by the size rule); restored afterwards"""
    def set_(wb, min_n=1):
        ctx.set_option(E.OPT_SHARED_WINDOW, wb)
        ctx.set_option(E.OPT_SHARED_MIN, min_n)
    yield set_
    ctx.set_option(E.OPT_SHARED_WINDOW, 0)
    ctx.set_option(E.OPT_SHARED_MIN, 0)


def to_rows(c, values):
    return np.frombuffer(b"".join(M.i2b(c, v) for v in values), dtype=np.uint8).reshape(len(values), c.nbytes).copy()


def pts_rows(c, pts):
    return np.frombuffer(b"".join(V.point_bytes(c, p) for p in pts), dtype=np.uint8).reshape(len(pts), 2 * c.nbytes).copy()


def plant(c, n, edge, seed):
    """n scalars from the seeded generator with the edge list at both ends and in the middle (cycled through where n is small)"""
    ks = [k % c.n for k in V.synth.scalars(c, n, seed=seed)]
    if n >= 3 * len(edge):
        for at in (0, (n - len(edge)) // 2, n - len(edge)):
            ks[at:at + len(edge)] = edge
        where = list(range(len(edge))) + list(range((n - len(edge)) // 2, (n - len(edge)) // 2 + len(edge))) + list(range(n - len(edge), n))
    else:
        ks = [edge[(i + n) % len(edge)] for i in range(n)]
        where = list(range(n))
    return ks, where


def oracle_lincomb(c, cid, ks, pts, terms):
    """sum_j ks[i terms + j] pts[j] for every element: per-term products from the C oracle (scalars mod n: it takes them reduced),
    folded in the affine model -> list of affine points (None = the identity)"""
    n = len(ks) // terms
    sc = to_rows(c, [k % c.n for k in ks])
    prods = CO.lincomb_batch(cid, sc, np.tile(pts_rows(c, pts), (n, 1)), threads=8)
    nb = c.nbytes
    out = []
    for i in range(n):
        acc = None
        for j in range(terms):
            row = prods[i * terms + j]
            if not row[2 * nb]:
                acc = M.affine_add(c, acc, (M.b2i(bytes(row[:nb])), M.b2i(bytes(row[nb:2 * nb]))))
        out.append(acc)
    return out


def check_affine(c, xy, inf, want, what):
    for i, w in enumerate(want):
        assert bytes(xy[i]) == V.point_bytes(c, w) and inf[i] == (1 if w is None else 0), (what, i)


def check_projective(c, xyz, want, what):
    nb = c.nbytes
    for i, w in enumerate(want):
        exp = bytes(nb) + M.i2b(c, 1) + bytes(nb) if w is None else V.point_bytes(c, w) + M.i2b(c, 1)
        assert bytes(xyz[i]) == exp, (what, i)


# ---- 1. one point ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("wb", [8, 16])
def test_mul(E, ctx, pin, cn, wb):
    c, cid, cv = M.CURVES[cn], M.CURVE_IDS[cn], ctx.curve(cn)
    pin(wb)
    h = V.points(c, 1, start=100 + wb)[0]
    hp = pts_rows(c, [h])
    edge = V.edge_scalars(c, wb)
    for n in (1, 63, 64, 65, 257, 1000):
        ks, where = plant(c, n, edge, seed=n)
        sc = to_rows(c, ks)
        want = oracle_lincomb(c, cid, ks, [h], 1)
        for i in where if n == 1000 else ():                 # the planted ones once more, from the independent affine model
            assert want[i] == M.affine_mul(c, ks[i], h), (n, i)
        xy, inf = cv.mul(sc, hp, flags=E.SHARED_POINTS)
        check_affine(c, xy, inf, want, (cn, wb, n))
        xyz = cv.mul(sc, hp, out_format=E.PROJECTIVE, flags=E.SHARED_POINTS)
        check_projective(c, xyz, want, (cn, wb, n))
        rxy, rinf = cv.mul(sc, np.tile(hp, (n, 1)))          # byte for byte the replicated call
        assert bytes(rxy) == bytes(xy) and bytes(rinf) == bytes(inf)
        assert bytes(cv.mul(sc, np.tile(hp, (n, 1)), out_format=E.PROJECTIVE)) == bytes(xyz)


# ---- 2. the table's entries, reached through scalars d 2^(16 j) ------------------------------------------------------------------
@pytest.mark.parametrize("cn", CURVES)
def test_table_content_through_the_api(E, ctx, pin, cn):
    c, cv = M.CURVES[cn], ctx.curve(cn)
    pin(16)
    h = V.points(c, 1, start=131)[0]
    entries = V.table_entries(c, 16, through_scalars=True)
    ks = [d << (16 * j) for d, j in entries]
    xy, inf = cv.mul(to_rows(c, ks), pts_rows(c, [h]), flags=E.SHARED_POINTS)
    check_affine(c, xy, inf, [M.affine_mul(c, k, h) for k in ks], cn)


# ---- 3. several points, related ones included ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("wb", [8, 16])
def test_lincomb_related_points(E, ctx, pin, cn, wb):
    c, cid, cv = M.CURVES[cn], M.CURVE_IDS[cn], ctx.curve(cn)
    pin(wb)
    n = 257
    k0 = 0x1234567 << 40 | 0x89AB
    sets = dict(V.related_sets(c))
    sets["3 unrelated"] = V.points(c, 3, start=60)
    identity_seen = 0
    for name, pts in sets.items():
        terms = len(pts)
        assert terms in (2, 3, 8)
        rows = [[k % c.n for k in V.synth.scalars(c, terms, seed=7, start=i * terms)] for i in range(n)]
        special = [[e] * terms for e in V.edge_scalars(c, wb)[:6]]
        if name in ("H,H", "H,-H", "H,2H", "H,O"):
            special += V.identity_sum_rows(c, name, k0)
        if name == "H,H,H":
            special += V.branch_rows(c, 3)
        for at, row in zip((0, 1, 2, 63, 64, 65, 128, 129, 130, 200, 254, 255, 256, 31, 32, 33), special):
            rows[at] = row
        ks = [k for row in rows for k in row]
        want = oracle_lincomb(c, cid, ks, pts, terms)
        for row in special:
            assert want[rows.index(row)] == V.combination(c, row, pts), (name, row)
        identity_seen += sum(w is None for w in want)
        sc, pp = to_rows(c, ks), pts_rows(c, pts)
        xy, inf = cv.lincomb(sc, pp, terms=terms, flags=E.SHARED_POINTS)
        check_affine(c, xy, inf, want, (cn, wb, name))
        xyz = cv.lincomb(sc, pp, terms=terms, out_format=E.PROJECTIVE, flags=E.SHARED_POINTS)
        check_projective(c, xyz, want, (cn, wb, name))
        rxy, rinf = cv.lincomb(sc, np.tile(pp, (n, 1)), terms=terms)
        assert bytes(rxy) == bytes(xy) and bytes(rinf) == bytes(inf), name
    assert identity_seen >= 8


# ---- 4. dynamic draws: many chunks per wave, device-resident ---------------------------------------------------------------------
def sampled(n):
    idx = set(range(4096)) | set(range(n - 4096, n)) | set(range(0, n, 64))
    return np.array(sorted(idx))


def test_two_terms_device_resident(E, ctx, pin):
    import torch
    c, cid, cv = M.K256, 0, ctx.curve("k256")
    pin(16)
    n, terms = (1 << 19) + 77, 2
    pts = V.points(c, 2, start=150)
    pp = pts_rows(c, pts)
    d_sc = torch.empty((n * terms, 32), dtype=torch.uint8, device="cuda")
    d_out = torch.full((n, 64), 0xAB, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")
    cv.synth_scalars_device(d_sc, n * terms, seed=99)
    cv._call("ecgpu_lincomb_batch", d_sc, pp, E.AFFINE, terms, d_out, E.AFFINE, d_inf, n, E.DEVICE, E.SHARED_POINTS)
    ctx.synchronize()
    idx = sampled(n)
    sc = d_sc.cpu().numpy().reshape(n, terms * 32)[idx].reshape(-1, 32)
    want = CO.lincomb_batch(cid, sc, np.tile(pp, (len(idx), 1)), terms=2, threads=8)
    got, inf = d_out.cpu().numpy()[idx], d_inf.cpu().numpy()[idx]
    assert bytes(got) == bytes(np.ascontiguousarray(want[:, :64])) and bytes(inf) == bytes(np.ascontiguousarray(want[:, 64]))
    assert set(np.unique(d_inf.cpu().numpy())) <= {0, 1}          # every element was written


# ---- 5. the host pipeline: the scalars stream in chunks, the point does not ----------------------------------------------------------
def test_host_pipeline(E, ctx, pin):
    c, cid, cv = M.K256, 0, ctx.curve("k256")
    pin(0)                                                        # the size rule: 16-bit windows at this size
    n = (1 << 21) + 12345
    h = V.points(c, 1, start=160)[0]
    hp = pts_rows(c, [h])
    sc = np.random.default_rng(5).integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 0] &= 0x7F                                              # below n
    builds = ctx.get_option(E.OPT_SHARED_TABLE_BUILDS)
    xy, inf = cv.mul(sc, hp, flags=E.SHARED_POINTS)
    assert ctx.get_option(E.OPT_SHARED_TABLE_BUILDS) == builds + 1
    idx = sampled(n)
    want = CO.lincomb_batch(cid, sc[idx], np.tile(hp, (len(idx), 1)), threads=8)
    assert bytes(xy[idx]) == bytes(np.ascontiguousarray(want[:, :64])) and bytes(inf[idx]) == bytes(np.ascontiguousarray(want[:, 64]))
    assert xy[n // 2 - 2048:n // 2 + 2048].any(axis=1).all()      # no row in the middle of the stream left unwritten


# ---- 6. 20-bit windows -----------------------------------------------------------------------------------------------------
def test_window_20(E, ctx, pin):
    c, cid, cv = M.K256, 0, ctx.curve("k256")
    pin(20)
    n = 1000
    pts = V.points(c, 2, start=170)
    ks, _ = plant(c, n, V.edge_scalars(c, 20), seed=20)
    xy, inf = cv.mul(to_rows(c, ks), pts_rows(c, pts[:1]), flags=E.SHARED_POINTS)
    check_affine(c, xy, inf, oracle_lincomb(c, cid, ks, pts[:1], 1), "one point")
    ks2 = ks + [k % c.n for k in V.synth.scalars(c, n, seed=21)]
    ks2 = [ks2[(i % 2) * n + i // 2] for i in range(2 * n)]       # interleaved: the edge scalars in the first term
    xy, inf = cv.lincomb(to_rows(c, ks2), pts_rows(c, pts), terms=2, flags=E.SHARED_POINTS)
    check_affine(c, xy, inf, oracle_lincomb(c, cid, ks2, pts, 2), "two points")


# ---- 7. secret scalars: the constant-time kernel on a 5-bit table of the point ------------------------------------------------------
@pytest.mark.parametrize("cn", CURVES)
def test_secret_scalars(E, ctx, pin, cn):
    c, cid, cv = M.CURVES[cn], M.CURVE_IDS[cn], ctx.curve(cn)
    pin(0)
    n = 257
    h = V.points(c, 1, start=180)[0]
    hp = pts_rows(c, [h])
    ks, _ = plant(c, n, V.edge_scalars(c, 5), seed=5)
    sc = to_rows(c, ks)
    want = oracle_lincomb(c, cid, ks, [h], 1)
    builds = ctx.get_option(E.OPT_SHARED_TABLE_BUILDS)
    xy, inf = cv.mul(sc, hp, flags=E.SHARED_POINTS | E.SECRET_SCALARS)
    assert ctx.get_option(E.OPT_SHARED_TABLE_BUILDS) == builds + 1
    check_affine(c, xy, inf, want, cn)
    xy2, inf2 = cv.mul(sc[::-1].copy(), hp, flags=E.SHARED_POINTS | E.SECRET_SCALARS)
    assert ctx.get_option(E.OPT_SHARED_TABLE_BUILDS) == builds + 1          # the 5-bit table was built once and reused
    check_affine(c, xy2, inf2, want[::-1], cn)
    rxy, rinf = cv.mul(sc, np.tile(hp, (n, 1)), flags=E.SECRET_SCALARS)
    assert bytes(rxy) == bytes(xy) and bytes(rinf) == bytes(inf)


# ---- 8. the broadcast path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", CURVES)
def test_fallbacks(E, ctx, pin, cn):
    c, cid, cv = M.CURVES[cn], M.CURVE_IDS[cn], ctx.curve(cn)
    pin(8)
    n = 65
    pts = V.points(c, 9, start=190)
    builds = ctx.get_option(E.OPT_SHARED_TABLE_BUILDS)
    # the reference schedule's exact (X, Y, Z), one and two terms
    for terms in (1, 2):
        ks = [k % c.n for k in V.synth.scalars(c, n * terms, seed=80 + terms)]
        sc, pp = to_rows(c, ks), pts_rows(c, pts[:terms])
        xyz = cv.lincomb(sc, pp, terms=terms, out_format=E.PROJECTIVE, flags=E.SHARED_POINTS | E.EXACT_REFERENCE)
        want = CO.lincomb_batch(cid, sc, np.tile(pp, (n, 1)), terms=terms, out_proj=True, threads=8)
        assert bytes(xyz) == bytes(want), (cn, terms)
    # nine terms: more tables than one launch reads
    ks = [k % c.n for k in V.synth.scalars(c, n * 9, seed=89)]
    xy, inf = cv.lincomb(to_rows(c, ks), pts_rows(c, pts), terms=9, flags=E.SHARED_POINTS)
    check_affine(c, xy, inf, oracle_lincomb(c, cid, ks, pts, 9), (cn, 9))
    # secret scalars with two terms
    ks = [k % c.n for k in V.synth.scalars(c, n * 2, seed=82)]
    xy, inf = cv.lincomb(to_rows(c, ks), pts_rows(c, pts[:2]), terms=2, flags=E.SHARED_POINTS | E.SECRET_SCALARS)
    check_affine(c, xy, inf, oracle_lincomb(c, cid, ks, pts[:2], 2), (cn, "secret, 2 terms"))
    assert ctx.get_option(E.OPT_SHARED_TABLE_BUILDS) == builds
    # the default size rule: five results do not pay for a table of a point that has none
    ctx.set_option(E.OPT_SHARED_MIN, 0)
    ctx.set_option(E.OPT_SHARED_WINDOW, 0)
    ks = [k % c.n for k in V.synth.scalars(c, 5, seed=85)]
    xy, inf = cv.mul(to_rows(c, ks), pts_rows(c, pts[8:]), flags=E.SHARED_POINTS)
    check_affine(c, xy, inf, oracle_lincomb(c, cid, ks, pts[8:], 1), (cn, "n = 5"))
    assert ctx.get_option(E.OPT_SHARED_TABLE_BUILDS) == builds


@pytest.mark.parametrize("cn,log2_min,width_at_min", [("k256", 20, 16), ("p256", 18, 8)])
def test_default_size_rule(E, cn, log2_min, width_at_min):
    """The measured defaults (profiles/shared_points.txt): one result below the curve's minimum a point without a table gets none, at the
    minimum it gets one, of the width the rule names for that size."""
    ctx = E.Context(0)
    try:
        c, cid, cv = M.CURVES[cn], M.CURVE_IDS[cn], ctx.curve(cn)
        B = E.OPT_SHARED_TABLE_BUILDS
        n = 1 << log2_min
        h = V.points(c, 1, start=250)[0]
        hp = pts_rows(c, [h])
        sc = np.random.default_rng(log2_min).integers(0, 256, size=(n, c.nbytes), dtype=np.uint8)
        sc[:, 0] &= 0x7F                                          # below n
        idx = np.array(sorted(set(range(256)) | set(range(n - 257, n - 1)) | set(range(0, n - 1, 4096))))
        want = CO.lincomb_batch(cid, sc[idx], np.tile(hp, (len(idx), 1)), threads=8)
        for count, builds in ((n - 1, 0), (n, 1)):
            xy, inf = cv.mul(sc[:count], hp, flags=E.SHARED_POINTS)
            assert ctx.get_option(B) == builds, count
            assert bytes(xy[idx]) == bytes(np.ascontiguousarray(want[:, :-1])) and bytes(inf[idx]) == bytes(np.ascontiguousarray(want[:, -1])), count
        ctx.set_option(E.OPT_SHARED_WINDOW, width_at_min)         # the table that was built has this width: pinned to it, a call that
        ctx.set_option(E.OPT_SHARED_MIN, 1)                       # would build any table it misses hits
        cv.mul(sc[:8], hp, flags=E.SHARED_POINTS)
        assert ctx.get_option(B) == 1
    finally:
        ctx.close()


# ---- 9. the cache ----------------------------------------------------------------------------------------------------------
def test_cache(E):
    ctx = E.Context(0)                                            # its own context: the counter and the budget start from nothing
    try:
        c, cid, cv = M.K256, 0, ctx.curve("k256")
        B = E.OPT_SHARED_TABLE_BUILDS
        ctx.set_option(E.OPT_SHARED_MIN, 1)
        ctx.set_option(E.OPT_SHARED_WINDOW, 16)
        n = 300
        p1, p2 = V.points(c, 2, start=200)
        ks = [k % c.n for k in V.synth.scalars(c, n, seed=90)]
        sc = to_rows(c, ks)
        want = {0: oracle_lincomb(c, cid, ks, [p1], 1), 1: oracle_lincomb(c, cid, ks, [p2], 1)}

        def run(which):
            xy, inf = cv.mul(sc, pts_rows(c, [(p1, p2)[which]]), flags=E.SHARED_POINTS)
            check_affine(c, xy, inf, want[which], which)
        assert ctx.get_option(B) == 0
        run(0)
        assert ctx.get_option(B) == 1
        run(0)
        assert ctx.get_option(B) == 1                             # a hit builds nothing
        run(1)
        assert ctx.get_option(B) == 2                             # a new point builds one table
        run(0), run(1)
        assert ctx.get_option(B) == 2
        # the default size rule uses a cached table at any size
        ctx.set_option(E.OPT_SHARED_MIN, 0)
        ctx.set_option(E.OPT_SHARED_WINDOW, 0)
        xy, inf = cv.mul(sc[:5], pts_rows(c, [p1]), flags=E.SHARED_POINTS)
        check_affine(c, xy, inf, want[0][:5], "hit at n = 5")
        assert ctx.get_option(B) == 2
        ctx.set_option(E.OPT_SHARED_MIN, 1)
        ctx.set_option(E.OPT_SHARED_WINDOW, 16)
        # room for ONE 16-bit table (17 x 2^15 entries of 64 bytes) and a little more: two points evict each other
        ctx.set_option(E.OPT_SHARED_TABLE_BUDGET, 17 * (1 << 15) * 64 + (1 << 20))
        ctx.set_option(B, 0)
        with pytest.raises(E.EcgpuError):
            ctx.set_option(B, 1)                                  # a counter: reset only
        for i in range(4):                                        # (p1 was used last, so it is p2 that the smaller budget put out first)
            run((i + 1) % 2)
            assert ctx.get_option(B) == i + 1
        # a budget below one 16-bit table: the call steps down to 8-bit windows and stays right
        ctx.set_option(E.OPT_SHARED_TABLE_BUDGET, 1 << 20)
        run(0)
        assert ctx.get_option(B) == 5
        run(0)
        assert ctx.get_option(B) == 5
        # a larger pinned width builds the wider table of a point that has a narrower one
        ctx.set_option(E.OPT_SHARED_TABLE_BUDGET, 1 << 31)
        ctx.set_option(E.OPT_SHARED_WINDOW, 8)
        run(1)
        assert ctx.get_option(B) == 6
        ctx.set_option(E.OPT_SHARED_WINDOW, 16)
        run(1)
        assert ctx.get_option(B) == 7
        # more points than a curve's 16 tables: the oldest go, everything stays right
        ctx.set_option(E.OPT_SHARED_WINDOW, 8)
        ctx.set_option(B, 0)
        many = V.points(c, 18, start=210)
        ks5 = ks[:5]
        for p in many:
            xy, inf = cv.mul(sc[:5], pts_rows(c, [p]), flags=E.SHARED_POINTS)
            check_affine(c, xy, inf, [M.affine_mul(c, k, p) for k in ks5], "many")
        assert ctx.get_option(B) == 18
        xy, inf = cv.mul(sc[:5], pts_rows(c, [many[-1]]), flags=E.SHARED_POINTS)       # the newest is still there
        assert ctx.get_option(B) == 18
        xy, inf = cv.mul(sc[:5], pts_rows(c, [many[0]]), flags=E.SHARED_POINTS)        # the oldest is not
        check_affine(c, xy, inf, [M.affine_mul(c, k, many[0]) for k in ks5], "rebuilt")
        assert ctx.get_option(B) == 19
        # four points, room for three 16-bit tables: the width is picked before the first build, nothing is built at 16 bits and dropped
        ctx.set_option(E.OPT_SHARED_WINDOW, 16)
        ctx.set_option(E.OPT_SHARED_TABLE_BUDGET, 3 * 17 * (1 << 15) * 64 + (1 << 20))
        ctx.set_option(B, 0)
        four = V.points(c, 4, start=300)
        ks4 = [k % c.n for k in V.synth.scalars(c, 4 * 9, seed=91)]
        xy, inf = cv.lincomb(to_rows(c, ks4), pts_rows(c, four), terms=4, flags=E.SHARED_POINTS)
        check_affine(c, xy, inf, oracle_lincomb(c, cid, ks4, four, 4), "four points")
        assert ctx.get_option(B) == 4
        xy, inf = cv.lincomb(to_rows(c, ks4), pts_rows(c, [four[0]] * 4), terms=4, flags=E.SHARED_POINTS)      # one distinct point: it fits at 16 bits
        check_affine(c, xy, inf, oracle_lincomb(c, cid, ks4, [four[0]] * 4, 4), "one point four times")
        assert ctx.get_option(B) == 5
    finally:
        ctx.close()


# ---- 10. errors: nothing is written ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", CURVES)
def test_errors(E, ctx, pin, cn):
    c, cv = M.CURVES[cn], ctx.curve(cn)
    nb = c.nbytes
    pin(8)
    n = 9
    h, p = V.points(c, 2, start=230)
    sc = to_rows(c, [k % c.n for k in V.synth.scalars(c, 2 * n, seed=3)])
    off_curve = (h[0], (h[1] + 1) % c.p)
    too_large = M.i2b(c, c.p) + M.i2b(c, h[1])                   # x = p is not below p
    for bad, index in ((pts_rows(c, [off_curve]), 0), (np.frombuffer(too_large, dtype=np.uint8).reshape(1, 2 * nb).copy(), 0),
                       (pts_rows(c, [p, off_curve]), 1)):
        terms = len(bad)
        for flags in (E.SHARED_POINTS, E.SHARED_POINTS | E.EXACT_REFERENCE, E.SHARED_POINTS | E.SECRET_SCALARS):
            out, inf = np.full((2 * n // terms, 2 * nb), 0xAB, dtype=np.uint8), np.full(2 * n // terms, 0xAB, dtype=np.uint8)
            with pytest.raises(E.EcgpuError) as ei:
                cv.lincomb(sc, bad, terms=terms, flags=flags, out=out, out_inf=inf)
            assert ERR_ARG in str(ei.value) and "shared point %d" % index in str(ei.value)
            assert (out == 0xAB).all() and (inf == 0xAB).all()
    # a projective point has many encodings of one key: refused at the C ABI as well as in the wrapper
    out = np.full((2 * n, 2 * nb), 0xAB, dtype=np.uint8)
    proj = np.frombuffer(V.point_bytes(c, h) + M.i2b(c, 1), dtype=np.uint8).reshape(1, 3 * nb).copy()
    with pytest.raises(E.EcgpuError) as ei:
        cv._call("ecgpu_lincomb_batch", sc, proj, E.PROJECTIVE, 1, out, E.AFFINE, None, 2 * n, E.HOST, E.SHARED_POINTS)
    assert ERR_ARG in str(ei.value)
    with pytest.raises(E.EcgpuError) as ei:
        cv._call("ecgpu_mul_batch", sc, None, E.AFFINE, out, E.AFFINE, None, 2 * n, E.HOST, E.SHARED_POINTS)
    assert ERR_ARG in str(ei.value)
    assert (out == 0xAB).all()


def test_entry_points_that_refuse_the_flag(E, ctx):
    c, cv = M.K256, ctx.curve("k256")
    n = 4
    sc = to_rows(c, [k % c.n for k in V.synth.scalars(c, n, seed=4)])
    pp = pts_rows(c, V.points(c, n, start=240))                   # n points: a library that ignored the flag would not overrun them
    out, inf, ok = np.full((n, 64), 0xAB, dtype=np.uint8), np.full(n, 0xAB, dtype=np.uint8), np.full(n, 0xAB, dtype=np.uint8)
    S = E.SHARED_POINTS
    msgs = [b"m%d" % i for i in range(n)]
    sig = np.ones((n, 64), dtype=np.uint8)
    rec, lens, stride = E.pack_messages_aligned(msgs)             # straight to the C ABI, with the caller's own `ok`
    for name, head in (("ecgpu_ecdsa_verify_msg_batch", ()), ("ecgpu_ecdsa_verify_digest_batch", (E.KECCAK256,))):
        with pytest.raises(E.EcgpuError) as ei:
            cv._call(name, *head, rec, stride, lens, sig, pp, ok, n, E.HOST, S)
        assert ERR_UNSUPPORTED in str(ei.value) and "ECGPU_SHARED_POINTS" in str(ei.value), name
        assert (ok == 0xAB).all(), name
    g = E.Group([0])
    try:
        import ctypes
        one = lambda a: (ctypes.c_void_p * 1)(a.ctypes.data)
        for name, args in (("ecgpu_group_lincomb_batch", (0, sc, pp, E.AFFINE, 1, out, E.AFFINE, inf, n, S)),
                           ("ecgpu_group_mul_batch", (0, sc, pp, E.AFFINE, out, E.AFFINE, inf, n, S)),
                           ("ecgpu_group_lincomb_sharded", (0, one(sc), one(pp), E.AFFINE, 1, one(out), E.AFFINE, None, (ctypes.c_size_t * 1)(n), S))):
            with pytest.raises(E.EcgpuError) as ei:
                E._call(g, name, *args)
            assert ERR_UNSUPPORTED in str(ei.value) and "ECGPU_SHARED_POINTS" in str(ei.value), name
    finally:
        g.close()
    assert (out == 0xAB).all() and (inf == 0xAB).all() and (ok == 0xAB).all()


# ---- 11. verification under one key ---------------------------------------------------------------------------------------------
def padded(c, hx):
    b = bytes.fromhex(hx)
    return b[len(b) - c.nbytes:] if len(b) >= c.nbytes else bytes(c.nbytes - len(b)) + b


@pytest.mark.parametrize("cn", CURVES)
def test_wycheproof_grouped_by_key(E, ctx, pin, cn):
    from ecgpu.der import decode_signature
    from ecgpu.ecdsa import DIGEST, bits2field
    c, cv = M.CURVES[cn], ctx.curve(cn)
    nb = c.nbytes
    pin(0)                                                        # the size rule picks the width, every key gets its table
    with open(os.path.join(HERE, "golden", f"wycheproof_{cn}.json")) as f:
        rows = json.load(f)["rows"]
    groups = {}
    for wx, wy, msg, der, verdict in rows:
        groups.setdefault(padded(c, wx) + padded(c, wy), []).append((bytes.fromhex(msg), bytes.fromhex(der), verdict))
    assert len(groups) > 1
    valid = 0
    for key, items in groups.items():
        z, sg, want = b"", b"", []
        for msg, der, verdict in items:
            rs = decode_signature(der, nb)
            if rs is None:                                        # Signature::from_der fails: the fixture's verdict is 0, nothing to verify
                assert verdict == 0
                continue
            r, s = rs
            if cn == "k256" and c.n // 2 < s < c.n:               # the k256 Wycheproof runner normalises s first (k256/src/ecdsa.rs:377)
                s = c.n - s
            z += bits2field(nb, DIGEST[cv.id](msg).digest())
            sg += r.to_bytes(nb, "big") + s.to_bytes(nb, "big")
            want.append(verdict)
        if not want:
            continue
        got = cv.ecdsa_verify(z, sg, key, flags=cv.default_ecdsa_flags() | E.SHARED_POINTS)
        assert list(got) == want, key.hex()
        assert bytes(got) == bytes(cv.ecdsa_verify(z, sg, key * len(want)))
        valid += sum(want)
    assert valid > 100


@pytest.mark.parametrize("cn,low_s", [("k256", False), ("k256", True), ("p256", False), ("p384", False)])
def test_signatures_under_one_key(E, ctx, pin, cn, low_s):
    c, cid, cv = M.CURVES[cn], M.CURVE_IDS[cn], ctx.curve(cn)
    nb = c.nbytes
    pin(8)
    n = 1000
    rng = random.Random(77 + nb)
    d = rng.randrange(1, c.n)
    q = M.affine_mul(c, d, (c.gx, c.gy))
    key = V.point_bytes(c, q)
    z = np.frombuffer(rng.randbytes(n * nb), dtype=np.uint8).reshape(n, nb).copy()
    sig, _, sok = cv.ecdsa_sign_prehash(M.i2b(c, d) * n, z, flags=E.ECDSA_LOW_S if low_s else 0)
    assert sok.all()
    sig = sig.copy()
    for i in range(0, n, 7):                                      # corrupt r, s or the digest of every seventh, in turn
        if i % 3 == 2:
            z[i, nb - 1] ^= 1
        else:
            sig[i, (i % 3) * nb + nb - 1] ^= 1
    sig[3] = 0                                                    # r = s = 0
    sig[5, nb:] = np.frombuffer(M.i2b(c, c.n), dtype=np.uint8)    # s = n
    if not low_s:                                                 # a high s verifies unless the low-s rule is on
        s10 = M.b2i(bytes(sig[10, nb:]))
        sig[10, nb:] = np.frombuffer(M.i2b(c, c.n - s10), dtype=np.uint8)
    flags = E.ECDSA_LOW_S if low_s else 0
    want = CO.ecdsa_verify_batch(cid, z, sig, np.tile(np.frombuffer(key, dtype=np.uint8), (n, 1)), low_s=low_s)
    for i in (0, 1, 3, 5, 7, 10, 14, 21):                         # a few from the Python model as well
        zi, r, s = bytes(z[i]), M.b2i(bytes(sig[i, :nb])), M.b2i(bytes(sig[i, nb:]))
        assert bool(want[i]) == M.ecdsa_verify_prehashed(c, q, zi, r, s, reject_high_s=low_s), i
    assert 0 < want.sum() < n
    got = cv.ecdsa_verify(z, sig, key, flags=flags | E.SHARED_POINTS)
    assert bytes(got) == bytes(want)
    assert bytes(cv.ecdsa_verify(z, sig, key * n, flags=flags)) == bytes(got)
    # device-resident, the key still in host memory
    import torch
    dz, ds = torch.from_numpy(z).cuda(), torch.from_numpy(sig).cuda()
    dok = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")
    cv.ecdsa_verify_device(dz, ds, key, dok, n, flags=flags | E.SHARED_POINTS)
    ctx.synchronize()
    assert bytes(dok.cpu().numpy()) == bytes(want)


@pytest.mark.parametrize("cn", CURVES)
def test_invalid_and_identity_keys_verify_nothing(E, ctx, pin, cn):
    c, cv = M.CURVES[cn], ctx.curve(cn)
    nb = c.nbytes
    pin(8)
    n = 50
    rng = random.Random(5)
    d = rng.randrange(1, c.n)
    q = M.affine_mul(c, d, (c.gx, c.gy))
    z = np.frombuffer(rng.randbytes(n * nb), dtype=np.uint8).reshape(n, nb).copy()
    sig, _, sok = cv.ecdsa_sign_prehash(M.i2b(c, d) * n, z, flags=0)
    assert sok.all() and cv.ecdsa_verify(z, sig, V.point_bytes(c, q), flags=E.SHARED_POINTS).all()
    builds = ctx.get_option(E.OPT_SHARED_TABLE_BUILDS)
    for key in (V.point_bytes(c, (q[0], (q[1] + 1) % c.p)), bytes(2 * nb), M.i2b(c, c.p) + M.i2b(c, q[1])):
        ok = cv.ecdsa_verify(z, sig, key, flags=E.SHARED_POINTS)  # no error, as the per-element call treats such a key
        assert not ok.any()
        assert not cv.ecdsa_verify(z, sig, key * n, flags=0).any()
    assert ctx.get_option(E.OPT_SHARED_TABLE_BUILDS) == builds
