"""Shared points on the CPU: the host build of csrc/sharedbase.hpp (tests/hosttwin/hosttwin_shared.cpp) against the oracle's affine
model.  The builder's two stages give the table the device kernels read; mul_shared_one is walked over tables built that way, on both
accumulators, for unrelated and related points, the edge scalars and combinations that are the identity; the ECGPU_EXC_NOTE counters
show that the related points really entered the exceptional branches of the additions."""
import pytest

import shared_points_vectors as V
from hosttwin_util import buf, lib, outbuf
from oracle import ecmodel as M
from related_point_hostwalks import exc_counts, exc_reset

CURVES = [("k256", 0), ("p256", 1), ("p384", 2)]


def _table(c, cid, wb, point):
    entries = V.nwin(c, wb) * (1 << (wb - 1))
    assert lib().ht_shared_windows(cid, wb) == V.nwin(c, wb)
    out = outbuf(entries * 2 * c.nbytes)
    assert lib().ht_shared_table(cid, wb, buf(V.point_bytes(c, point)), out) == entries
    return bytes(out)


def _mul(c, cid, wb, jacobian, pts, rows):
    """rows: one list of len(pts) scalars per element -> list of affine points (None = the identity)"""
    nb = c.nbytes
    sc = b"".join(M.i2b(c, k) for row in rows for k in row)
    out, inf = outbuf(len(rows) * 2 * nb), outbuf(len(rows))
    rc = lib().ht_shared_mul(cid, wb, jacobian, buf(b"".join(V.point_bytes(c, p) for p in pts)), len(pts), buf(sc), out, inf, len(rows))
    assert rc == 0
    res = []
    for i in range(len(rows)):
        xy = bytes(out[i * 2 * nb:(i + 1) * 2 * nb])
        if inf[i]:
            assert xy == bytes(2 * nb)
            res.append(None)
        else:
            res.append((M.b2i(xy[:nb]), M.b2i(xy[nb:])))
    return res


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("wb", [5, 8])
def test_table_entries(name, cid, wb):
    c = M.CURVES[name]
    h = V.points(c, 1, start=7)[0]
    tab = _table(c, cid, wb, h)
    nb, per = c.nbytes, 1 << (wb - 1)
    for d, j in V.table_entries(c, wb):
        e = j * per + d - 1
        want = M.affine_mul(c, d << (wb * j), h)
        assert tab[e * 2 * nb:(e + 1) * 2 * nb] == V.point_bytes(c, want), (d, j)


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("wb", [5, 8])
@pytest.mark.parametrize("terms", [1, 2, 3, 8])
def test_unrelated_points_and_edge_scalars(name, cid, wb, terms):
    c = M.CURVES[name]
    pts = V.points(c, terms, start=11)
    edge = V.edge_scalars(c, wb)
    # every edge scalar in every term's place, the other terms on ordinary scalars; then rows of edge scalars only
    ordinary = [int.from_bytes(bytes([17 + t] * c.nbytes), "big") % c.n for t in range(terms)]
    rows = [[e if t == i % terms else ordinary[t] for t in range(terms)] for i, e in enumerate(edge)]
    rows += [[edge[(i + t) % len(edge)] for t in range(terms)] for i in range(len(edge))]
    for jacobian in (0, 1):
        got = _mul(c, cid, wb, jacobian, pts, rows)
        for row, g in zip(rows, got):
            assert g == V.combination(c, row, pts), (jacobian, row)


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("wb", [5, 8])
def test_related_points(name, cid, wb):
    c = M.CURVES[name]
    k = 0x1234567 << 40 | 0x89AB
    for set_name, pts in V.related_sets(c).items():
        edge = V.edge_scalars(c, wb)
        rows = [[edge[(i + 3 * t) % len(edge)] for t in range(len(pts))] for i in range(len(edge))]
        rows += [[(k * (t + 1) + i) % c.n for t in range(len(pts))] for i in range(4)]
        if set_name in ("H,H", "H,-H", "H,2H", "H,O"):
            sums = V.identity_sum_rows(c, set_name, k)
            for row in sums:
                assert V.combination(c, row, pts) is None
            rows += sums
        for jacobian in (0, 1):
            got = _mul(c, cid, wb, jacobian, pts, rows)
            for row, g in zip(rows, got):
                assert g == V.combination(c, row, pts), (set_name, jacobian, row)


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("terms", [3, 8])
def test_exceptional_branches_are_entered(name, cid, terms):
    """equal points and the rows of branch_rows: the same point, the opposite point and the accumulator back at infinity"""
    c = M.CURVES[name]
    h = V.points(c, 1, start=23)[0]
    pts = [h] * terms
    rows = V.branch_rows(c, terms)
    for jacobian, site in ((0, "msm.xyzz_add_mixed"), (1, "jac.add_mixed")):
        exc_reset()
        got = _mul(c, cid, 8, jacobian, pts, rows)
        counts = exc_counts()
        for row, g in zip(rows, got):
            assert g == V.combination(c, row, pts), (jacobian, row)
        for branch in ("same", "opp", "inf"):
            assert counts.get(site + "." + branch, 0) > 0, (site, branch, counts)
        # an accumulator that is no longer one affine entry met its negative: the shortcut for the second addition was not what resolved it
        assert counts.get(site + ".opp:z", 0) > 0, counts
        if jacobian:
            assert counts.get("jac.add_affine.same", 0) > 0 and counts.get("jac.add_affine.opp", 0) > 0, counts
