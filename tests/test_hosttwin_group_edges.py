"""The point formulas and masked additions one pair at a time on the host twin (tests/hosttwin/hosttwin_group.cpp over
tests/devtwin/group_ops.hpp), on the vectors of tests/group_edge_vectors.py: every result equals the integer model, and the
ECGPU_EXC_NOTE counters show, class by class, that the vectors reach the branch their class names - which is what lets
tests/test_gpu_group_edges.py claim that the same vectors reach those branches on the device, where the hook is empty.
k256::jac_add_mixed_neg, jac_double_neg and the add_affine forms of msm.hpp carry no sites: their evidence is the class and the
exact result."""
import functools
import os
import re

import pytest

import group_edge_vectors as V
from hosttwin_util import lib
from oracle import ecmodel as M
from related_point_hostwalks import CSRC, exc_counts, exc_reset

CURVE_OPS = [(cn, op) for cn in M.CURVES for op in V.ops_of(cn)]
HEADERS = ("jacobian.hpp", "msm.hpp", "mulfast_k256.hpp")


def sites_in_headers():
    names = set()
    for fn in HEADERS:
        with open(os.path.join(CSRC, fn)) as f:
            names.update(re.findall(r'ECGPU_EXC_NOTE\("([^"]+)"', f.read()))
    return names


def expected_sites(op, r):
    """the sites one pair of this class counts, once each"""
    if op not in V.SITES or r.branch is None:
        return set()
    prefix, inf = V.SITES[op]
    if r.branch in ("p_inf", "q_inf", "both_inf"):
        return {prefix + "." + inf[r.branch]}
    s = {prefix + "." + r.branch}
    if not r.z1 and op != "add_affine":
        s.add(prefix + "." + r.branch + ":z")
    return s


@functools.lru_cache(maxsize=None)
def run_op(cn, op):
    """outputs of every row, and per class the counters of its rows"""
    c = M.CURVES[cn]
    rs = V.rows(cn, op)
    out = V.run(lib().ht_pt_op, c, op, rs)
    by_cls = {}
    for r in rs:
        by_cls.setdefault(r.cls, []).append(r)
    counts = {}
    for cls, part in by_cls.items():
        exc_reset()
        V.run(lib().ht_pt_op, c, op, part)
        counts[cls] = exc_counts()
    exc_reset()
    return rs, out, by_cls, counts


@pytest.mark.parametrize("cn,op", CURVE_OPS)
def test_results_and_branches(cn, op):
    c = M.CURVES[cn]
    rs, out, by_cls, counts = run_op(cn, op)
    assert len(rs) <= V.MAX_CALL
    for i, r in enumerate(rs):
        err = V.check(c, op, r, out[i])
        assert err is None, (cn, op, i, r.cls, err, [hex(x) for x in r.p], [hex(x) for x in r.q], r.aux)
    for cls, part in by_cls.items():
        want = {}
        for r in part:
            for s in expected_sites(op, r):
                want[s] = want.get(s, 0) + 1
        # a formula that doubles or adds inside an exceptional branch may count the inner formula's sites too; none of the
        # three headers does, so the counters of a class are exactly the sites its rows name - and none for the ordinary,
        # near-miss, non-canonical and masked classes
        assert counts[cls] == want, (cn, op, cls, counts[cls], want)


def test_wave_layouts_cover_every_row():
    for cn, op in CURVE_OPS:
        rs = V.rows(cn, op)
        lay = V.layouts(rs)
        assert set(lay) == {"sorted", "interleaved", "single"}
        assert sorted(lay["interleaved"]) == list(range(len(rs)))
        assert set(lay["sorted"]) == set(range(len(rs))) and len(lay["sorted"]) % V.WAVE == 0
        for w in range(0, len(lay["sorted"]), V.WAVE):                       # a wave of the sorted layout holds one class
            assert len({rs[i].cls for i in lay["sorted"][w:w + V.WAVE]}) == 1
        inter = lay["interleaved"]
        for k in range(len(inter) - 1):                                      # neighbours differ in class while two classes are left
            if len({rs[i].cls for i in inter[k:]}) > 1:
                assert rs[inter[k]].cls != rs[inter[k + 1]].cls, (cn, op, k)
        exc = [i for i, r in enumerate(rs) if V.is_exceptional(r)]
        assert len(lay["single"]) == V.WAVE * len(exc)
        lanes = set()
        for n, i in enumerate(exc):
            wave = lay["single"][V.WAVE * n:V.WAVE * (n + 1)]
            odd = [k for k, j in enumerate(wave) if V.is_exceptional(rs[j])]
            assert odd == [(0, 31, 32, 63)[n % 4]] and wave[odd[0]] == i
            lanes.add(odd[0])
        assert lanes == {0, 31, 32, 63}, (cn, op, lanes)


def test_k256_jac_add_mixed_with_and_without_zr():
    """k256::jac_add_mixed as the kernels call it (zr = nullptr) and with the ratio, over the same rows: both exact (the per-op
    test), both counted at the same sites, and the same X, Y, Z words - except where the accumulator is doubled with a denominator
    that is not one: there the kernels' form doubles (x2, y2), Z3 = 2 y2, and the ratio form doubles p itself, Z3 = 2 Y1 Z1, two
    triples of one point (a ratio Z3 / Z1 of the first would cost an inversion)"""
    rs, with_zr, _, counts_zr = run_op("k256", "k_jac_add_mixed")
    rs2, without, _, counts = run_op("k256", "k_jac_add_mixed_nozr")
    assert rs2 is rs and counts == counts_zr
    assert any(v for cnt in counts.values() for k, v in cnt.items() if k == "k256.jac_add_mixed.same:z")
    differ = 0
    for i, r in enumerate(rs):
        if r.branch == "same" and not r.z1:
            if r.p[2] % M.K256.p != M.K256.p - 1:                            # (x, -y, -1) doubles to the triple that (x, y, 1) doubles to
                differ += 1
                assert (with_zr[i, :24] != without[i, :24]).any(), i
        else:
            assert (with_zr[i, :24] == without[i, :24]).all(), (i, r.cls)
        assert not without[i, 32:40].any()
    assert differ >= 30


def test_near_miss_rows_pass_the_prefilter():
    """H = U2 - U1 of a near-miss pair is +-t in the field's internal form, t small and not zero: a top word of 0 (or, for -t on
    secp256k1 and P-256 / P-384's p - t, of 2^32 - 1), so is_zero_fast has to run its exact test and say no"""
    seen = 0
    for cn, op in CURVE_OPS:
        c = M.CURVES[cn]
        spec = V.OPS[op]
        for r in V.rows(cn, op):
            if not r.cls.startswith("near:"):
                continue
            zz = lambda form, t: 1 if form == "aff" else t[2] * t[2] % c.p if form == "jac" else t[2]
            h = (r.Qa[0] - r.Pa[0]) * zz(spec.pform, r.p) * zz(spec.qform, r.q) % c.p
            hi = V.to_internal(c, h) % c.p
            t = int(r.cls.split(":")[1])
            assert hi == t % c.p and 0 < abs(t) < 64, (cn, op, r.cls, hex(hi))
            assert r.branch is None and r.Pa != r.Qa and r.Pa != M.affine_neg(c, r.Qa)
            seen += 1
    assert seen > 100


def test_every_site_of_the_three_headers_is_hit():
    hit = {cn: set() for cn in M.CURVES}
    for cn, op in CURVE_OPS:
        _, _, _, counts = run_op(cn, op)
        for cnt in counts.values():
            hit[cn].update(k for k, v in cnt.items() if v > 0)
    sites = sites_in_headers()
    assert len(sites) == 29, sorted(sites)
    generic = {s for s in sites if not s.startswith("k256.")}
    for cn in M.CURVES:
        want = sites if cn == "k256" else generic
        missing = want - hit[cn]
        print(cn, "sites hit:", " ".join(sorted(hit[cn] & want)))
        assert not missing, (cn, sorted(missing))


@pytest.mark.parametrize("name", sorted(V.RFC_STREAMS))
def test_rfc6979_streams_mix_rounds_in_a_wave(name):
    """on the model alone: what the device test needs from its inputs - lanes of one wave that leave the rejection loop of
    rfc6979::generate_k after 0, 1, 2 and >= 3 rejections (the round >= 2 arm runs while other lanes are done)"""
    _, q, ins, want = V.rfc6979_stream(name)
    count = V.RFC_STREAMS[name][5]
    assert len(ins) >= count and (len(ins) - count) % V.WAVE == 0
    rej = [r for _, r in want]
    assert V.wave_mixes_rounds(rej), name
    assert max(rej) >= 3
    assert all(0 < k < q for k, _ in want)
    print(name, len(ins), "inputs; rejections:", {r: rej.count(r) for r in sorted(set(rej))})


# rows per curve, summed over its ops, by the first word of the class (the rows of k256::jac_add_mixed count for both of its forms)
ROWS = {
    "k256": {"ordinary": 1732, "same": 384, "opp": 384, "p_inf": 56, "q_inf": 16, "both_inf": 8, "dbl_inf": 32, "near": 288, "noncanon": 314, "mask": 292},
    "p256": {"ordinary": 1008, "same": 240, "opp": 240, "p_inf": 16, "q_inf": 8, "both_inf": 4, "dbl_inf": 8, "near": 192, "mask": 288},
    "p384": {"ordinary": 1008, "same": 240, "opp": 240, "p_inf": 16, "q_inf": 8, "both_inf": 4, "dbl_inf": 8, "near": 192, "mask": 288},
}


def test_rows_per_class():
    """the rows are seeded, so their number is fixed: a few thousand per curve, every class on every curve that can have it, no op
    above the limit of one call"""
    for cn in M.CURVES:
        fam = {}
        for cls, n in V.class_counts(cn).items():
            fam[cls.split(":")[0]] = fam.get(cls.split(":")[0], 0) + n
        assert fam == ROWS[cn], (cn, fam)
        assert sum(fam.values()) == {"k256": 3506, "p256": 2004, "p384": 2004}[cn]
        assert all(len(V.rows(cn, op)) <= V.MAX_CALL for op in V.ops_of(cn))
