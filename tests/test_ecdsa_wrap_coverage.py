"""The rows of tests/ecdsa_wrap_vectors.py are what they claim, checked on the CPU: x(R) >= n where a class says so, with R
recomputed from the row's inputs by the oracle; `second` of verify_check_kernel true or false as each class says; r + n carrying
exactly where it should; the class counts, the layout and the anchors.  Then every verify row through oracle/ecoracle.c, the
benchmark's CPU baseline, against the model's verdicts."""
from collections import Counter

import numpy as np
import pytest

import ecdsa_wrap_vectors as V
from oracle import ecmodel as M

CURVES = ["k256", "p256", "p384"]


def _rs(c, row):
    sig = row.inputs[1]
    return M.b2i(sig[:c.nbytes]), M.b2i(sig[c.nbytes:])


@pytest.mark.parametrize("cn", CURVES)
def test_anchors(cn):
    c, a = M.CURVES[cn], V.anchors(cn)
    on = lambda x: M.decompress(c, x, 0) is not None
    want = {"k256": (True, c.n + 2, c.p - 3, 1), "p256": (False, c.n + 3, c.p - 3, 0), "p384": (True, c.n + 2, c.p - 1, 0)}[cn]
    assert (a.n_on_curve, a.lo, a.hi, a.xs0) == want
    # nothing on the curve between the bounds and the anchors
    assert not any(on(x) for x in range(c.n + 1, a.lo)) and not any(on(x) for x in range(a.hi + 1, c.p))
    assert not any(on(x) for x in range(a.xs0)) and not any(on(x) for x in range(1, a.xs1))
    assert all(on(x) for x in a[1:]) and on(c.n) == a.n_on_curve
    assert abs(a.mid - (c.n + c.p) // 2) < 64
    assert len({P[0] for P in V.wrap_points(cn)}) == 3 and sorted(P[1] & 1 for P in V.wrap_points(cn)) == [0, 0, 0, 1, 1, 1]
    assert all(M.on_curve(c, P) for P in V.wrap_points(cn) + V.small_points(cn))


@pytest.mark.parametrize("kind", ["verify", "recover", "sign"])
@pytest.mark.parametrize("cn", CURVES)
def test_counts_and_layout(cn, kind):
    if kind == "sign":
        rs, fam = V.sign_rows(cn), V.sign_classes(cn)
        counts = dict(V.SIGN_COUNTS)
        if not V.anchors(cn).n_on_curve:
            counts["wrap"] += counts.pop("x_eq_n")
    else:
        rs, fam = V.rows(cn, kind), {"verify": V.VERIFY_CLASSES, "recover": V.RECOVER_CLASSES}[kind]
        counts = {"verify": V.VERIFY_COUNTS, "recover": V.RECOVER_COUNTS}[kind]
    assert len(rs) == V.N == sum(counts.values()) and V.class_counts(rs) == counts
    assert rs[0].cls == "wrap" and len(V.MIXED) == 13
    held = Counter()
    for lane in V.MIXED:
        mine = [rs[i].cls for i in range(lane, V.N, V.T)]
        assert len(mine) in (4, 5) and all(cls in fam for cls in mine)
        assert len(set(mine[:4])) >= (4 if kind != "sign" else 3), (lane, mine)         # sign: wrap or wrap_low_s may come twice
        good = [bool(rs[i].want[0] if kind == "sign" else rs[i].want) for i in range(lane, V.N, V.T)]
        assert True in good and False in good, (lane, mine)
        held.update(mine)
        assert ("k_bad" if kind == "sign" else "rejected") in [rs[i].cls for i in range(lane + 1, V.N, V.T)]
    assert all(held[cls] >= 6 for cls in fam), held
    # the whole pool is in use
    pool = {"verify": V.verify_pool, "recover": V.recover_pool, "sign": V.sign_pool}[kind](cn)
    assert {id(r) for r in rs} == {id(r) for cls in pool for r in pool[cls]}
    assert all(len(pool[cls]) == V.POOL and len({str(r.inputs if kind != "sign" else r[:6]) for r in pool[cls]}) == V.POOL for cls in set(fam))


@pytest.mark.parametrize("cn", CURVES)
def test_verify_rows_are_what_they_claim(cn):
    c, a = M.CURVES[cn], V.anchors(cn)
    n, p, W = c.n, c.p, 1 << (8 * c.nbytes)
    pool = V.verify_pool(cn)
    low = cn == "k256"
    small = {a.xs0, a.xs1}
    for cls in V.VERIFY_CLASSES + ("chord", "chord_bad", "rejected"):
        seen_second = set()
        for row in pool[cls]:
            r, s = _rs(c, row)
            assert row.cls == cls and row.want is (cls in V.VERIFY_VALID), (cls, row.want)
            if cls == "rejected":
                assert r == 0 or s == n
                continue
            assert 0 < s < n and not (low and s > n // 2)
            if cls == "r_is_x":
                assert n <= r == row.R[0] < p
                continue
            assert 0 < r < n
            A, B = V.sum_point(c, row)
            S = M.affine_add(c, A, B)
            seen_second.add(V.second(c, row))
            if cls in ("wrap", "wrap_ainf", "z_edge"):
                assert S == row.R and n <= S[0] < p and S[0] == r + n and V.second(c, row)
                assert (A is None) == (cls == "wrap_ainf")
                z = M.b2i(row.inputs[0])
                if cls == "wrap_ainf":
                    assert z in (0, n)
                if cls == "z_edge":
                    assert z in (n - 1, n + 1, W - 1)
            elif cls == "wrap_bad":
                assert n <= row.R[0] < p and abs(r + n - row.R[0]) == 1 and S is not None and S[0] % n != r
                assert V.second(c, row) == (r + n < p)
            elif cls == "no_p_check":
                assert S == row.R and S[0] in small and r + n == p + S[0] and r + n < W and not V.second(c, row)
            elif cls == "dropped_carry":
                assert S == row.R and S[0] in small and r + n == W + S[0] and (r + n) >> (8 * c.nbytes) == 1 and not V.second(c, row)
            elif cls == "first_small":
                assert S == row.R and S[0] == r and r + n < p and V.second(c, row)
        if cls == "wrap_bad":       # r + 1 at the largest x of P-384, p - 1, is the one row of the class whose r + n reaches p
            assert seen_second == ({True, False} if cn == "p384" else {True})
        if cls == "first_small":
            assert pool[cls][0].R[0] == a.xs1
    assert {row.R[0] for row in pool["wrap"]} == {a.lo, a.mid, a.hi} and {row.R for row in pool["wrap"]} == set(V.wrap_points(cn))
    assert {abs(_rs(c, row)[0] + n - row.R[0]) * (1 if _rs(c, row)[0] + n > row.R[0] else -1) for row in pool["wrap_bad"]} == {1, -1}
    assert {M.b2i(row.inputs[0]) for row in pool["wrap_ainf"]} == {0, n} and {M.b2i(row.inputs[0]) for row in pool["z_edge"]} == {n - 1, n + 1, W - 1}
    assert sum(r.want for r in V.verify_rows(cn)) == sum(V.VERIFY_COUNTS[cls] for cls in V.VERIFY_VALID)


@pytest.mark.parametrize("cn", CURVES)
def test_recover_rows_are_what_they_claim(cn):
    c, a = M.CURVES[cn], V.anchors(cn)
    n, p, W = c.n, c.p, 1 << (8 * c.nbytes)
    pool = V.recover_pool(cn)
    low = cn == "k256"
    for cls in V.RECOVER_CLASSES + ("chord", "chord_bad"):
        for i, row in enumerate(pool[cls]):
            r, s = _rs(c, row)
            z, _, recid = row.inputs
            assert 0 < r < n and 0 < s < n, cls                                     # none of them falls to the range check
            if cls in ("wrap", "wrong_parity", "high_s"):
                assert recid in (2, 3) and n <= row.R[0] == r + n < p
                Rr = row.R if (recid & 1) == (row.R[1] & 1) else M.affine_neg(c, row.R)
                key = V.key_for(c, Rr, r, s, z)
                assert (recid & 1 == row.R[1] & 1) == (cls != "wrong_parity")
                if cls == "high_s":
                    assert s > n // 2 and (row.want is None if low else row.want == key)
                    same_s = _rs(c, pool["wrap"][i])[1] == s                        # else (r, n - s) under R, which is (r, s) under -R
                    assert low or row.want == pool["wrap" if same_s else "wrong_parity"][i].want
                else:
                    assert not (low and s > n // 2) and row.want == key and row.want != V.key_for(c, M.affine_neg(c, Rr), r, s, z)
                    assert M.ecdsa_verify_prehashed(c, row.want, z, r, s, reject_high_s=low)
                continue
            if cls in ("chord", "chord_bad"):
                assert recid < 2 and row.want is not None
                continue
            assert row.want is None and (recid & 2 or cls == "recid_4_7") and not (low and s > n // 2)
            if cls == "ge_p":
                assert p <= r + n < W
            elif cls == "carry":
                assert r + n >= W
            elif cls == "no_root":
                assert r + n < p and M.decompress(c, r + n, 0) is None
            elif cls == "recid_4_7":
                assert 4 <= recid <= 7 and M.decompress(c, r + n, 0) is not None
            elif cls == "chord_bit1":
                assert recid in (2, 3)
    assert {row.R for row in pool["wrap"]} == set(V.wrap_points(cn)) and {row.inputs[2] for row in pool["wrap"]} == {2, 3}
    assert {M.b2i(row.inputs[0]) for row in pool["wrap"]} >= {0, n} and {row.inputs[2] for row in pool["recid_4_7"]} == {4, 5, 6, 7}
    assert {_rs(c, row)[0] + n - p for row in pool["ge_p"]} >= {0, a.xs0, a.xs1}
    assert all(_rs(c, row)[0] == 0 or _rs(c, row)[1] == n for row in pool["rejected"]) and all(row.want is None for row in pool["rejected"])


@pytest.mark.parametrize("cn", CURVES)
def test_sign_rows_are_what_they_claim(cn):
    c = M.CURVES[cn]
    n = c.n
    pool = V.sign_pool(cn)
    G = (c.gx, c.gy)
    # the model is the oracle's signing with R = k G supplied
    for k, low_s in ((3, False), (n - 2, True), (0x1234567 << 100, False), (n // 3, True), (0, False), (n, True)):
        R = M.affine_mul(c, k, G) or (0, 0)
        for z in (bytes(c.nbytes), b"\xff" * c.nbytes):
            assert V.sign_finish_model(c, 77, k, z, R, 0, low_s) == M.ecdsa_sign_prehashed(c, 77, k, z, normalize_s=low_s)
    for cls in ("wrap", "wrap_low_s"):
        ids = {f: set() for f in (0, V.LOW_S)}
        for row in pool[cls]:
            w0, w1 = row.want[0], row.want[V.LOW_S]
            assert n <= row.R[0] < c.p and not row.r_inf and w0[0] == w1[0] == row.R[0] - n
            assert w0[2] == 2 | (row.R[1] & 1) and (w0[1] > n // 2) == (cls == "wrap_low_s")
            assert w1 == (w0 if cls == "wrap" else (w0[0], n - w0[1], w0[2] ^ 1))
            ids[0].add(w0[2])
            ids[V.LOW_S].add(w1[2])
        assert ids == {0: {2, 3}, V.LOW_S: {2, 3}}
        assert {row.R for row in pool[cls]} == set(V.wrap_points(cn))
    for cls in ("x_eq_n", "s_zero", "r_inf", "k_bad"):
        for row in pool[cls]:
            assert row.want == {0: None, V.LOW_S: None} and 0 < row.d < n
            if cls == "x_eq_n":
                assert row.R[0] == n and M.on_curve(c, row.R) and 0 < row.k < n
            if cls == "s_zero":
                assert 0 < row.k < n and (M.b2i(row.z) + row.R[0] % n * row.d) % n == 0 and row.R[0] % n != 0
            if cls == "r_inf":
                assert row.r_inf == 1 and row.R == (0, 0) and 0 < row.k < n
            if cls == "k_bad":
                assert row.k in (0, n) and n <= row.R[0] < c.p
    assert len(pool["x_eq_n"]) == (V.POOL if V.anchors(cn).n_on_curve else 0)
    assert {row.R[1] & 1 for row in pool["x_eq_n"]} == ({0, 1} if pool["x_eq_n"] else set())
    assert {row.k for row in pool["k_bad"]} == {0, n} and {row.R[0] >= n for row in pool["s_zero"]} == {True, False}
    assert all(row.R[0] < n and row.want[0] is not None and row.want[0][2] < 2 for row in pool["control"])


@pytest.mark.parametrize("cn", CURVES)
def test_check_rows_are_what_they_claim(cn):
    c, a = M.CURVES[cn], V.anchors(cn)
    n, p, W = c.n, c.p, 1 << (8 * c.nbytes)
    pool = V.check_pool(cn)
    assert {(r.cls, r.kind) for r in pool} == {(cls, kind) for cls in V.CHECK_CLASSES for kind in V.CHECK_KINDS}
    for row in pool:
        S = M.affine_add(c, row.A, row.B)
        assert (S is None) == (row.kind == "opp")
        assert {"tangent": row.A == row.B, "chord": None not in (row.A, row.B) and row.A[0] != row.B[0], "a_inf": row.A is None and row.B is not None,
                "b_inf": row.B is None and row.A is not None, "opp": row.A == M.affine_neg(c, row.B)}[row.kind]
        x = S[0] if S else row.A[0]                 # opp: the x of the two operands, which a kernel without that arm would see
        second = row.r + n < p
        if row.cls in ("wrap", "ok_in_0"):
            assert n <= x == row.r + n and second and row.ok_in == (row.cls == "wrap") and row.want == (row.cls == "wrap" and row.kind != "opp")
        elif row.cls == "wrap_bad":
            assert n <= x and abs(row.r + n - x) == 1 and not row.want and second == (row.r + n != p)
        elif row.cls == "no_p_check":
            assert x in (a.xs0, a.xs1) and row.r + n == p + x and not second and not row.want
        elif row.cls == "dropped_carry":
            assert x in (a.xs0, a.xs1) and row.r + n == W + x and not second and not row.want
        elif row.cls == "first_small":
            assert 1 <= x == row.r and second and row.want == (row.kind != "opp")
        assert 0 < row.r < n
    assert V.check_rows(cn, 1)[0][:2] == ("wrap", "tangent") and len(pool) <= 257


@pytest.mark.parametrize("cn", CURVES)
def test_c_oracle_on_the_verify_rows(cn):
    """oracle/ecoracle.c, the benchmark's CPU baseline, gives the model's verdict on every row"""
    from oracle import coracle as CO
    c = M.CURVES[cn]
    rs = V.verify_rows(cn)
    col = lambda j: np.frombuffer(b"".join(r.inputs[j] for r in rs), dtype=np.uint8)
    got = CO.ecdsa_verify_batch(M.CURVE_IDS[cn], col(0), col(1), col(2), low_s=(cn == "k256"))
    assert not [(i, r.cls) for i, (g, r) in enumerate(zip(got, rs)) if bool(g) != r.want]
    assert int(got.sum()) == sum(V.VERIFY_COUNTS[cls] for cls in V.VERIFY_VALID)
