"""Inputs shared by the shared-points tests (ECGPU_SHARED_POINTS): edge scalars, related point sets and scalar rows that drive the
one accumulator of the multi-table loop into every exceptional branch of its additions.  Expected values come from the oracle
(oracle/ecmodel.py), never from the code under test."""
from oracle import ecmodel as M
from oracle import synth


def nwin(c, wb):
    bits = 8 * c.nbytes
    return (bits + wb - 1) // wb + (1 if bits % wb == 0 else 0)


def edge_scalars(c, wb):
    """0, 1, n - 1, n, (n +- 1) / 2 and, at the first, second and last window boundary, 2^(wb j - 1) and 2^(wb j) - 1"""
    n = c.n
    out = [0, 1, n - 1, n, (n - 1) // 2, (n + 1) // 2]
    last = (8 * c.nbytes - 1) // wb
    for j in (1, 2, last):
        out += [1 << (wb * j - 1), (1 << (wb * j)) - 1]
    return out


def table_entries(c, wb, through_scalars=False):
    """(d, j) for d in {1, 2, 16, 17, 2^(wb-1)} and j in {0, 1, last}: entry T[j][d-1] = d 2^(wb j) H.  `last` is the table's last
    window (a carry window where wb divides the width), or, for a test that reaches the entries through scalars d 2^(wb j), the last
    window that holds bits of a scalar.  (A 5-bit window has 16 entries: d = 17 does not exist there.)
    Through a scalar, d = 2^(wb-1) recodes to the digit -2^(wb-1) with a carry: it still reads T[j][2^(wb-1) - 1], negated, and
    T[j+1][0] with it.  In the top window that scalar, 2^(bits - 1), is above n / 2 and would be folded to n - k, which reads other
    entries altogether: there the largest digit that is reached as named is 2^(wb-1) - 1."""
    half = 1 << (wb - 1)
    if not through_scalars:
        return [(d, j) for j in (0, 1, nwin(c, wb) - 1) for d in sorted({1, 2, 16, 17, half}) if d <= half]
    last = (8 * c.nbytes - 1) // wb
    out = [(d, j) for j in (0, 1) for d in sorted({1, 2, 16, 17, half})] + [(d, last) for d in sorted({1, 2, 16, 17, half - 1})]
    assert all((d << (wb * j)) <= c.n // 2 for d, j in out)          # none is folded
    return out


def points(c, count, start=0):
    return synth.points(c, count, start=start)


def related_sets(c):
    """name -> list of points (None = the identity): H with itself, its negative, its double and the identity; longer sets around them"""
    h, p, q = synth.points(c, 3, start=40)
    neg = lambda a: M.affine_neg(c, a)
    dbl = lambda a: M.affine_add(c, a, a)
    return {
        "H,H": [h, h],
        "H,-H": [h, neg(h)],
        "H,2H": [h, dbl(h)],
        "H,O": [h, None],
        "H,H,H": [h, h, h],
        "H,-H,2H": [h, neg(h), dbl(h)],
        "8 related": [h, neg(h), dbl(h), h, None, p, neg(p), dbl(p)],
        "8 mixed": [h, p, q, neg(q), None, dbl(q), h, p],
    }


def branch_rows(c, terms):
    """scalar rows for `terms` equal points (H, H, ...), terms >= 3, that reach, in this order of terms: the doubling of the first entry
    (1, 1: add_affine on the same point), the mixed addition of the accumulator's own value (.., 2: same), of its negative (.., n - 2:
    opposite, the identity comes out) and of anything after that (the accumulator at infinity again)."""
    n = c.n
    pad = [0] * (terms - 3)
    return [[1, 1, 2] + pad, [1, 1, n - 2] + pad, [1, n - 1, 5] + pad, [2, n - 1, n - 1] + pad, [3, 5, n - 8] + pad]


def identity_sum_rows(c, name, k):
    """scalar rows whose combination over related_sets(c)[name] is the identity"""
    n = c.n
    return {"H,H": [[k, n - k], [1, n - 1], [0, 0]], "H,-H": [[k, k], [1, 1], [n - 1, n - 1]], "H,2H": [[(2 * k) % n, n - k], [2, n - 1], [n - 2, 1]],
            "H,O": [[0, k], [n, 1]]}[name]


def combination(c, ks, pts):
    """sum_j ks[j] pts[j] in the affine model (None = the identity)"""
    acc = None
    for k, p in zip(ks, pts):
        acc = M.affine_add(c, acc, M.affine_mul(c, k, p))
    return acc


def point_bytes(c, p):
    return bytes(2 * c.nbytes) if p is None else M.i2b(c, p[0]) + M.i2b(c, p[1])
