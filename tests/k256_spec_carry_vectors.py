"""Inputs for the speculative products of the k256 field products (csrc/fe_k256.hpp: mul, mul_add2, mul_add_sqr, sqr without
ECGPU_K256_BRANCHFREE) and a model of their column order that says which speculative sites an input raises.

A site is (form, column): the one product of that column that is issued without its carry addition; it is "raised" when adding
that product wraps the accumulator's low 64 bits.  The model (numpy, vectorised over the inputs) walks the columns in the order of
the C++ and keeps the exact 96-bit accumulator, as the device does once the rare branch has added the missing carry.

SITES lists the speculative columns per form; high columns are 9..14, low columns 0..7, the squaring's cross columns 6..10
(its columns 1 to 5 and 11 to 13 cannot carry at their first product: the model asserts that, as for every no-carry product)."""
import numpy as np

P = 2**256 - 2**32 - 977
TOP = 2**256 - 1
M32 = np.uint64(0xFFFFFFFF)
C_LO = np.uint64(977)
FORMS = ["mul", "sqr", "mul_add2", "mul_add_sqr"]
SITES = {
    "mul": [9, 10, 11, 12, 13, 1, 2, 3, 4, 5, 6, 7],
    "mul_add2": [9, 10, 11, 12, 13, 1, 2, 3, 4, 5, 6, 7],
    "mul_add_sqr": [9, 10, 11, 12, 13, 14, 0, 1, 2, 3, 4, 5, 6, 7],
    "sqr": [6, 7, 8, 9, 10],
}
EXPECT = {"mul": lambda a, b, e, f: a * b, "sqr": lambda a, b, e, f: a * a, "mul_add2": lambda a, b, e, f: a * b + e * f,
          "mul_add_sqr": lambda a, b, e, f: a * b + e * e}
SEARCH_SEED = 20240607
SEARCH_TRIALS = 400_000            # per form, well inside the 10^6 the search may use


def to_words(vals):
    raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u4").reshape(len(vals), 8).astype(np.uint32)


def from_words(arr):
    raw = np.ascontiguousarray(arr, dtype="<u4").tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(arr.shape[0])]


class Acc:
    """the 96-bit accumulator of n lanes: lo (64 bits) and hi (carry count)"""

    def __init__(self, n):
        self.lo = np.zeros(n, dtype=np.uint64)
        self.hi = np.zeros(n, dtype=np.uint64)

    def add(self, x, y):
        """+= x * y (32-bit words held in uint64); returns whether the low 64 bits wrapped"""
        p = x * y
        self.lo = self.lo + p
        c = self.lo < p
        self.hi = self.hi + c.astype(np.uint64)
        return c

    def pop(self):
        w = self.lo & M32
        self.lo = (self.lo >> np.uint64(32)) | (self.hi << np.uint64(32))
        self.hi = np.zeros_like(self.hi)
        return w


def _sqr2_terms(K, s, e, d):
    """the square's terms of column K of a * b + s^2 in the order of sqr2_column_terms (without s_(K-8) d_8)"""
    out = []
    if K % 2 == 1 and (K - 1) // 2 <= 6:
        out.append((s[(K - 1) // 2], e[(K + 1) // 2]))
    if K % 2 == 0 and K // 2 <= 7:
        out.append((s[K // 2], s[K // 2]))
    for i in range(7):
        if K - i >= i + 2 and K - i <= 7:
            out.append((s[i], d[K - i]))
    return out


def _column_terms(form, K, a, b, e, f, h, sq):
    """(x, y, kind) of column K in issue order; kind 'nc', 'spec' or 'pair'"""
    lo, hi = max(0, K - 7), min(K, 7)
    ab = [(a[i], b[K - i]) for i in range(lo, hi + 1)]
    terms = []
    if K < 8:
        terms.append((h[K], C_LO, "nc"))
    if form == "mul_add_sqr":
        s, ee, d = sq
        if K >= 8:
            terms.append((s[K - 8], d[8], "nc"))
        rest = ab + _sqr2_terms(K, s, ee, d)
        first = "nc" if K == 8 else "spec"
    else:
        rest = ab + ([(e[i], f[K - i]) for i in range(lo, hi + 1)] if form == "mul_add2" else [])
        if K == 8 or (K == 14 and form == "mul"):
            first = "nc"
        elif K == 0 or K == 14:
            first = "pair"
        else:
            first = "spec"
    terms.append(rest[0] + (first,))
    terms += [t + ("pair",) for t in rest[1:]]
    return terms


def raised(form, A, B, E=None, F=None):
    """{column: bool array} of the speculative sites raised by the (n, 8) uint32 operand arrays"""
    n = A.shape[0]
    a = [A[:, i].astype(np.uint64) for i in range(8)]
    flags = {}
    if form == "sqr":
        c = Acc(n)
        for K in range(1, 14):
            lo, hi = max(0, K - 7), (K - 1) // 2
            for m, i in enumerate(range(lo, hi + 1)):
                w = c.add(a[i], a[K - i])
                if m == 0 and K in SITES["sqr"]:
                    flags[K] = w
                elif m == 0:           # columns 1 to 5 and 11 to 13: no-carry products (mp32.hpp: sqr_cross_first_nc)
                    assert not w.any(), ("sqr", K, "a no-carry product carried")
            c.pop()
        return flags
    b = [B[:, i].astype(np.uint64) for i in range(8)]
    e = [E[:, i].astype(np.uint64) for i in range(8)] if E is not None else None
    f = [F[:, i].astype(np.uint64) for i in range(8)] if F is not None else None
    sq = None
    if form == "mul_add_sqr":
        s = e
        ee = [None] + [(s[j] << np.uint64(1)) & M32 for j in range(1, 8)]
        d = [None, None] + [((s[j] << np.uint64(1)) & M32) | (s[j - 1] >> np.uint64(31)) for j in range(2, 8)] + [s[7] >> np.uint64(31)]
        sq = (s, ee, d)
    h = [None] * 8
    c = Acc(n)
    for K in list(range(8, 15)) + list(range(0, 8)):
        if K == 0:
            h[7] = c.lo & M32
            c = Acc(n)
        for x, y, kind in _column_terms(form, K, a, b, e, f, h, sq):
            w = c.add(x, y)
            if kind == "spec":
                flags[K] = w
            elif kind == "nc":
                assert not w.any(), (form, K, "a no-carry product carried")
        if K >= 8:
            h[K - 8] = c.pop()
        else:
            c.pop()
    return flags


def flag_matrix(form, A, B, E, F):
    """(n, len(SITES[form])) bool array in the order of SITES[form]"""
    fl = raised(form, A, B, E, F)
    assert sorted(fl) == sorted(SITES[form]), (form, sorted(fl))
    return np.stack([fl[K] for K in SITES[form]], axis=1)


def flag_mask(form, A, B, E, F):
    """per input the bit mask the host twin reports: bit K for column K"""
    fl = raised(form, A, B, E, F)
    m = np.zeros(A.shape[0], dtype=np.uint32)
    for K, w in fl.items():
        m |= w.astype(np.uint32) << np.uint32(K)
    return m


STRUCT_WORDS = np.array([0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFF0000, 0x80000000, 0, 1, 2, 977, 0x10000], dtype=np.uint64)


def structured(g, n):
    """n x 8 words: per row a share of words near 2^32, the rest small, a few uniform"""
    hot = g.random((n, 1)) * 0.9 + 0.05
    r = g.random((n, 8))
    w = np.where(r < hot, STRUCT_WORDS[g.integers(0, 4, (n, 8))], STRUCT_WORDS[g.integers(5, len(STRUCT_WORDS), (n, 8))])
    w = np.where(g.random((n, 8)) < 0.05, g.integers(0, 2**32, (n, 8), dtype=np.uint64), w)
    return w.astype(np.uint32)


_ISO = {}


def isolating(form):
    """{column: (a, b, e, f) word rows} raising that site and no other, found by a seeded search over structured words, and
    {column: rows} raising that site at all (possibly with others) for the sites the search could not isolate"""
    if form in _ISO:
        return _ISO[form]
    g = np.random.default_rng(SEARCH_SEED + FORMS.index(form))
    iso, anyhit = {}, {}
    batch = 50_000
    for _ in range(SEARCH_TRIALS // batch):
        ops = [structured(g, batch) for _ in range(4)]
        if g.random() < 0.5:           # related operands: squares and shared factors drive the same columns
            ops[1] = ops[0].copy()
        fm = flag_matrix(form, *ops)
        cnt = fm.sum(axis=1)
        for j, K in enumerate(SITES[form]):
            if K not in iso:
                idx = np.nonzero(fm[:, j] & (cnt == 1))[0]
                if len(idx):
                    iso[K] = tuple(o[idx[0]].copy() for o in ops)
            if K not in anyhit:
                idx = np.nonzero(fm[:, j])[0]
                if len(idx):
                    anyhit[K] = tuple(o[idx[0]].copy() for o in ops)
        if len(iso) == len(SITES[form]):
            break
    _ISO[form] = (iso, anyhit)
    return _ISO[form]


def edge_rows():
    """(a, b, e, f) integer rows: all ones, and the column-maximising pairs and quads of field_edge_vectors"""
    import field_edge_vectors as V
    rows = [(TOP, TOP, TOP, TOP)]
    rows += [(x, y, y, x) for x, y in V.pairs(400)]
    rows += [q for q in V.quads(400)]
    return rows


def vector_set(form):
    """the operands (four (n, 8) uint32 arrays) of cases (a) to (c) for one form, and the index ranges of each part"""
    rows = edge_rows()
    ops = [to_words([r[k] for r in rows]) for k in range(4)]
    iso, anyhit = isolating(form)
    extra = [iso[K] for K in SITES[form] if K in iso] + [anyhit[K] for K in SITES[form] if K not in iso and K in anyhit]
    if extra:
        ops = [np.concatenate([o, np.stack([x[k] for x in extra])]) for k, o in enumerate(ops)]
    return ops


def raising_row(form):
    """one operand row that raises at least one site of the form (all ones does for every form)"""
    one = to_words([TOP])
    assert flag_mask(form, one, one, one, one)[0] != 0
    return one[0]
