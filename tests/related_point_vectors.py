"""Inputs whose points are RELATED: every point of a call is a known multiple m B of one base point B, so that the partial sums
of the multi-point schedules (two-term kernels, shared-doubling many-term schedule, bucket method) meet the exceptional cases of
the incomplete addition formulas - accumulator at infinity, the same point, opposite points - and the expected result is

    sum_i k_i (m_i B) = (sum_i k_i m_i mod n) B

from Python integers and ONE oracle.ecmodel.affine_mul, however many terms there are.  Nothing here depends on the library or on
its host build; the only curve arithmetic is the big-integer model's.

- Family(curve, base): B = G or oracle.synth.point, multipliers (each with both signs)
    1 .. 16                         table entries of one term equal another term's
    lambda j, lambda^2 j (k256)     the two GLV halves of different terms; MSM half-terms of different terms in one bucket
    2^4, 2^5, 2^15, 2^16, 2^18, 2^19   a digit of one term one window up equals a digit of another
    (n + 1) / 2, (n - 1) / 2        2 P_j = +-P_i: a doubling lands on another term's table entry
- combos(family, pattern, terms, count, seed): `count` combinations of `terms` terms, each a pair (ks, ms) of scalars in [0, n) and
  multipliers mod n (0 = the identity point), for the patterns
    "random"   scalars uniform in [0, n)
    "small"    |k| < 2^10, both signs (n - k)
    "equal"    all scalars equal, or equal up to sign; every few combinations all points equal too, or the groups of the many-term
               schedule given equal partial sums (the fold meets P + P)
    "collide"  crafted: k_0 = R a_0 + d_0, k_1 = R a_1 + d_1 with R (a_0 m_0 + a_1 m_1) + d_0 m_0 = +-d_1 m_1, found by a search over
               a, d, m and checked on walk_events; shifted up by a random number of windows so that it happens in mid loop
    "cancel"   the whole sum is the identity: pairwise, at the last addition only, by a solved last scalar, between the groups
    "awkward"  0, 1, n - 1, (n +- 1) / 2, 2^128 +- 1 and identity points mixed in
- expected(curve, ks, ms, base): affine bytes and the infinity flag of the sum
- walk_events: an integer model of a window loop (which additions find the accumulator at infinity / equal / opposite), used to
  select crafted inputs - never as the reference for a result."""
import functools
import random

import numpy as np

from oracle import ecmodel as M
from oracle import synth

CURVE_IDS = {"k256": 0, "p256": 1, "p384": 2}
PATTERNS = ("random", "small", "equal", "collide", "cancel", "awkward")
SHIFT_BITS = (4, 5, 15, 16, 18, 19)
SMALL = 1 << 10
SLOTS = 16                                   # terms per group of the many-term schedule (17 terms are cut 9 + 8)


def lam(c):
    """lambda of the curve's endomorphism, or None"""
    return M.K256_LAMBDA if c is M.K256 else None


def base_point(c, which):
    """which = "G": the generator; "S": a synthetic point with no known relation to G"""
    return (c.gx, c.gy) if which == "G" else synth.point(c, 0, seed=0x5E1A7ED)


class Family:
    """{ m B }: .mult the multipliers mod n (both signs), .ints the ones that are small integers (signed), .point(m) the affine point
    (None for m = 0)."""

    def __init__(self, c, which="G"):
        self.c, self.which, self.base = c, which, base_point(c, which)
        n = c.n
        small = list(range(1, 17)) + [1 << b for b in SHIFT_BITS if (1 << b) > 16]
        pos = small + [(n + 1) // 2, (n - 1) // 2]
        self.ints = [s * m for m in small for s in (1, -1)]
        self.lams = []
        L = lam(c)
        if L is not None:
            x, y = self.base
            assert M.affine_mul(c, L, self.base) == (M.K256_BETA * x % c.p, y), "lambda and beta of the model do not belong together"
            for j in range(1, 17):
                pos += [L * j % n, L * L * j % n]
            self.lams = [L, L * L % n]
        self._pts = {}
        for m in pos:
            P = M.affine_mul(c, m, self.base)
            self._pts[m] = P
            self._pts[n - m] = (P[0], c.p - P[1])
        self.mult = sorted(self._pts)

    def has(self, m):
        return m % self.c.n in self._pts

    def point(self, m):
        m %= self.c.n
        return None if m == 0 else self._pts[m]


@functools.lru_cache(maxsize=None)
def family(curve_name, which="G"):
    return Family(M.CURVES[curve_name], which)


def expected(c, ks, ms, base):
    """(x || y bytes, infinity flag) of sum_i k_i (m_i base): one scalar multiplication of the integer sum"""
    s = sum(k * m for k, m in zip(ks, ms)) % c.n
    if s == 0:
        return bytes(2 * c.nbytes), 1
    P = M.affine_mul(c, s, base)
    return M.i2b(c, P[0]) + M.i2b(c, P[1]), 0


def scalar_bytes(c, ks):
    return b"".join(int(k).to_bytes(c.nbytes, "big") for k in ks)


def point_bytes(fam, ms, proj_rng=None):
    """affine x || y (zeros: the identity) or, with proj_rng, homogeneous X || Y || Z with a random Z (identity (0 : 1 : 0))"""
    c = fam.c
    out = []
    for m in ms:
        P = fam.point(m)
        if proj_rng is None:
            out.append(bytes(2 * c.nbytes) if P is None else M.i2b(c, P[0]) + M.i2b(c, P[1]))
        elif P is None:
            out.append(M.proj_bytes(c, M.IDENTITY))
        else:
            z = proj_rng.randrange(1, c.p)
            out.append(M.proj_bytes(c, (P[0] * z % c.p, P[1] * z % c.p, z)))
    return b"".join(out)


# ---- integer model of a window loop -------------------------------------------------------------------------------------------
def signed_digits(k, wbits):
    """digits of k >= 0 in [-2^(w-1), 2^(w-1)), least significant first: the recoding of every throughput schedule"""
    R, out = 1 << wbits, []
    while k:
        d = k & (R - 1)
        if d >= R >> 1:
            d -= R
        out.append(d)
        k = (k - d) >> wbits
    return out


def half_terms(c, k, m):
    """the (signed scalar, multiplier) pairs a schedule walks for the term (k, m): secp256k1 its two GLV halves (the model's own
    decomposition), P-256 / P-384 min(k, n - k) with the sign on the point"""
    n = c.n
    k %= n
    if c is M.K256:
        r1, r2 = M.k256_decompose_scalar(k)
        sg = lambda r: r - n if M.k256_is_high(r) else r
        return [(sg(r1), m), (sg(r2), m * M.K256_LAMBDA % n)]
    return [(k - n if n - k < k else k, m)]


def walk_events(c, ks, ms, wbits=4):
    """Counts, over one shared-doubling window loop that adds the terms in order at every position, the additions that find the
    accumulator at infinity ("inf"), equal to the addend ("same") or opposite to it ("opp"), and the last two again while the
    accumulator's Z has left 1 ("same_z", "opp_z": a doubling or a regular addition came before)."""
    n = c.n
    halves = [h for k, m in zip(ks, ms) if m % n for h in half_terms(c, k, m)]
    digs = [(signed_digits(abs(k), wbits), 1 if k >= 0 else -1, m) for k, m in halves]
    npos = max([len(d) for d, _, _ in digs] + [0])
    ev = {"inf": 0, "same": 0, "opp": 0, "same_z": 0, "opp_z": 0}
    acc, z_one = 0, True
    for j in range(npos - 1, -1, -1):
        if j != npos - 1 and acc:
            acc, z_one = (acc << wbits) % n, False
        for d, s, m in digs:
            if j >= len(d) or d[j] == 0:
                continue
            add = s * d[j] * m % n
            if acc == 0:
                ev["inf"] += 1
                acc, z_one = add, True
                continue
            if acc == add:
                ev["same"] += 1
                ev["same_z"] += not z_one
            elif (acc + add) % n == 0:
                ev["opp"] += 1
                ev["opp_z"] += not z_one
            acc, z_one = (acc + add) % n, False
    return ev


def craft_collision(fam, rng, wbits=4, want="same", z_free=True, with_lambda=True, first=None):
    """Two terms (k_0, m_0), (k_1, m_1) whose window loop of width `wbits` meets `want` ("same" / "opp") when it adds the digit of
    term 1, with Z != 1 if z_free: R (a_0 m_0 + a_1 m_1) + d_0 m_0 = +-d_1 m_1 over the integers, by a search over a, d, m.  On
    secp256k1 every other result moves the pair onto the lambda halves.  Returns (ks, ms, shift): scalars mod n, and the number of
    window positions below the collision (free for other terms' digits).  first: the multiplier of term 0, if it is prescribed (no
    lambda form then)."""
    c, n, R = fam.c, fam.c.n, 1 << wbits
    e = 1 if want == "same" else -1
    key = want + ("_z" if z_free else "")
    for _ in range(20000):
        m0, m1 = (rng.choice(fam.ints) if first is None else first), rng.choice(fam.ints)
        d0, d1 = rng.randrange(-(R // 2) + 1, R // 2), rng.randrange(1, R // 2) * rng.choice((1, -1))
        if m0 % 2 and rng.random() < 0.5:                         # solve R | e d_1 m_1 - d_0 m_0 for d_0 (wide windows: chance alone is too rare)
            d0 = (e * d1 * m1 * pow(m0, -1, R)) % R
            d0 = d0 - R if d0 >= R // 2 else d0
        v = e * d1 * m1 - d0 * m0
        if v % R or (z_free and v == 0):
            continue
        T = v // R                                                # a_0 m_0 + a_1 m_1
        a1 = rng.randrange(-40, 41) if rng.random() < 0.7 else rng.randrange(-(1 << 40), 1 << 40)
        if (T - a1 * m1) % m0:
            continue
        a0 = (T - a1 * m1) // m0
        k0, k1 = R * a0 + d0, R * a1 + d1
        if k0 == 0 or max(abs(k0), abs(k1)) >> 100:
            continue
        shift = rng.randrange(0, 6) if wbits <= 5 else rng.randrange(0, 2)
        k0, k1 = k0 << (wbits * shift), k1 << (wbits * shift)
        if shift:                                                 # digits below the collision: they do not reach it (|low| < R^shift / 4)
            k0 += rng.randrange(-(1 << (wbits * shift - 2)), 1 << (wbits * shift - 2))
            k1 += rng.randrange(-(1 << (wbits * shift - 2)), 1 << (wbits * shift - 2))
        ks, ms = [k0 % n, k1 % n], [m0 % n, m1 % n]
        if with_lambda and first is None and fam.lams and rng.random() < 0.5:       # (k_0, lambda m_0) and (lambda k_1, m_1): the same two group elements
            L = fam.lams[0]
            if fam.has(m0 * L):
                ks, ms = [k0 % n, k1 * L % n], [m0 * L % n, m1 % n]
        if walk_events(c, ks, ms, wbits)[key] >= 1:
            return ks, ms, shift
    raise RuntimeError("no crafted collision found")


def group_sizes(terms):
    """how the many-term schedule cuts a combination when every lane has work: ceil(terms / 16) balanced groups"""
    gpc = -(-terms // SLOTS)
    g = -(-terms // gpc)
    return [min(g, terms - t0) for t0 in range(0, terms, g)]


# ---- the patterns ---------------------------------------------------------------------------------------------------------------
def _signed_small(rng, n):
    k = rng.randrange(1, SMALL)
    return k if rng.random() < 0.5 else n - k


def _grouped(fam, rng, terms, sign_of_group):
    """every group of the many-term schedule gets the same r terms (r = the smallest group), times sign_of_group(g), and zero
    scalars / identity points for the rest: the groups' partial sums are equal or opposite when the fold adds them"""
    n = fam.c.n
    sizes = group_sizes(terms)
    r = min(sizes)
    core = [(rng.randrange(1, n) if rng.random() < 0.5 else _signed_small(rng, n), rng.choice(fam.mult)) for _ in range(r)]
    ks, ms = [], []
    for gi, sz in enumerate(sizes):
        s = sign_of_group(gi)
        for t in range(sz):
            if t < r:
                ks.append(core[t][0] * s % n)
                ms.append(core[t][1])
            else:
                ks.append(0 if t % 2 else rng.randrange(n))
                ms.append(rng.choice(fam.mult) if t % 2 else 0)
    return ks, ms


def combos(fam, pattern, terms, count, seed, wbits=4):
    """`count` combinations (ks, ms) of `terms` terms, deterministic in (family, pattern, terms, seed, wbits)"""
    c, n = fam.c, fam.c.n
    rng = random.Random("%s/%s/%s/%d/%d/%d" % (c.name, fam.which, pattern, terms, seed, wbits))
    pick = lambda: rng.choice(fam.mult)
    out = []
    for i in range(count):
        if pattern == "random":
            ks, ms = [rng.randrange(n) for _ in range(terms)], [pick() for _ in range(terms)]
        elif pattern == "small":
            ks, ms = [_signed_small(rng, n) for _ in range(terms)], [pick() for _ in range(terms)]
            if i % 3 == 0:                                         # small multiples of B only: the partial sums walk over the table entries
                ms = [rng.choice(fam.ints[:32]) % n for _ in range(terms)]
        elif pattern == "equal":
            k0 = rng.randrange(1, n) if i % 2 else rng.randrange(1, SMALL)
            up_to_sign = i % 4 >= 2
            ks = [k0 if not up_to_sign or rng.random() < 0.5 else n - k0 for _ in range(terms)]
            ms = [pick() for _ in range(terms)]
            if i % 3 == 1:                                         # the same point everywhere (up to sign: m, -m)
                m = pick()
                ms = [m if not up_to_sign or rng.random() < 0.5 else n - m for _ in range(terms)]
            elif i % 3 == 2 and terms > SLOTS:
                ks, ms = _grouped(fam, rng, terms, lambda g: 1)
        elif pattern == "collide":
            if terms == 1:
                ks, ms = [_signed_small(rng, n)], [pick()]
            else:
                want = "same" if i % 2 == 0 else "opp"
                k2, m2, shift = craft_collision(fam, rng, wbits, want, z_free=(i % 8 < 6))
                # the pair sits in two neighbouring terms of the first group; the others only have digits below the collision, or none
                at = rng.randrange(0, group_sizes(terms)[0] - 1)
                ks, ms = [], []
                for t in range(terms):
                    if t in (at, at + 1):
                        ks.append(k2[t - at])
                        ms.append(m2[t - at])
                    elif shift and t > at + 1 and rng.random() < 0.5:
                        lim = 1 << (wbits * shift - 2)
                        ks.append(rng.randrange(-lim, lim) % n)
                        ms.append(pick())
                    elif rng.random() < 0.5:
                        ks.append(0)
                        ms.append(pick())
                    else:
                        ks.append(rng.randrange(n))
                        ms.append(0)
        elif pattern == "cancel":
            v = i % 4
            if terms == 1:
                ks, ms = [0], [pick()]
            elif v == 0:                                           # pairwise: (k, m), (n - k, m) or (k, m), (k, -m); an odd last term is zero
                ks, ms = [], []
                for t in range(0, terms - 1, 2):
                    k, m = (rng.randrange(1, n) if rng.random() < 0.5 else _signed_small(rng, n)), pick()
                    if rng.random() < 0.5:
                        ks += [k, n - k]
                        ms += [m, m]
                    else:
                        ks += [k, k]
                        ms += [m, n - m]
                if terms % 2:
                    ks.append(0)
                    ms.append(pick())
            elif v == 1:                                           # only the last addition cancels: k_0 = m_1 t, k_1 = -m_0 t over the integers
                m0, m1 = rng.choice(fam.ints), rng.choice(fam.ints)
                t = rng.randrange(1, 1 << rng.choice((8, 40, 100)))
                ks = [0] * (terms - 2) + [m1 * t % n, -m0 * t % n]
                ms = [pick() for _ in range(terms - 2)] + [m0 % n, m1 % n]
            elif v == 2 or terms <= SLOTS:                         # the last scalar solves sum k_i m_i = 0
                ks, ms = [rng.randrange(n) for _ in range(terms)], [pick() for _ in range(terms)]
                s = sum(k * m for k, m in zip(ks[:-1], ms[:-1])) % n
                ks[-1] = -s * pow(ms[-1], -1, n) % n
            else:                                                  # the groups' partial sums cancel in the fold, two by two
                ks, ms = _grouped(fam, rng, terms, lambda g: 1 if g % 2 == 0 else -1)
                sizes = group_sizes(terms)
                if len(sizes) % 2:                                 # an odd last group contributes nothing
                    ks[-sizes[-1]:] = [0] * sizes[-1]
        elif pattern == "awkward":
            pool = [0, 1, 2, n - 1, n - 2, (n - 1) // 2, (n + 1) // 2, (1 << 128) - 1, (1 << 128) + 1, n - (1 << 128), 1 << (8 * c.nbytes - 1)]
            ks = [rng.choice(pool) % n for _ in range(terms)]
            ms = [0 if rng.random() < 0.15 else pick() for _ in range(terms)]
            if terms > SLOTS and i % 2 == 0:                       # a later group of nothing but zero scalars / identity points: the fold adds infinity
                sizes = group_sizes(terms)
                gi = rng.randrange(1, len(sizes))
                for t in range(sum(sizes[:gi]), sum(sizes[:gi + 1])):
                    if t % 2:
                        ks[t] = 0
                    else:
                        ms[t] = 0
        else:
            raise ValueError(pattern)
        assert len(ks) == terms and len(ms) == terms, (pattern, terms, len(ks))
        out.append((ks, ms))
    return out


def flatten(cs):
    """combinations -> the flat scalar and multiplier lists of one batched call"""
    return [k for ks, _ in cs for k in ks], [m for _, ms in cs for m in ms]


# ---- large sums for the bucket method --------------------------------------------------------------------------------------------
MSM_DESIGNS = ("same_point", "alternating", "walk_random", "walk_small", "window_shift", "cancel")


def msm_inputs(fam, design, n, seed, wbits=16):
    """(scalars (n, NB) uint8, points (n, 2 NB) uint8, (expected x || y bytes, infinity flag)) of one n-term sum over the family:
    "same_point"    every point B, every scalar the same k: whatever the sort order, each bucket run meets B + B at its second entry
    "alternating"   points B, -B, B, .. and one scalar: infinity, restart and cancellation in every run
    "walk_random" / "walk_small"   points cycling through {+-1 .. +-8} B (secp256k1: and {+-1 .. +-8} lambda B), scalars random / below
                    2^10 with both signs: the partial sums are a short random walk over the very multiples that are added
    "window_shift"  crafted pairs for `wbits`-bit windows over the multipliers 2^15 .. 2^19 and 1 .. 16: bucket j of one window and
                    bucket j' of the next are related, for the running sums and the Horner step
    "cancel"        "walk_random" with the last scalar solved so that the whole sum is the identity
    Scalars and points are drawn from pools of a few thousand values, so the expected sum is a sum over the distinct (scalar,
    multiplier) pairs with their counts."""
    c, nn = fam.c, fam.c.n
    rng = random.Random("msm/%s/%s/%s/%d/%d/%d" % (c.name, fam.which, design, n, seed, wbits))
    nprng = np.random.default_rng(rng.randrange(1 << 32))
    walk = [s * j % nn for j in range(1, 9) for s in (1, -1)]
    if fam.lams:
        walk += [s * j * fam.lams[0] % nn for j in range(1, 9) for s in (1, -1)]
    if design in ("same_point", "alternating"):
        k0 = rng.randrange(1, nn) if seed % 2 else rng.randrange(1, SMALL)
        kpool, mpool = [k0], [1, nn - 1]
        ki = np.zeros(n, dtype=np.int64)
        mi = np.zeros(n, dtype=np.int64) if design == "same_point" else (np.arange(n) & 1)
    elif design in ("walk_random", "walk_small", "cancel"):
        kpool = [k for j in range(1, SMALL) for k in (j, nn - j)] if design == "walk_small" else [rng.randrange(nn) for _ in range(4096)]
        mpool = walk
        ki = nprng.integers(0, len(kpool), n)
        mi = np.arange(n) % len(mpool)
    elif design == "window_shift":
        kpool, mpool, ki, mi = [], sorted({m % nn for m in fam.ints}), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        pairs = [craft_collision(fam, rng, wbits, "same" if j % 2 else "opp", with_lambda=False) for j in range(32)]
        for ks, ms, _ in pairs:
            kpool += ks
        idx = nprng.integers(0, len(pairs), (n + 1) // 2)
        for t in range(2):
            sel = idx[:len(ki[t::2])]
            ki[t::2] = 2 * sel + t
            mi[t::2] = np.array([mpool.index(ms[t]) for _, ms, _ in pairs])[sel]
    else:
        raise ValueError(design)
    nb = c.nbytes
    krows = np.frombuffer(scalar_bytes(c, kpool), dtype=np.uint8).reshape(len(kpool), nb)
    prows = np.frombuffer(point_bytes(fam, mpool), dtype=np.uint8).reshape(len(mpool), 2 * nb)
    scalars, points = krows[ki].copy(), prows[mi].copy()
    pair, cnt = np.unique(ki * len(mpool) + mi, return_counts=True)
    total = sum(int(q) * kpool[int(pr) // len(mpool)] * mpool[int(pr) % len(mpool)] for pr, q in zip(pair, cnt)) % nn
    if design == "cancel" and n >= 2:
        m_last = mpool[int(mi[-1])]
        total = (total - kpool[int(ki[-1])] * m_last) % nn
        k_last = -total * pow(m_last, -1, nn) % nn
        scalars[-1] = np.frombuffer(k_last.to_bytes(nb, "big"), dtype=np.uint8)
        total = 0
    return scalars, points, expected(c, [total], [1], fam.base)
