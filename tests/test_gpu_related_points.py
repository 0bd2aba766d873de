"""Multi-point entry points of the C ABI on RELATED points (tests/related_point_vectors.py: every point of a call is a known
multiple - +-j, +-lambda j, +-2^w, (n +- 1) / 2 - of one base point B), where the accumulators of the two-term kernels, of the
shared-doubling many-term schedule and of the bucket method meet the exceptional cases of the incomplete addition formulas:
infinity, the same point, opposite points.  Every result is compared with (sum k_i m_i mod n) B - Python integers and one scalar
multiplication of the big-integer model - not with another path of the library.  tests/test_related_point_coverage.py shows on
the host build that the lincomb inputs enter every branch; the bucket method has no host build, see test_msm below."""
import random

import numpy as np
import pytest

from oracle import ecmodel as M
import related_point_vectors as V

pytestmark = pytest.mark.gpu
CURVES = ["k256", "p256", "p384"]
# combinations per pattern, six patterns: 3072 / 2304 combinations per call at 2 / 3 and 5 terms (many waves, the dynamic chunks of
# sched.hpp, identity results next to finite ones under one shared inversion).  Cut for run time where a combination is long - the
# Python reference is one scalar multiplication per combination: 1536 at 16 and 17 terms, 576 (nine waves of work items) at 100
PER_PATTERN = {2: 512, 3: 384, 5: 384, 16: 256, 17: 256, 100: 96}


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


def _arr(raw, w):
    return np.frombuffer(raw, dtype=np.uint8).reshape(-1, w).copy()


def _batch(cn, terms, per_pattern, seed, patterns=V.PATTERNS):
    """all patterns over both bases in one call's worth of inputs: scalars, points, expected rows, expected flags"""
    c = M.CURVES[cn]
    sb, pb, want, winf = [], [], [], []
    for which in ("G", "S"):
        fam = V.family(cn, which)
        for pat in patterns:
            for ks, ms in V.combos(fam, pat, terms, per_pattern // 2, seed):
                sb.append(V.scalar_bytes(c, ks))
                pb.append(V.point_bytes(fam, ms))
                xy, inf = V.expected(c, ks, ms, fam.base)
                want.append(xy)
                winf.append(inf)
    return _arr(b"".join(sb), c.nbytes), _arr(b"".join(pb), 2 * c.nbytes), _arr(b"".join(want), 2 * c.nbytes), np.array(winf, dtype=np.uint8)


@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("terms", sorted(PER_PATTERN))
def test_lincomb(ctx, cn, terms):
    """terms = 2: the two-term throughput kernels; 3 .. 100: the many-term schedule (one group, two balanced groups, seven groups and
    the fold).  The default plan and the term-by-term plan must both give the expected element."""
    import ecgpu
    cv = ctx.curve(cn)
    s, p, want, winf = _batch(cn, terms, PER_PATTERN[terms], seed=7)
    try:
        for tbt in (0, 1):
            ctx.set_option(ecgpu.OPT_LINCOMB_TERM_BY_TERM, tbt)
            xy, inf = cv.lincomb(s, p, terms=terms)
            bad = np.nonzero((xy != want).any(axis=1) | (inf != winf))[0]
            assert len(bad) == 0, (cn, terms, "term by term" if tbt else "default plan", len(bad), bad[:8])
    finally:
        ctx.set_option(ecgpu.OPT_LINCOMB_TERM_BY_TERM, 0)
    assert 0 < winf.sum() < len(winf)                      # identity results sit next to finite ones


@pytest.mark.parametrize("cn", CURVES)
def test_mul_control(ctx, cn):
    """single term: the exceptional branches must not matter, the result still comes from the integer sum"""
    cv = ctx.curve(cn)
    s, p, want, winf = _batch(cn, 1, 512, seed=8, patterns=("small", "awkward"))
    xy, inf = cv.mul(s, p)
    assert (xy == want).all() and (inf == winf).all()


def _set_path(ctx, path, slab=0):
    """as in tests/test_gpu_msm.py: "auto" the library's own choice, "buckets16" / "buckets19" the bucket method with that window"""
    import ecgpu
    ctx.set_option(ecgpu.OPT_MSM_SMALL_PATH, 1 if path == "auto" else 0)
    ctx.set_option(ecgpu.OPT_MSM_WINDOW_BITS, 0 if path == "auto" else int(path[-2:]))
    ctx.set_option(ecgpu.OPT_MSM_SLAB_TERMS, slab)


@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("path", ["auto", "buckets16", "buckets19"])
@pytest.mark.parametrize("n,slab", [(5, 0), (300, 0), (20000, 0), (2**16 + 777, 30000), (2**19, 0)])
def test_msm(ctx, cn, path, n, slab):
    """The bucket method (and below 5 * 2^14 terms on "auto" the small path's tree sum) on the designs of
    related_point_vectors.msm_inputs.  There is no host build of these kernels, so branch hits cannot be counted: "same_point"
    (every bucket run adds B to B at its second entry, whatever the sort order) and "alternating" (B, -B: infinity and restart in
    every run) reach the XYZZ same-point and opposite-point branches by construction, but only with ZZ = 1 (the second entry of a
    run, or the one after a restart).  The hits with ZZ != 1 in the bucket runs, in the tree of running sums and in the Horner step
    rest on the other designs ("walk_*": partial sums walk over the multiples that are added; "window_shift": related buckets in
    neighbouring windows; "cancel").  Those branches themselves run on the device, with ZZ = 2, p - 1 and random and with lanes of
    one wave in different branches, in tests/test_gpu_group_edges.py (msm::xyzz_add_mixed, xyzz_add and jac::add one pair per lane;
    tests/test_hosttwin_group_edges.py counts the ":z" sites its vectors reach)."""
    cv = ctx.curve(cn)
    try:
        _set_path(ctx, path, slab)
        for which in ("G", "S"):
            fam = V.family(cn, which)
            for seed, design in enumerate(V.MSM_DESIGNS):
                if which == "S" and n > 20000 and design not in ("same_point", "window_shift"):
                    continue                               # the large sizes once per design; both bases for the two cheapest designs
                s, p, (xy, inf) = V.msm_inputs(fam, design, n, seed + (0 if which == "G" else 1), wbits=19 if path == "buckets19" else 16)
                got = bytes(cv.msm(s, p))
                assert got == xy, (cn, path, n, which, design, "identity expected" if inf else "")
    finally:
        _set_path(ctx, "auto")


def _ecdsa_rows(cn, per_pattern):
    """signatures that are valid by construction for chosen (u1, u2): Q = m G, R = (u1 + u2 m) G, r = R.x mod n, s = r / u2,
    z = u1 s.  -> rows (Q, z, r, s, recovery id) and the (u1, u2, m) behind each row.  u1 is the scalar the kernel recodes for
    the table of G, u2 the one for the table of Q:
      small    |u1|, |u2| < 2^10, Q any member of the family
      equal    u2 = +-u1 (u1 small or random): identical digit streams on both tables, so every window adds d G and then +-d (m G) -
               for m = +-1 the same point or the opposite one, for m = 2 .. 16 and lambda j another entry of the first table
      crafted  a searched window collision between u1 G and u2 (m G) with Z != 1"""
    c = M.CURVES[cn]
    n = c.n
    fam = V.family(cn, "G")
    rng = random.Random("ecdsa/" + cn)
    us = []
    for ks, _ in V.combos(fam, "small", 2, per_pattern, seed=9):
        us.append((ks[0], ks[1], rng.choice(fam.mult)))
    near = [1, n - 1] + [s * j % n for j in range(2, 17) for s in (1, -1)] + [s * j * L % n for L in fam.lams[:1] for j in range(1, 17) for s in (1, -1)]
    for i in range(per_pattern):
        k0 = rng.randrange(1, V.SMALL) if i % 2 else rng.randrange(1, n)
        m = near[i % len(near)] if i % 4 < 3 else rng.choice(fam.mult)
        u2 = k0 if (i // 2) % 2 == 0 else n - k0
        if (k0 + u2 * m) % n == 0:                         # u1 G + u2 Q would be the identity: no signature; take the other sign (whole-sum doubling)
            u2 = n - u2
        us.append((k0, u2, m))
    for i in range(per_pattern):                           # crafted: u1 on G itself, u2 on Q = m G meets u1 G's partial sum
        ks, ms, _ = V.craft_collision(fam, rng, 4, "same" if i % 2 else "opp", first=1)
        us.append((ks[0], ks[1], ms[1]))
    rows, kept = [], []
    for u1, u2, m in us:
        t = (u1 + u2 * m) % n
        if t == 0 or u2 == 0:
            continue
        R = M.affine_mul(c, t, fam.base)
        r = R[0] % n
        if r == 0:
            continue
        s = r * pow(u2, -1, n) % n
        rows.append((fam.point(m), u1 * s % n, r, s, (R[1] & 1) | ((1 if R[0] >= n else 0) << 1)))
        kept.append((u1, u2, m))
    return rows, kept


@pytest.mark.parametrize("cn", CURVES)
def test_ecdsa_constructed(ctx, cn):
    """u1 G + u2 Q with Q a small / lambda / 2^w multiple of G and (u1, u2) small, equal up to sign, or crafted to collide: verify
    accepts, the same row with z + 1 is rejected, recovery returns Q; the model agrees on every row."""
    c = M.CURVES[cn]
    cv = ctx.curve(cn)
    nb, n = c.nbytes, c.n
    rows, us = _ecdsa_rows(cn, 96)
    assert len(rows) > 250
    assert sum(u1 == u2 or u1 == n - u2 for u1, u2, _ in us) >= 90                   # pattern 3 reaches the kernel as such
    assert sum((u1 - u2 * m) % n == 0 for u1, u2, m in us) >= 4                      # u1 G == u2 Q: the whole sum is a doubling
    tob = lambda v: int(v).to_bytes(nb, "big")
    q = _arr(b"".join(tob(Q[0]) + tob(Q[1]) for Q, _, _, _, _ in rows), 2 * nb)
    z = _arr(b"".join(tob(zz) for _, zz, _, _, _ in rows), nb)
    z1 = _arr(b"".join(tob((zz + 1) % n) for _, zz, _, _, _ in rows), nb)
    sig = _arr(b"".join(tob(r) + tob(s) for _, _, r, s, _ in rows), 2 * nb)
    rid = np.array([v for _, _, _, _, v in rows], dtype=np.uint8)
    for i, (Q, zz, r, s, _) in enumerate(rows):
        assert M.ecdsa_verify_prehashed(c, Q, tob(zz), r, s) and not M.ecdsa_verify_prehashed(c, Q, tob((zz + 1) % n), r, s), i
    ok = cv.ecdsa_verify(z, sig, q, flags=0)
    assert ok.all(), np.nonzero(ok == 0)[0][:8]
    bad = cv.ecdsa_verify(z1, sig, q, flags=0)
    assert not bad.any(), np.nonzero(bad)[0][:8]
    rec, rok = cv.ecdsa_recover(z, sig, rid, flags=0)
    assert rok.all() and (rec == q).all(), np.nonzero((rec != q).any(axis=1))[0][:8]


def test_staging_slots_of_a_new_context_start_zero():
    """Regression: a staging slot is allocated with slack above the bytes a call stages, and the allocator hands back memory that
    earlier buffers of the process left as it was (this file's MSM workspaces, freed with their contents, made
    tests/test_gpu_scalar_ops.py::test_host_staging_is_cleared read stale bytes in that slack).  A slot now starts out zero.  The
    test first dirties memory on purpose: buffers of the very sizes the slots will have (and a large MSM's workspaces), filled with
    non-zero bytes and given back to the driver; then a new context's slots must hold nothing once a small secret-scalar call
    returns.  Best effort: it can only fail where the driver does hand such memory back."""
    import ecgpu
    import torch
    cnt = 4099
    fam = V.family("k256", "G")
    first = ecgpu.Context(0)
    s, p, (xy, _) = V.msm_inputs(fam, "walk_random", 2**19, 3)
    assert bytes(first.curve("k256").msm(s, p)) == xy
    first.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    sizes = [b + b // 4 + 256 for b in (cnt * 32, cnt)]                             # stage_reserve's capacity for the operand / result and the ok slots
    dirt = [torch.full((sz,), 0xA5, dtype=torch.uint8, device="cuda") for sz in sizes for _ in range(64)]
    torch.cuda.synchronize()
    del dirt
    torch.cuda.empty_cache()                                                        # back to the driver, contents and all
    second = ecgpu.Context(0)
    try:
        cv = second.curve("k256")
        a = _arr(V.scalar_bytes(M.K256, range(1, cnt + 1)), 32)
        cv.scalar_op(0, a, a)
        for slot in range(4):
            assert not any(second.debug_workspace(16 + slot)), slot
    finally:
        second.close()
