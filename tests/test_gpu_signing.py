"""Deterministic signing on the GPU (include/ecgpu.h, "deterministic signing"): ecgpu_rfc6979_nonce_batch against the RFC 6979 model
(tests/rfc6979_model.py, pinned by tests/test_hosttwin_signing.py), ecgpu_ecdsa_sign_prehash_batch against the reference's six signatures
and against ecgpu_ecdsa_sign_batch fed the model's nonces, ecgpu_schnorr_sign_prehash_batch against the BIP340 vectors and the oracle, and
the workspaces after each call.  Batch sizes: a single lane, below one wave, a ragged workgroup, and ragged tails of the 16-per-lane
finish batches and the 8-per-lane fixed-base batches.  Everything is byte-exact."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import rfc6979_model as R
from conftest import GOLDEN
from oracle import ecmodel as M

pytestmark = pytest.mark.gpu

CURVES = [("k256", 0), ("p256", 1), ("p384", 2)]
SIZES = [1, 63, 257, 4099]
NMAX = max(SIZES)
N = M.K256.n
ERR_ARG, ERR_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


def _rows(values, nb):
    return np.frombuffer(b"".join(v if isinstance(v, bytes) else v.to_bytes(nb, "big") for v in values), dtype=np.uint8).reshape(len(values), nb).copy()


_POOL = {}


def pool(cn):
    """NMAX random (key, prehash, additional data) per curve with the model's nonces for both forms: computed once, read-only"""
    if cn not in _POOL:
        c = M.CURVES[cn]
        rng = random.Random(0x516E + c.nbytes + len(_POOL))
        d = [rng.randrange(1, c.n) for _ in range(NMAX)]
        z = [rng.randbytes(c.nbytes) for _ in range(NMAX)]
        x = [rng.randbytes(c.nbytes) for _ in range(NMAX)]
        _POOL[cn] = (d, z, x, [R.nonce(c, d[i], z[i]) for i in range(NMAX)], [R.nonce(c, d[i], z[i], x[i]) for i in range(NMAX)])
    return _POOL[cn]


def batch(cn, n, with_extra):
    """the first n of the pool; from 63 elements on, the edges (x in {1, n-1} with z in {0, n-1, n, n+1, 2^(8 NB)-1}) and three invalid
    keys (0, n, n+1) planted in the middle -> (d, z, extra or None, expected k, indices of the invalid keys)"""
    c = M.CURVES[cn]
    nb = c.nbytes
    d, z, x, k0, k1 = pool(cn)
    d, z, x, k = list(d[:n]), list(z[:n]), list(x[:n]), list((k1 if with_extra else k0)[:n])
    bad = []
    if n >= 63:
        top = (1 << (8 * nb)) - 1
        plant = [(key, zz.to_bytes(nb, "big")) for key in (1, c.n - 1) for zz in (0, c.n - 1, c.n, c.n + 1, top)] + [(key, z[0]) for key in (0, c.n, c.n + 1)]
        at = n // 3
        for j, (key, zz) in enumerate(plant):
            d[at + j], z[at + j] = key, zz
            k[at + j] = R.nonce(c, key, zz, x[at + j] if with_extra else b"")
            if not 0 < key < c.n:
                bad.append(at + j)
    return _rows(d, nb), _rows(z, nb), (_rows(x, nb) if with_extra else None), _rows(k, nb), bad


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(a).cuda()


@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cn,cid", CURVES)
def test_rfc6979_nonce_batch(ctx, cn, cid, n, with_extra):
    import torch
    cv = ctx.curve(cn)
    d, z, x, want, bad = batch(cn, n, with_extra)
    got = cv.rfc6979_nonce(d, z, x)
    assert bytes(got) == bytes(want)
    assert all(not got[i].any() for i in bad) and (n < 63 or len(bad) == 3)
    t_k = torch.full((n, cv.nb), 0xA5, dtype=torch.uint8, device="cuda")
    t_d, t_z, t_x = _dev(d), _dev(z), _dev(x)
    torch.cuda.synchronize()
    cv.rfc6979_nonce_device(t_d, t_z, t_x, t_k, n)
    ctx.synchronize()
    assert bytes(t_k.cpu().numpy()) == bytes(want)


def test_sign_prehash_reference_vectors(ctx):
    """the six signatures of p256/src/ecdsa.rs and p384/src/ecdsa.rs (`rfc6979`, `prehash_signer_signing_with_*`)"""
    from ecgpu import ecdsa as E
    with open(os.path.join(GOLDEN, "rfc6979_sign.json")) as f:
        fixture = json.load(f)
    count = 0
    for cn, entry in fixture.items():
        cv = ctx.curve(cn)
        key = bytes.fromhex(entry["secret_key"])
        digests = [hashlib.new(v["hash"], bytes.fromhex(v["message"])).digest() for v in entry["vectors"]]
        sig, _, ok = E.sign_prehash(cv, [key] * len(digests), digests)
        assert ok.all()
        for i, v in enumerate(entry["vectors"]):
            assert bytes(sig[i]).hex() == v["signature"], (cn, v["test"])
            count += 1
    assert count == 6


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cn,cid", CURVES)
def test_sign_prehash_equals_sign_with_model_nonces(ctx, cn, cid, n):
    """signature, recovery id and ok of ecgpu_ecdsa_sign_prehash_batch = those of ecgpu_ecdsa_sign_batch fed the model's nonces (with and
    without additional data, host and device buffers); every signature verifies; an invalid key gives ok = 0 and zeros and leaves
    its neighbours alone"""
    import torch
    cv = ctx.curve(cn)
    nb = cv.nb
    for with_extra in (False, True):
        d, z, x, k, bad = batch(cn, n, with_extra)
        want_sig, want_rec, want_ok = cv.ecdsa_sign(d, k, z)
        sig, rec, ok = cv.ecdsa_sign_prehash(d, z, x)
        assert bytes(sig) == bytes(want_sig) and bytes(rec) == bytes(want_rec) and bytes(ok) == bytes(want_ok)
        good = np.ones(n, dtype=bool)
        good[bad] = False
        assert ok[good].all() and not ok[bad].any() and not sig[bad].any() and not rec[bad].any()
        pub, inf = cv.mul_by_generator(d)
        assert not inf[good].any()
        assert cv.ecdsa_verify(z[good], sig[good], pub[good]).all()
        t_sig = torch.full((n, 2 * nb), 0xA5, dtype=torch.uint8, device="cuda")
        t_rec = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        t_ok = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        t_d, t_z, t_x = _dev(d), _dev(z), _dev(x)
        torch.cuda.synchronize()
        cv.ecdsa_sign_prehash_device(t_d, t_z, t_x, t_sig, t_rec, t_ok, n)
        ctx.synchronize()
        assert bytes(t_sig.cpu().numpy()) == bytes(want_sig) and bytes(t_rec.cpu().numpy()) == bytes(want_rec) and bytes(t_ok.cpu().numpy()) == bytes(want_ok)


@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("cn", ["k256", "p384"])
def test_sign_prehash_first_call_and_growing_workspace(ctx, cn, with_extra):
    """ecgpu_ecdsa_sign_prehash_batch as the first call a context ever sees (its workspace does not exist yet), then on a larger
    batch (the workspace grows between the calls and loses its contents), then on the first batch again: the nonces derived into
    the workspace reach the signing kernels every time - signature, recovery id and ok equal those of ecgpu_ecdsa_sign_batch
    (on the module's context) fed the model's nonces"""
    import ecgpu
    c = M.CURVES[cn]
    nb = c.nbytes
    small = batch(cn, 300, with_extra)[:4]
    # 5000 rows: the pool's NMAX (with its planted edges), then rows of a generator of their own
    d, z, x, k, _ = batch(cn, NMAX, with_extra)
    rng = random.Random(0x6A0 + nb + with_extra)
    td = [rng.randrange(1, c.n) for _ in range(5000 - NMAX)]
    tz = [rng.randbytes(nb) for _ in td]
    tx = [rng.randbytes(nb) for _ in td]
    tk = [R.nonce(c, td[i], tz[i], tx[i] if with_extra else b"") for i in range(len(td))]
    large = (np.concatenate([d, _rows(td, nb)]), np.concatenate([z, _rows(tz, nb)]), np.concatenate([x, _rows(tx, nb)]) if with_extra else None,
             np.concatenate([k, _rows(tk, nb)]))
    want = [ctx.curve(cn).ecdsa_sign(bd, bk, bz) for bd, bz, _, bk in (small, large)]
    fresh = ecgpu.Context(0)
    try:
        cv = fresh.curve(cn)
        assert fresh.debug_workspace(1) == b""
        for (bd, bz, bx, _), w in ((small, want[0]), (large, want[1]), (small, want[0])):
            got = cv.ecdsa_sign_prehash(bd, bz, bx)
            for a, b in zip(got, w):
                assert bytes(a) == bytes(b), (cn, with_extra, len(bd))
            assert got[2].sum() == len(bd) - 3        # the three invalid keys batch() plants
    finally:
        fresh.close()


@pytest.mark.parametrize("cn,cid", CURVES)
def test_sign_prehash_flags(ctx, cn, cid):
    import ecgpu
    cv = ctx.curve(cn)
    n = 257
    d, z, _, k, _ = batch(cn, n, False)
    for flags in (0, ecgpu.ECDSA_LOW_S) if cn == "k256" else (0,):
        want = cv.ecdsa_sign(d, k, z, flags=flags)
        fast = cv.ecdsa_sign_prehash(d, z, flags=flags)
        exact = cv.ecdsa_sign_prehash(d, z, flags=flags | ecgpu.EXACT_REFERENCE)
        for a, b, c in zip(want, fast, exact):
            assert bytes(a) == bytes(b) == bytes(c), flags
    if cn == "k256":
        low = cv.ecdsa_sign_prehash(d, z, flags=ecgpu.ECDSA_LOW_S)[0]
        assert all(int.from_bytes(bytes(s[32:]), "big") <= N // 2 for s in low)
        assert bytes(low) != bytes(cv.ecdsa_sign_prehash(d, z, flags=0)[0])
    sig, rec, ok = np.zeros((n, 2 * cv.nb), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = ctx.lib.ecgpu_ecdsa_sign_prehash_batch(ctx.handle, cid, vp(d), vp(z), None, vp(sig), vp(rec), vp(ok), n, 0, ecgpu.PUBLIC_SCALARS)
    assert rc == ERR_ARG and "PUBLIC_SCALARS" in ctx.last_error()
    assert not sig.any() and not ok.any()


# --- BIP340 ---------------------------------------------------------------------------------------------------------

_SCHNORR = {}


def schnorr_pool():
    """NMAX random (key, digest, aux_rand) with the oracle's signatures, and computed once for the module (the
    Python oracle takes about 5 ms per signature: some 20 s here, shared by every BIP340 test below)"""
    if not _SCHNORR:
        rng = random.Random(0xB340)
        d = [rng.randrange(1, N).to_bytes(32, "big") for _ in range(NMAX)]
        m = [rng.randbytes(32) for _ in range(NMAX)]
        a = [rng.randbytes(32) for _ in range(NMAX)]
        out = [M.schnorr_sign_prehash(d[i], m[i], a[i]) for i in range(NMAX)]
        _SCHNORR.update(d=_rows(d, 32), m=_rows(m, 32), a=_rows(a, 32), sig=_rows([s for s, _ in out], 64), px=_rows([p for _, p in out], 32))
    return _SCHNORR


def test_schnorr_sign_reference_vectors(ctx, ref_vectors):
    cv = ctx.curve("k256")
    vs = ref_vectors["k256"]["bip340"]["sign"]
    assert len(vs) >= 4
    d = _rows([bytes.fromhex(v["secret_key"]) for v in vs], 32)
    m = _rows([bytes.fromhex(v["message"]) for v in vs], 32)
    a = _rows([bytes.fromhex(v["aux_rand"]) for v in vs], 32)
    sig, px, ok = cv.schnorr_sign_prehash(d, m, a)
    assert ok.all()
    for i, v in enumerate(vs):
        assert bytes(sig[i]).hex() == v["signature"].lower() and bytes(px[i]).hex() == v["public_key"].lower()
    from ecgpu import schnorr as S
    sigs, pxs = S.sign_batch_device(cv, [bytes(r) for r in d], [bytes(r) for r in m], [bytes(r) for r in a])
    assert b"".join(sigs) == bytes(sig) and b"".join(pxs) == bytes(px)


@pytest.mark.parametrize("n", SIZES)
def test_schnorr_sign_random_batches(ctx, n):
    import torch
    cv = ctx.curve("k256")
    p = schnorr_pool()
    d, m, a = p["d"][:n].copy(), p["m"][:n].copy(), p["a"][:n].copy()
    want_sig, want_px = p["sig"][:n].copy(), p["px"][:n].copy()
    bad = []
    if n >= 63:
        bad = [n // 3, n // 3 + 1, n // 3 + 2]
        for i, key in zip(bad, (0, N, N + 1)):
            d[i] = np.frombuffer(key.to_bytes(32, "big"), dtype=np.uint8)
            want_sig[i], want_px[i] = 0, 0
    good = np.ones(n, dtype=bool)
    good[bad] = False
    sig, px, ok = cv.schnorr_sign_prehash(d, m, a)
    assert bytes(sig) == bytes(want_sig) and bytes(px) == bytes(want_px)
    assert ok[good].all() and not ok[bad].any()
    assert cv.schnorr_verify_prehash(px[good], sig[good], m[good]).all()
    if n == NMAX:
        # both parities of y(P) and of y(R) occurred: P = d G and R = rand G on the throughput kernel, rand rebuilt from the tagged hashes
        P, _ = cv.mul_by_generator(d[good])
        p_odd = [int(r[63]) & 1 for r in P]
        k0 = []
        for i, (key, mm, aa) in enumerate(zip(d[good], m[good], a[good])):
            dp = N - int.from_bytes(bytes(key), "big") if p_odd[i] else int.from_bytes(bytes(key), "big")
            t = (dp ^ int.from_bytes(M._tagged_hash(b"BIP0340/aux", bytes(aa)), "big")).to_bytes(32, "big")
            k0.append(M._tagged_hash(b"BIP0340/nonce", t, bytes(P[i][:32]), bytes(mm)))
        Rp, _ = cv.mul_by_generator(_rows(k0, 32))
        assert np.array_equal(Rp[:, :32], sig[good][:, :32])
        r_odd = [int(r[63]) & 1 for r in Rp]
        assert min(p_odd.count(0), p_odd.count(1)) > n // 4 and min(r_odd.count(0), r_odd.count(1)) > n // 4
    t_sig = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
    t_px = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda")
    t_ok = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    t_d, t_m, t_a = _dev(d), _dev(m), _dev(a)
    torch.cuda.synchronize()
    cv.schnorr_sign_prehash_device(t_d, t_m, t_a, t_sig, t_px, t_ok, n)
    ctx.synchronize()
    assert bytes(t_sig.cpu().numpy()) == bytes(want_sig) and bytes(t_px.cpu().numpy()) == bytes(want_px) and bytes(t_ok.cpu().numpy()) == bytes(ok)
    # pubkeys_x is optional
    cv.schnorr_sign_prehash_device(t_d, t_m, t_a, t_sig, None, t_ok, n)
    ctx.synchronize()
    assert bytes(t_sig.cpu().numpy()) == bytes(want_sig)


def test_schnorr_sign_other_curves_unsupported(ctx):
    z = np.zeros((4, 32), np.uint8)
    sig, ok = np.zeros((4, 64), np.uint8), np.zeros(4, np.uint8)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = ctx.lib.ecgpu_schnorr_sign_prehash_batch(ctx.handle, 1, vp(z), vp(z), vp(z), vp(sig), None, vp(ok), 4, 0)
    assert rc == ERR_UNSUPPORTED and "secp256k1" in ctx.last_error()


# --- hygiene ----------------------------------------------------------------------------------------------------------

def _limbs(b):
    """big-endian bytes -> little-endian 32-bit limbs, least significant first (the kernels' internal form)"""
    return b"".join(b[i:i + 4][::-1] for i in range(len(b) - 4, -1, -4))


def _assert_absent(ctx, secrets, what):
    """no secret - as the wire bytes or as limbs - in the table workspace, the intermediate workspace or any staging slot"""
    blobs = {0: ctx.debug_workspace(0), 1: ctx.debug_workspace(1)}
    for slot in range(24):
        blobs[16 + slot] = ctx.debug_workspace(16 + slot)
    assert len(blobs[1]) > 0
    for which, blob in blobs.items():
        for i, sec in enumerate(secrets):
            assert sec not in blob and _limbs(sec) not in blob, (what, "workspace %d" % which, i)


@pytest.mark.parametrize("cn,cid", CURVES)
def test_no_nonce_or_key_stays_behind_ecdsa(ctx, cn, cid):
    cv = ctx.curve(cn)
    n = 257
    for with_extra in (False, True):
        d, z, x, k, bad = batch(cn, n, with_extra)
        # the planted prehash n-1 has the bytes of the planted key n-1, and a prehash is public: its staged copy stays.  Here those
        # rows take n-2, so that the key n-1 is searched for like every other key
        c = M.CURVES[cn]
        keys = {bytes(d[i]) for i in range(n) if i not in bad and 1 < int.from_bytes(bytes(d[i]), "big")}
        for i in range(n):
            if bytes(z[i]) in keys:
                zz = (c.n - 2).to_bytes(c.nbytes, "big")
                z[i] = np.frombuffer(zz, dtype=np.uint8)
                k[i] = np.frombuffer(R.nonce(c, int.from_bytes(bytes(d[i]), "big"), zz, bytes(x[i]) if with_extra else b"").to_bytes(c.nbytes, "big"), dtype=np.uint8)
        assert not keys & {bytes(r) for r in z}
        keep = [i for i in range(n) if i not in bad and 1 < int.from_bytes(bytes(d[i]), "big")]
        secrets = [bytes(k[i]) for i in keep] + [bytes(d[i]) for i in keep] + ([bytes(x[i]) for i in keep] if with_extra else [])
        got = cv.rfc6979_nonce(d, z, x)
        assert bytes(got) == bytes(k)
        _assert_absent(ctx, secrets, "ecgpu_rfc6979_nonce_batch")
        _, _, ok = cv.ecdsa_sign_prehash(d, z, x)
        assert ok[keep].all()
        _assert_absent(ctx, secrets, "ecgpu_ecdsa_sign_prehash_batch")
        _, _, ok = cv.ecdsa_sign_prehash(d, z, x, flags=cv.default_ecdsa_flags() | 1)
        assert ok[keep].all()
        _assert_absent(ctx, secrets, "ecgpu_ecdsa_sign_prehash_batch, reference schedule")


def test_no_nonce_or_key_stays_behind_schnorr(ctx):
    cv = ctx.curve("k256")
    c = M.K256
    n = 257
    p = schnorr_pool()
    d, m, a = p["d"][:n].copy(), p["m"][:n].copy(), p["a"][:n].copy()
    sig, px, ok = cv.schnorr_sign_prehash(d, m, a)
    assert ok.all() and bytes(sig) == bytes(p["sig"][:n])
    secrets = []
    for i in range(n):
        d0 = int.from_bytes(bytes(d[i]), "big")
        P = M.affine_mul(c, d0, (c.gx, c.gy))
        dp = N - d0 if P[1] & 1 else d0
        t = dp ^ int.from_bytes(M._tagged_hash(b"BIP0340/aux", bytes(a[i])), "big")
        k0 = int.from_bytes(M._tagged_hash(b"BIP0340/nonce", t.to_bytes(32, "big"), P[0].to_bytes(32, "big"), bytes(m[i])), "big")
        assert 0 < k0 < N
        secrets += [v.to_bytes(32, "big") for v in (d0, N - d0, t, k0, N - k0)] + [bytes(a[i])]
    _assert_absent(ctx, secrets, "ecgpu_schnorr_sign_prehash_batch")
