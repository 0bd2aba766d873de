"""ECDSA batch verify / sign on the GPU against the reference's vectors (ECDSA KATs, Wycheproof) and the
oracle on random and edge-case batches."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

from oracle import ecmodel as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = ["k256", "p256", "p384"]


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


def padded(c, hx):
    b = bytes.fromhex(hx)
    if len(b) >= c.nbytes:
        return b[len(b) - c.nbytes:]
    return bytes(c.nbytes - len(b)) + b


@pytest.mark.parametrize("cn", CURVES)
def test_wycheproof(ctx, cn):
    from ecgpu import ecdsa
    c = M.CURVES[cn]
    cv = ctx.curve(cn)
    with open(os.path.join(HERE, "golden", f"wycheproof_{cn}.json")) as f:
        rows = json.load(f)["rows"]
    keys = [padded(c, wx) + padded(c, wy) for wx, wy, _, _, _ in rows]
    msgs = [bytes.fromhex(r[2]) for r in rows]
    sigs = [bytes.fromhex(r[3]) for r in rows]
    want = np.array([r[4] for r in rows], dtype=np.uint8)
    got = ecdsa.verify_der_batch(cv, keys, msgs, sigs, normalize_s=(cn == "k256"))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"rows {bad[:10]} differ"
    assert want.sum() > 100


@pytest.mark.parametrize("cn", CURVES)
def test_sign_kats_and_roundtrip(ctx, cn, ref_vectors):
    c = M.CURVES[cn]
    cv = ctx.curve(cn)
    vs = ref_vectors[cn]["ecdsa"]
    d = b"".join(bytes.fromhex(v["d"]) for v in vs)
    k = b"".join(bytes.fromhex(v["k"]) for v in vs)
    z = b"".join(M.bits2field(c, bytes.fromhex(v["m"])) for v in vs)
    sig, rec, ok = cv.ecdsa_sign(d, k, z, flags=0)
    assert ok.all()
    for i, v in enumerate(vs):
        assert bytes(sig[i]).hex() == v["r"] + v["s"]
        want = M.ecdsa_sign_prehashed(c, int(v["d"], 16), int(v["k"], 16), z[c.nbytes * i:c.nbytes * (i + 1)])
        assert rec[i] == want[2]
    q = b"".join(bytes.fromhex(v["q_x"]) + bytes.fromhex(v["q_y"]) for v in vs)
    assert cv.ecdsa_verify(z, sig, q, flags=0).all()
    import ecgpu
    sig_ref, rec_ref, ok_ref = cv.ecdsa_sign(d, k, z, flags=ecgpu.EXACT_REFERENCE)      # reference schedule for k G: same values
    assert bytes(sig_ref) == bytes(sig) and bytes(rec_ref) == bytes(rec) and ok_ref.all()
    # k256 low-s behaviour (k256/src/ecdsa.rs:182-207)
    if cn == "k256":
        sig2, rec2, ok2 = cv.ecdsa_sign(d, k, z)
        for i, v in enumerate(vs):
            want = M.ecdsa_sign_prehashed(c, int(v["d"], 16), int(v["k"], 16), z[32 * i:32 * i + 32], normalize_s=True)
            assert (int.from_bytes(bytes(sig2[i][:32]), "big"), int.from_bytes(bytes(sig2[i][32:]), "big"), rec2[i]) == want
        assert cv.ecdsa_verify(z, sig2, q).all()


@pytest.mark.parametrize("cn", CURVES)
def test_random_and_edge_cases_vs_oracle(ctx, cn):
    c = M.CURVES[cn]
    cv = ctx.curve(cn)
    nb = c.nbytes
    rng = random.Random(1234 + nb)
    n = 600
    ds = [rng.randrange(1, c.n) for _ in range(n)]
    ks = [rng.randrange(1, c.n) for _ in range(n)]
    zs = [rng.randbytes(nb) for _ in range(n)]
    # edge cases for signing: out-of-range d / k, extreme prehashes
    ds[0] = 0; ks[1] = 0; ds[2] = c.n; ks[3] = c.n; zs[4] = bytes(nb); zs[5] = b"\xff" * nb; ks[6] = 1; ks[7] = c.n - 1; ds[8] = c.n - 1
    tob = lambda v: (v % (1 << (8 * nb))).to_bytes(nb, "big")
    sig, rec, ok = cv.ecdsa_sign(b"".join(map(tob, ds)), b"".join(map(tob, ks)), b"".join(zs))
    low_s = (cn == "k256")
    qs = []
    for i in range(n):
        want = M.ecdsa_sign_prehashed(c, ds[i], ks[i], zs[i], normalize_s=low_s) if 0 < ds[i] < c.n else None
        if want is None:
            assert ok[i] == 0 and not bytes(sig[i]).strip(b"\0")
        else:
            assert ok[i] == 1
            assert (int.from_bytes(bytes(sig[i][:nb]), "big"), int.from_bytes(bytes(sig[i][nb:]), "big"), rec[i]) == want, i
        Q = M.affine_mul(c, ds[i] % c.n or 1, (c.gx, c.gy))
        qs.append(tob(Q[0]) + tob(Q[1]))
    # verification: valid signatures, then systematic corruptions, all against the oracle
    sigs = [bytes(sig[i]) for i in range(n)]
    zz = list(zs)
    for i in range(20, n):
        m = i % 12
        r = int.from_bytes(sigs[i][:nb], "big"); s = int.from_bytes(sigs[i][nb:], "big")
        if m == 0: s = c.n - s                       # high s (valid on NIST, rejected on k256)
        elif m == 1: r = 0
        elif m == 2: s = 0
        elif m == 3: r = c.n
        elif m == 4: s = c.n
        elif m == 5: zz[i] = rng.randbytes(nb)
        elif m == 6: qs[i] = qs[i - 1]
        elif m == 7: qs[i] = bytes(2 * nb)           # identity key
        elif m == 8: qs[i] = qs[i][:nb] + tob(int.from_bytes(qs[i][nb:], "big") ^ 1)   # off the curve
        elif m == 9: r = (r + 1) % c.n
        sigs[i] = tob(r) + tob(s)
    got = cv.ecdsa_verify(b"".join(zz), b"".join(sigs), b"".join(qs))
    n_ok = 0
    for i in range(n):
        Q = (int.from_bytes(qs[i][:nb], "big"), int.from_bytes(qs[i][nb:], "big"))
        key_ok = Q != (0, 0) and Q[0] < c.p and Q[1] < c.p and M.on_curve(c, Q)
        r = int.from_bytes(sigs[i][:nb], "big"); s = int.from_bytes(sigs[i][nb:], "big")
        want = key_ok and M.ecdsa_verify_prehashed(c, Q, zz[i], r, s, reject_high_s=low_s)
        assert bool(got[i]) == bool(want), (i, i % 12)
        n_ok += bool(want)
    assert 50 < n_ok < n


def test_x_coordinate_wraparound(ctx):
    """r + n < p: a signature whose x(R) lies in [n, p) must still verify (x mod n == r).  No search finds such an R = k G (2^-128
    on this curve), but one is constructed: lift the smallest on-curve x above n to R, choose s and z, set r = x - n and
    Q = r^-1 (s R - z G).  It verifies by the check kernel's second candidate, its twin with r + 1 does not, and an ordinary signature
    stays valid.  tests/test_gpu_ecdsa_wrap.py has the classes around this branch on all three curves."""
    import ecdsa_wrap_vectors as W
    c = M.K256
    cv = ctx.curve("k256")
    d, k, z = 12345, 67890, hashlib.sha256(b"wrap").digest()
    r, s, _ = M.ecdsa_sign_prehashed(c, d, k, z, normalize_s=True)
    Q = M.affine_mul(c, d, (c.gx, c.gy))
    tob = lambda v: v.to_bytes(32, "big")
    assert cv.ecdsa_verify(z, tob(r) + tob(s), tob(Q[0]) + tob(Q[1]))[0] == 1
    R = M.decompress(c, W.anchors("k256").lo, 0)
    r = R[0] - c.n
    assert c.n < R[0] < c.p and 0 < r
    Q = W.key_for(c, R, r, s, z)
    assert M.ecdsa_verify_prehashed(c, Q, z, r, s, reject_high_s=True) and not M.ecdsa_verify_prehashed(c, Q, z, r + 1, s, reject_high_s=True)
    got = cv.ecdsa_verify(z + z, tob(r) + tob(s) + tob(r + 1) + tob(s), 2 * (tob(Q[0]) + tob(Q[1])))
    assert got.tolist() == [1, 0]


def test_large_batch_all_valid_and_sparse_invalid(ctx):
    """2^18 signatures made on the device, verified on the device; every 1000th is corrupted."""
    import torch
    from oracle import synth
    cv = ctx.curve("k256")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = 1 << 18
    d_d = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    d_k = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    d_z = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    cv.synth_scalars_device(d_d, n, synth.SEED, 100)
    cv.synth_scalars_device(d_k, n, synth.SEED, 100 + n)
    cv.synth_scalars_device(d_z, n, synth.SEED, 100 + 2 * n)
    d_sig = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    d_rec = torch.empty((n,), dtype=torch.uint8, device="cuda")
    d_ok = torch.empty((n,), dtype=torch.uint8, device="cuda")
    cv.ecdsa_sign_device(d_d, d_k, d_z, d_sig, d_rec, d_ok, n)
    d_q = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    cv.mul_device(d_d, None, d_q, n)
    d_sig[::1000, 40] ^= 1
    d_v = torch.empty((n,), dtype=torch.uint8, device="cuda")
    cv.ecdsa_verify_device(d_z, d_sig, d_q, d_v, n)
    ctx.synchronize()
    assert bool(d_ok.all())
    v = d_v.cpu().numpy()
    want = np.ones(n, dtype=np.uint8)
    want[::1000] = 0
    assert (v == want).all()
    ctx.set_stream(0)


@pytest.mark.parametrize("cn,n", [("k256", (1 << 22) + 4321), ("p256", 1 << 22), ("k256", 1 << 23), ("p384", (3 << 20) + 77)])
def test_signing_constant_time_grid_sizes(ctx, cn, n):
    """The constant-time fixed-base kernel launches up to four times the resident workgroups once every lane keeps a full
    inversion batch (ecgpu_grid_oversubscribed: from 2^22 signatures per call on): at those sizes, ragged included, the signatures
    must be byte-identical to the ones the throughput schedule (PUBLIC_SCALARS: table gathers, another kernel and grid) produces,
    and the first and last few to the oracle's."""
    import torch
    import ecgpu
    from oracle import synth
    cv = ctx.curve(cn)
    nb = cv.nb
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d_d = torch.empty((n, nb), dtype=torch.uint8, device="cuda")
    d_k = torch.empty((n, nb), dtype=torch.uint8, device="cuda")
    d_z = torch.empty((n, nb), dtype=torch.uint8, device="cuda")
    cv.synth_scalars_device(d_d, n, synth.SEED, 7)
    cv.synth_scalars_device(d_k, n, synth.SEED, 7 + n)
    cv.synth_scalars_device(d_z, n, synth.SEED, 7 + 2 * n)
    outs = []
    for fl in (ecgpu.SECRET_SCALARS, ecgpu.PUBLIC_SCALARS):
        d_sig = torch.zeros((n, 2 * nb), dtype=torch.uint8, device="cuda")
        d_rec = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        d_ok = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        cv.ecdsa_sign_device(d_d, d_k, d_z, d_sig, d_rec, d_ok, n, flags=fl | cv.default_ecdsa_flags())
        ctx.synchronize()
        outs.append((d_sig, d_rec, d_ok))
    assert bool(outs[0][2].all())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    c = M.CURVES[cn]
    sig = outs[0][0]
    rec = outs[0][1]
    for i in [0, 1, n // 2, n - 2, n - 1]:
        d, k = (int.from_bytes(bytes(t[i].cpu().numpy()), "big") for t in (d_d, d_k))
        want = M.ecdsa_sign_prehashed(c, d, k, bytes(d_z[i].cpu().numpy()), normalize_s=(cn == "k256"))
        got = bytes(sig[i].cpu().numpy())
        assert (int.from_bytes(got[:nb], "big"), int.from_bytes(got[nb:], "big"), int(rec[i])) == want, (cn, i)
    ctx.set_stream(0)


def test_bip340_schnorr_vectors_and_random(ctx, ref_vectors):
    """BIP340 sign vectors 0-3 and verify vectors 4-14 of k256/src/schnorr.rs, then random signatures made through the
    device (mul_by_generator) and systematic corruptions, all against the model."""
    from ecgpu import schnorr
    cv = ctx.curve("k256")
    v = ref_vectors["k256"]["bip340"]
    sigs, pxs = schnorr.sign_batch(cv, [bytes.fromhex(s["secret_key"]) for s in v["sign"]], [bytes.fromhex(s["message"]) for s in v["sign"]],
                                   [bytes.fromhex(s["aux_rand"]) for s in v["sign"]])
    assert [s.hex() for s in sigs] == [s["signature"] for s in v["sign"]]
    assert [p.hex() for p in pxs] == [s["public_key"] for s in v["sign"]]
    keys = [bytes.fromhex(t["public_key"]) for t in v["verify"]] + pxs
    msgs = [bytes.fromhex(t["message"]) for t in v["verify"]] + [bytes.fromhex(s["message"]) for s in v["sign"]]
    sg = [bytes.fromhex(t["signature"]) for t in v["verify"]] + sigs
    want = [t["valid"] for t in v["verify"]] + [True] * 4
    assert list(map(bool, schnorr.verify_batch(cv, keys, msgs, sg))) == want
    rng = random.Random(340)
    n = 300
    sk = [rng.randrange(1, M.K256.n).to_bytes(32, "big") for _ in range(n)]
    ms = [rng.randbytes(32) for _ in range(n)]
    aux = [rng.randbytes(32) for _ in range(n)]
    sigs, pxs = schnorr.sign_batch(cv, sk, ms, aux)
    for i in range(0, n, 37):
        assert (sigs[i], pxs[i]) == M.schnorr_sign_prehash(sk[i], ms[i], aux[i])
    for i in range(10, n):
        m = i % 9
        b = bytearray(sigs[i])
        if m == 0: b[5] ^= 1                                     # r changed
        elif m == 1: b[40] ^= 1                                  # s changed
        elif m == 2: ms[i] = rng.randbytes(32)
        elif m == 3: pxs[i] = pxs[i - 1]
        elif m == 4: b[32:] = M.K256.n.to_bytes(32, "big")       # s = n
        elif m == 5: b[:32] = M.K256.p.to_bytes(32, "big")       # r = p
        elif m == 6: b[32:] = bytes(32)                          # s = 0
        sigs[i] = bytes(b)
    got = schnorr.verify_batch(cv, pxs, ms, sigs)
    good = 0
    for i in range(n):
        w = M.schnorr_verify_prehash(pxs[i], ms[i], sigs[i])
        assert bool(got[i]) == w, (i, i % 9)
        good += w
    assert 50 < good < n


@pytest.mark.parametrize("cn", CURVES)
def test_public_key_recovery(ctx, cn, ref_vectors):
    """recover_from_prehash: the reference's two secp256k1 vectors, then sign -> recover == d G on random batches of
    every curve, wrong recovery ids, corrupted signatures and out-of-range values against the model."""
    c = M.CURVES[cn]
    cv = ctx.curve(cn)
    nb = c.nbytes
    tob = lambda v: v.to_bytes(nb, "big")
    if cn == "k256":
        vs = ref_vectors["k256"]["recovery"]
        z = b"".join(hashlib.sha256(v["msg"].encode()).digest() for v in vs)
        out, ok = cv.ecdsa_recover(z, b"".join(bytes.fromhex(v["sig"]) for v in vs), [v["recid"] for v in vs])
        assert ok.all()
        assert [bytes(g).hex() for g in cv.to_bytes(out)] == [v["pk"] for v in vs]
    rng = random.Random(4321 + nb)
    n = 400
    ds = [rng.randrange(1, c.n) for _ in range(n)]
    ks = [rng.randrange(1, c.n) for _ in range(n)]
    zs = [rng.randbytes(nb) for _ in range(n)]
    sig, rec, okv = cv.ecdsa_sign(b"".join(map(tob, ds)), b"".join(map(tob, ks)), b"".join(zs))
    assert okv.all()
    keys, _ = cv.mul_by_generator(b"".join(map(tob, ds)))
    out, ok = cv.ecdsa_recover(b"".join(zs), sig, rec)
    assert ok.all() and bytes(out) == bytes(keys)
    sigs = [bytes(sig[i]) for i in range(n)]
    rid = [int(x) for x in rec]
    for i in range(n):
        m = i % 8
        r = int.from_bytes(sigs[i][:nb], "big"); s = int.from_bytes(sigs[i][nb:], "big")
        if m == 0: rid[i] ^= 1
        elif m == 1: rid[i] |= 2                    # r + n >= p for these random r (p - n < 2^191); tests/test_gpu_ecdsa_wrap.py has constructed r with r + n < p
        elif m == 2: s = c.n - s                    # high s: refused on k256, a different key elsewhere
        elif m == 3: r = 0
        elif m == 4: s = c.n
        elif m == 5: zs[i] = rng.randbytes(nb)
        elif m == 6: rid[i] = 4
        sigs[i] = tob(r) + tob(s)
    out, ok = cv.ecdsa_recover(b"".join(zs), b"".join(sigs), rid)
    hits = 0
    for i in range(n):
        r = int.from_bytes(sigs[i][:nb], "big"); s = int.from_bytes(sigs[i][nb:], "big")
        Q = M.ecdsa_recover_prehashed(c, zs[i], r, s, rid[i], reject_high_s=(cn == "k256"))
        if Q is None:
            assert ok[i] == 0 and not bytes(out[i]).strip(b"\0"), (i, i % 8)
        else:
            assert ok[i] == 1 and bytes(out[i]) == tob(Q[0]) + tob(Q[1]), (i, i % 8)
            hits += 1
    assert 100 < hits < n
