"""ECDSA where x(R) lies in [n, p), on the device: the rows of tests/ecdsa_wrap_vectors.py (tests/test_ecdsa_wrap_coverage.py shows on
the CPU that they are what they claim) through ecdsa_verify and ecdsa_recover at 1, 257 and 1031 rows, with default and explicit
flags, from device-resident buffers and through the message-level entry points; every ok byte and every key byte is the oracle's.
Then the two arms no public call reaches with a chosen R - x_reduced of sign_finish_kernel, and the tangent and operand arms of
verify_check_kernel with the second candidate r + n - on the device twin (tests/devtwin/devtwin_ecdsa.hip), one test per class."""
import functools
import hashlib

import numpy as np
import pytest

import ecdsa_wrap_vectors as V
import keccak_model
from oracle import ecmodel as M

pytestmark = pytest.mark.gpu
CURVES = ["k256", "p256", "p384"]


@pytest.fixture(scope="module")
def ctx():
    import ecgpu
    c = ecgpu.Context(0)
    yield c
    c.close()


def _col(rs, j, width):
    return np.frombuffer(b"".join(r.inputs[j] for r in rs), dtype=np.uint8).reshape(len(rs), width).copy()


def _xy(c, P):
    return M.i2b(c, P[0]) + M.i2b(c, P[1])


def _verify_mismatch(got, rs, want=None):
    want = [r.want for r in rs] if want is None else want
    assert set(np.asarray(got).tolist()) <= {0, 1}
    return [(i, r.cls, int(g), bool(w)) for i, (g, r, w) in enumerate(zip(got, rs, want)) if bool(g) != bool(w)][:10]


def _recover_mismatch(c, out, ok, rs, want=None):
    want = [r.want for r in rs] if want is None else want
    bad = []
    for i, (r, w) in enumerate(zip(rs, want)):
        good = (ok[i] == 0 and not out[i].any()) if w is None else (ok[i] == 1 and bytes(out[i]) == _xy(c, w))
        if not good:
            bad.append((i, r.cls, int(ok[i]), w is not None))
    return bad[:10]


@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("n", V.SIZES)
def test_ecdsa_verify(ctx, cn, n):
    nb = M.CURVES[cn].nbytes
    rs = V.rows(cn, "verify")[:n]
    got = ctx.curve(cn).ecdsa_verify(_col(rs, 0, nb), _col(rs, 1, 2 * nb), _col(rs, 2, 2 * nb))
    assert not _verify_mismatch(got, rs)
    if n == V.N:
        assert int(got.sum()) == sum(V.VERIFY_COUNTS[cls] for cls in V.VERIFY_VALID)


@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("n", V.SIZES)
def test_ecdsa_recover_and_round_trip(ctx, cn, n):
    c = M.CURVES[cn]
    nb = c.nbytes
    cv = ctx.curve(cn)
    rs = V.rows(cn, "recover")[:n]
    z, sg = _col(rs, 0, nb), _col(rs, 1, 2 * nb)
    out, ok = cv.ecdsa_recover(z, sg, [r.inputs[2] for r in rs])
    assert not _recover_mismatch(c, out, ok, rs)
    if n == V.N:
        assert int(ok.sum()) == sum(1 for r in rs if r.want is not None) >= V.RECOVER_COUNTS["wrap"] + V.RECOVER_COUNTS["wrong_parity"]
    # the keys recovered from the wrap rows verify their signatures on the device
    keep = [i for i, r in enumerate(rs) if r.cls == "wrap"]
    assert keep and ok[keep].all()
    assert cv.ecdsa_verify(z[keep], sg[keep], out[keep]).tolist() == [1] * len(keep)


@pytest.mark.parametrize("cn", CURVES)
def test_explicit_flags(ctx, cn):
    """ECDSA_LOW_S given and withheld, on half of every class's pool: without it a high s on secp256k1 recovers the other key; with
    it the NIST curves reject the rows whose s is high"""
    import ecgpu
    c = M.CURVES[cn]
    nb = c.nbytes
    cv = ctx.curve(cn)
    vs = [r for rows in V.verify_pool(cn).values() for r in rows[:4]]
    rs = [r for rows in V.recover_pool(cn).values() for r in rows[:4]]
    num = lambda r: (M.b2i(r.inputs[1][:nb]), M.b2i(r.inputs[1][nb:]))
    for flags in (0, ecgpu.ECDSA_LOW_S):
        want = [M.ecdsa_verify_prehashed(c, (M.b2i(r.inputs[2][:nb]), M.b2i(r.inputs[2][nb:])), r.inputs[0], *num(r), reject_high_s=bool(flags)) for r in vs]
        got = cv.ecdsa_verify(_col(vs, 0, nb), _col(vs, 1, 2 * nb), _col(vs, 2, 2 * nb), flags=flags)
        assert not _verify_mismatch(got, vs, want)
        assert any(want[i] for i, r in enumerate(vs) if r.cls == "wrap")
        want = [M.ecdsa_recover_prehashed(c, r.inputs[0], *num(r), r.inputs[2], reject_high_s=bool(flags)) for r in rs]
        out, ok = cv.ecdsa_recover(_col(rs, 0, nb), _col(rs, 1, 2 * nb), [r.inputs[2] for r in rs], flags=flags)
        assert not _recover_mismatch(c, out, ok, rs, want)
        assert all((want[i] is None) == bool(flags) for i, r in enumerate(rs) if r.cls == "high_s")


@pytest.mark.parametrize("cn", CURVES)
def test_device_resident_buffers(ctx, cn):
    import torch
    c = M.CURVES[cn]
    nb = c.nbytes
    cv = ctx.curve(cn)
    n = 257
    dev = lambda a: torch.from_numpy(a).cuda()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        vs, rs = V.rows(cn, "verify")[:n], V.rows(cn, "recover")[:n]
        d_ok = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        cv.ecdsa_verify_device(dev(_col(vs, 0, nb)), dev(_col(vs, 1, 2 * nb)), dev(_col(vs, 2, 2 * nb)), d_ok, n)
        d_key = torch.full((n, 2 * nb), 0xEE, dtype=torch.uint8, device="cuda")
        d_rok = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        cv.ecdsa_recover_device(dev(_col(rs, 0, nb)), dev(_col(rs, 1, 2 * nb)), dev(np.array([r.inputs[2] for r in rs], dtype=np.uint8)), d_key, d_rok, n)
        ctx.synchronize()
        assert not _verify_mismatch(d_ok.cpu().numpy(), vs)
        assert not _recover_mismatch(c, d_key.cpu().numpy(), d_rok.cpu().numpy(), rs)
    finally:
        ctx.set_stream(0)


def _digests(cn):
    own = ("sha384", lambda m: hashlib.sha384(m).digest()) if cn == "p384" else ("sha256", lambda m: hashlib.sha256(m).digest())
    return [own] + ([("keccak256", keccak_model.keccak256)] if cn == "k256" else [])


@pytest.mark.parametrize("cn", CURVES)
def test_byte_entry_points(ctx, cn):
    """64 wrap / wrap_bad / no_p_check rows whose z is the digest of a random message, the key constructed from that z: the curve's
    own digest through ecdsa_verify_msg and ecdsa_recover_msg, Keccak-256 on secp256k1 through verify_digest and recover_digest"""
    import ecgpu
    from ecgpu import ecdsa
    c = M.CURVES[cn]
    cv = ctx.curve(cn)
    for name, digest in _digests(cn):
        ms = V.msg_rows(cn, name, digest)
        assert len(ms) == 64 and [m.valid for m in ms] == [m.cls == "wrap" for m in ms]
        assert all(m.key is not None for m in ms if m.cls == "wrap") and not any(m.key for m in ms if m.cls == "no_p_check")
        msgs, sigs, keys, rids = [m.msg for m in ms], [m.sig for m in ms], [m.Q for m in ms], [m.recid for m in ms]
        if name == "keccak256":
            got = ecdsa.verify_digest(cv, ecgpu.KECCAK256, keys, msgs, sigs)
            out, ok = ecdsa.recover_digest(cv, ecgpu.KECCAK256, msgs, sigs, rids)
        else:
            got = cv.ecdsa_verify_msg(msgs, b"".join(sigs), b"".join(keys))
            out, ok = cv.ecdsa_recover_msg(msgs, b"".join(sigs), rids)
        assert got.tolist() == [int(m.valid) for m in ms], name
        for i, m in enumerate(ms):
            if m.key is None:
                assert ok[i] == 0 and not out[i].any(), (name, i, m.cls)
            else:
                assert ok[i] == 1 and bytes(out[i]) == _xy(c, m.key), (name, i, m.cls)
            assert m.cls != "wrap" or bytes(out[i]) == m.Q
        if cn == "k256":
            keep = [i for i, m in enumerate(ms) if m.key is not None]
            addr = ecdsa.eth_addresses(ctx, out[keep])
            assert [bytes(a) for a in addr] == [keccak_model.eth_address(_xy(c, ms[i].key)) for i in keep]


# ---------------------------------------------------------------------------------------------------------------------------------
# the device twin: sign_finish_kernel and verify_check_kernel on chosen R, A and B
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sign_run(cn, n, flags):
    import devtwin_util as D
    c = M.CURVES[cn]
    rs = V.sign_rows(cn)[:n]
    return D.ecdsa_sign_finish(cn, [M.i2b(c, r.d) for r in rs], [M.i2b(c, r.k) for r in rs], [r.z for r in rs], [_xy(c, r.R) for r in rs],
                               [r.r_inf for r in rs], flags)


@pytest.mark.parametrize("cls", sorted(set(V.SIGN_CLASSES)) + ["control"])
@pytest.mark.parametrize("cn", CURVES)
def test_devtwin_sign_finish(cn, cls):
    """r || s, the recovery id and ok of every row of the class, at the three sizes, with ECDSA_LOW_S off and on"""
    c = M.CURVES[cn]
    nb = c.nbytes
    if cls == "x_eq_n" and not V.anchors(cn).n_on_curve:
        assert cls not in V.sign_classes(cn) and not V.sign_pool(cn)[cls]       # P-256: n is no x of the curve, nothing to run
        return
    seen = 0
    for n in V.SIZES:
        for flags in (0, V.LOW_S):
            sig, recid, ok = _sign_run(cn, n, flags)
            for i, r in enumerate(V.sign_rows(cn)[:n]):
                if r.cls != cls:
                    continue
                seen += 1
                want = r.want[flags]
                if want is None:
                    assert ok[i] == 0 and recid[i] == 0 and not sig[i].any(), (n, flags, i)
                else:
                    assert ok[i] == 1 and (M.b2i(bytes(sig[i, :nb])), M.b2i(bytes(sig[i, nb:])), int(recid[i])) == want, (n, flags, i)
    assert seen >= 2 * V.SIGN_COUNTS[cls]


@functools.lru_cache(maxsize=None)
def _check_run(cn, n):
    import devtwin_util as D
    c = M.CURVES[cn]
    rs = V.check_rows(cn, n)
    xy = lambda P: bytes(2 * c.nbytes) if P is None else _xy(c, P)
    return D.ecdsa_verify_check(cn, [xy(r.A) for r in rs], [int(r.A is None) for r in rs], [xy(r.B) for r in rs], [int(r.B is None) for r in rs],
                                [M.i2b(c, r.r) + M.i2b(c, 1) for r in rs], [r.ok_in for r in rs])


@pytest.mark.parametrize("cls", V.CHECK_CLASSES)
@pytest.mark.parametrize("cn", CURVES)
def test_devtwin_verify_check(cn, cls):
    """ok of every row of the class - each as a tangent, a chord, with either operand at infinity and as A = -B - at the three sizes"""
    seen = set()
    for n in V.SIZES:
        got = _check_run(cn, n)
        assert set(got.tolist()) <= {0, 1}
        for i, r in enumerate(V.check_rows(cn, n)):
            if r.cls == cls:
                seen.add(r.kind)
                assert bool(got[i]) == r.want, (n, i, r.kind, hex(r.r))
    assert seen == set(V.CHECK_KINDS)
