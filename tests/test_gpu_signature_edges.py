"""The rows of tests/signature_edge_vectors.py through the public calls: signatures whose final affine sum is a tangent, the
identity, or has an operand at infinity, mixed into the lanes of the batched kernels with ordinary and rejected ones, at 1, 257 and
1031 elements.  Every ok byte and every recovered key is the oracle's.  tests/test_hosttwin_sigsum.py shows on the CPU, by the
ECGPU_EXC_NOTE counters, that each class enters the arm it names.  Then decompress, validate_points and sec1_decode on the lift and
curve-check rows."""
import numpy as np
import pytest

import signature_edge_vectors as V
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


def _mismatch(got, rs):
    return [(i, r.cls, int(g), bool(r.want)) for i, (g, r) in enumerate(zip(got, rs)) if bool(g) != bool(r.want)][:10]


@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("n", V.SIZES)
def test_ecdsa_verify(ctx, cn, n):
    c = M.CURVES[cn]
    nb = c.nbytes
    rs = V.rows(cn, "ecdsa")[:n]
    got = ctx.curve(cn).ecdsa_verify(_col(rs, 0, nb), _col(rs, 1, 2 * nb), _col(rs, 2, 2 * nb))
    assert set(got.tolist()) <= {0, 1} and not _mismatch(got, rs)
    if n == V.N:
        assert sum(r.want for r in rs) == 2 * 14 + V.COUNTS["chord"]


@pytest.mark.parametrize("cn", CURVES)
@pytest.mark.parametrize("n", V.SIZES)
def test_ecdsa_recover(ctx, cn, n):
    c = M.CURVES[cn]
    nb = c.nbytes
    rs = V.rows(cn, "recover")[:n]
    out, ok = ctx.curve(cn).ecdsa_recover(_col(rs, 0, nb), _col(rs, 1, 2 * nb), [r.inputs[2] for r in rs])
    for i, r in enumerate(rs):
        if r.want is None:
            assert ok[i] == 0 and not out[i].any(), (i, r.cls)
        else:
            assert ok[i] == 1 and bytes(out[i]) == M.i2b(c, r.want[0]) + M.i2b(c, r.want[1]), (i, r.cls)


@pytest.mark.parametrize("n", V.SIZES)
def test_schnorr_verify_and_batch_verify(ctx, n):
    import ecgpu
    cv = ctx.curve("k256")
    rs = V.rows("k256", "schnorr")[:n]
    px, sig, e = _col(rs, 0, 32), _col(rs, 1, 64), _col(rs, 2, 32)
    got = cv.schnorr_verify(px, sig, e)
    assert set(got.tolist()) <= {0, 1} and not _mismatch(got, rs)
    ok, all_valid = cv.schnorr_batch_verify(px, sig, e, flags=ecgpu.BATCH_EQUATION_ALWAYS)
    assert bytes(ok) == bytes(got) and all_valid is all(r.want for r in rs)
    # the valid rows alone - tangents and operands at infinity among them: the equation itself holds
    keep = [i for i, r in enumerate(rs) if r.want]
    ok, all_valid = cv.schnorr_batch_verify(px[keep], sig[keep], e[keep], flags=ecgpu.BATCH_EQUATION_ALWAYS | ecgpu.BATCH_VERDICT_ONLY)
    assert ok.tolist() == [1] * len(keep) and all_valid is True


@pytest.mark.parametrize("cn", CURVES)
def test_decompress_and_sec1_on_lift_rows(ctx, cn):
    c = M.CURVES[cn]
    cv = ctx.curve(cn)
    nb = c.nbytes
    rows = V.lift_rows(cn)
    xs = np.frombuffer(b"".join(x.to_bytes(nb, "big") for x, _ in rows), dtype=np.uint8).reshape(-1, nb).copy()
    out, ok = cv.decompress(xs, np.array([o for _, o in rows], dtype=np.uint8))
    hits = 0
    for i, (x, o) in enumerate(rows):
        want = M.decompress(c, x, o)
        if want is None:
            assert ok[i] == 0 and not out[i].any(), (i, hex(x))
        else:
            assert ok[i] == 1 and bytes(out[i]) == M.i2b(c, want[0]) + M.i2b(c, want[1]), (i, hex(x))
            hits += 1
    assert 16 <= hits <= len(rows) - 16
    # the same x under the tags 2, 3 and 5 (compact: the even root on secp256k1, the numerically smaller one on the NIST curves),
    # in short records and zero padded in wide ones
    for tag in (2, 3, 5):
        enc = np.zeros((len(rows), 1 + 2 * nb), dtype=np.uint8)
        enc[:, 0] = tag
        enc[:, 1:1 + nb] = xs
        for width in (1 + nb, 1 + 2 * nb):
            out, ok = cv.sec1_decode(np.ascontiguousarray(enc[:, :width]), record_bytes=width)
            for i, (x, _) in enumerate(rows):
                good, pt = M.group_from_bytes(c, bytes(enc[i, :1 + nb]))
                if not good:
                    assert ok[i] == 0 and not out[i].any(), (tag, i, hex(x))
                else:
                    assert ok[i] == 1 and bytes(out[i]) == M.i2b(c, pt[0]) + M.i2b(c, pt[1]), (tag, i, hex(x))


@pytest.mark.parametrize("cn", CURVES)
def test_validate_points_and_sec1_on_curve_check_rows(ctx, cn):
    c = M.CURVES[cn]
    cv = ctx.curve(cn)
    nb = c.nbytes
    rows = V.curve_check_rows(cn)
    xy = np.frombuffer(b"".join(x.to_bytes(nb, "big") + y.to_bytes(nb, "big") for x, y, _ in rows), dtype=np.uint8).reshape(-1, 2 * nb).copy()
    # validate_points takes the all-zero encoding for the identity; the uncompressed SEC1 record with tag 4 does not
    assert cv.validate_points(xy).tolist() == [1 if good or (x, y) == (0, 0) else 0 for x, y, good in rows]
    enc = np.zeros((len(rows), 1 + 2 * nb), dtype=np.uint8)
    enc[:, 0] = 4
    enc[:, 1:] = xy
    out, ok = cv.sec1_decode(enc)
    assert ok.tolist() == [1 if good else 0 for _, _, good in rows]
    for i, (_, _, good) in enumerate(rows):
        assert bytes(out[i]) == (bytes(xy[i]) if good else bytes(2 * nb)), i
    # the same keys under ECDSA verification: a key that is not canonical or not on the curve, or the identity, rejects a signature
    r = V.rows(cn, "ecdsa")[3 * V.T]
    assert r.cls == "chord" and r.want
    z, sg = _col([r] * len(rows), 0, nb), _col([r] * len(rows), 1, 2 * nb)
    rr, ss = M.b2i(r.inputs[1][:nb]), M.b2i(r.inputs[1][nb:])
    want = [1 if good and M.ecdsa_verify_prehashed(c, (x, y), r.inputs[0], rr, ss, reject_high_s=(cn == "k256")) else 0 for x, y, good in rows]
    assert cv.ecdsa_verify(z, sg, xy).tolist() == want and not any(want)
