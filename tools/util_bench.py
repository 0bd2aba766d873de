"""Throughput of the secondary entry points (SURVEY.md 8f rows and the element-wise field / point / scalar ops) on device-resident
batches: python tools/util_bench.py [log2n] [--scalar]   -> one line per (curve, operation), M elements/s

--scalar: the scalar-field rows only (ecgpu_scalar_op_batch, ecgpu_scalar_reduce_batch), plus the scalar inversion of every
SCALAR_INV_BATCH variant found in rustcrypto-elliptic-curves_amd/lib_exp/libecgpu_inv<B>_<curve>.so, built by
    make -C rustcrypto-elliptic-curves_amd variant NAME=inv<B>_<curve> TU=ops_<curve> DEFS=-DSCALAR_INV_BATCH=<B>"""
import ctypes
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "rustcrypto-elliptic-curves_amd"))
import torch
import ecgpu
from oracle import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
SCALAR_ONLY = "--scalar" in sys.argv
lg = int(args[0]) if args else 20
n = 1 << lg
ctx = ecgpu.Context(0)
lib, h = ctx.lib, ctx.handle
vp = ctypes.c_void_p


def P(t):
    return vp(t.data_ptr()) if t is not None else None


def timed(name, cn, fn, reps=3, lib=lib, h=h):
    best = 1e9
    for _ in range(reps):
        assert lib.ecgpu_timer_start(h) == 0
        rc = fn()
        ms = ctypes.c_float()
        assert lib.ecgpu_timer_stop(h, ctypes.byref(ms)) == 0
        assert rc in (0, None), (name, rc, lib.ecgpu_last_error(h))
        best = min(best, ms.value)
    print(f"{cn:5s} {name:34s} n=2^{lg}  {best:8.3f} ms  {n / best / 1e3:9.2f} M/s", flush=True)


SC_NAMES = ("mul", "sqr", "add", "sub", "neg", "invert", "sqrt")


def scalar_rows(cn, cid, nb, s, s2):
    """every scalar op and the reductions on device-resident scalars s, s2 (n x NB, valid)"""
    u8 = dict(dtype=torch.uint8, device="cuda")
    so, sk = torch.empty((n, nb), **u8), torch.empty((n,), **u8)
    for op, nm in enumerate(SC_NAMES):
        timed("scalar " + nm, cn, lambda op=op: lib.ecgpu_scalar_op_batch(h, cid, op, P(s), P(s2), P(so), P(sk), n, 1))
    for width, nm in ((nb, "scalar reduce (NB bytes)"), (2 * nb, "scalar reduce (2 NB bytes)"), (72 if nb == 48 else 48, "scalar reduce (FromOkm width)")):
        wide = torch.cat([s, s2], 1)[:, :width].contiguous()
        timed(nm, cn, lambda w=wide, width=width: lib.ecgpu_scalar_reduce_batch(h, cid, P(w), width, P(so), n, 1, 0))
        timed(nm.replace("reduce", "reduce_nonzero"), cn, lambda w=wide, width=width: lib.ecgpu_scalar_reduce_batch(h, cid, P(w), width, P(so), n, 1, 1))
    # the inversion at each SCALAR_INV_BATCH variant: a context of that library build on the same device buffers, checked against
    # the default build
    exp = os.path.join(ROOT, "rustcrypto-elliptic-curves_amd", "lib_exp")
    for b in (1, 8, 16, 32):
        path = os.path.join(exp, "libecgpu_inv%d_%s.so" % (b, cn))
        if not os.path.exists(path):
            continue
        vlib = ecgpu.load_library(path)
        vh = vp()
        assert vlib.ecgpu_create(ctypes.byref(vh), 0) == 0
        timed("scalar invert, SCALAR_INV_BATCH=%d" % b, cn, lambda: vlib.ecgpu_scalar_op_batch(vh, cid, 5, P(s), None, P(so), P(sk), n, 1),
              lib=vlib, h=vh)
        assert vlib.ecgpu_synchronize(vh) == 0
        ref = torch.empty_like(so)
        assert lib.ecgpu_scalar_op_batch(h, cid, 5, P(s), None, P(ref), None, n, 1) == 0
        ctx.synchronize()
        assert bool((ref == so).all()), "SCALAR_INV_BATCH=%d differs from the default build" % b
        vlib.ecgpu_destroy(vh)


for cn in ("k256", "p256", "p384"):
    cv = ctx.curve(cn)
    nb, cid = cv.nb, cv.id
    u8 = dict(dtype=torch.uint8, device="cuda")
    s = torch.empty((n, nb), **u8); s2 = torch.empty((n, nb), **u8)
    p = torch.empty((n, 2 * nb), **u8); o = torch.empty((n, 3 * nb), **u8); o2 = torch.empty((n, 3 * nb), **u8)
    f = torch.empty((n,), **u8); f2 = torch.empty((n,), **u8)
    cv.synth_scalars_device(s, n, synth.SEED, 0); cv.synth_scalars_device(s2, n, synth.SEED + 1, 0)
    cv.synth_points_device(p, n, synth.SEED, 0)
    ctx.synchronize()
    scalar_rows(cn, cid, nb, s, s2)
    if SCALAR_ONLY:
        del s, s2, p, o, o2
        torch.cuda.empty_cache()
        continue
    x = p[:, :nb].contiguous(); y = p[:, nb:].contiguous()
    fo = torch.empty((n, nb), **u8)
    for op, nm in ((0, "field mul"), (1, "field sqr"), (2, "field add"), (5, "field invert"), (6, "field sqrt")):
        timed(nm, cn, lambda op=op: lib.ecgpu_field_op_batch(h, cid, op, P(x), P(y), P(fo), n, 1))
    cv.mul_device(s, p, o, n, out_format=ecgpu.PROJECTIVE, flags=0)
    cv.mul_device(s2, p, o2, n, out_format=ecgpu.PROJECTIVE, flags=0)
    ctx.synchronize()
    q = torch.empty((n, 3 * nb), **u8)
    timed("point add (complete, X Y Z)", cn, lambda: lib.ecgpu_point_add_batch(h, cid, P(o), P(o2), P(q), n, 1))
    timed("point double", cn, lambda: lib.ecgpu_point_double_batch(h, cid, P(o), P(q), n, 1))
    timed("point eq", cn, lambda: lib.ecgpu_point_eq_batch(h, cid, P(o), P(o2), P(f), n, 1))
    xy = torch.empty((n, 2 * nb), **u8)
    timed("batch_normalize", cn, lambda: lib.ecgpu_batch_normalize(h, cid, P(q), P(xy), P(f), n, 1))
    timed("validate_points", cn, lambda: lib.ecgpu_validate_points(h, cid, P(p), P(f), n, 1))
    odd = (y[:, -1] & 1).contiguous()
    timed("decompress", cn, lambda: lib.ecgpu_decompress_batch(h, cid, P(x), P(odd), P(xy), P(f), n, 1))
    enc = torch.empty((n, nb + 1), **u8)
    timed("to_bytes (SEC1 compressed)", cn, lambda: lib.ecgpu_to_bytes_batch(h, cid, P(p), 0, P(enc), n, 1))
    timed("from_bytes", cn, lambda: lib.ecgpu_from_bytes_batch(h, cid, P(enc), P(xy), P(f), n, 1))
    unc = torch.empty((n, 2 * nb + 1), **u8)
    timed("sec1_encode (uncompressed)", cn, lambda: lib.ecgpu_sec1_encode_batch(h, cid, P(p), 0, 0, P(unc), n, 1))
    timed("sec1_decode (uncompressed)", cn, lambda: lib.ecgpu_sec1_decode_batch(h, cid, P(unc), 2 * nb + 1, P(xy), P(f), n, 1))
    timed("map_to_curve (2 elements, sum)", cn, lambda: lib.ecgpu_map_to_curve_batch(h, cid, P(torch.cat([x, y], 1)), 2, P(xy), P(f), n, 1))
    timed("mul_by_generator (throughput)", cn, lambda: cv.mul_device(s, None, xy, n))
    timed("mul_by_generator (reference, CT)", cn, lambda: cv.mul_device(s, None, xy, n, flags=ecgpu.EXACT_REFERENCE))
    timed("mul (throughput)", cn, lambda: cv.mul_device(s, p, xy, n))
    timed("mul (reference, CT)", cn, lambda: cv.mul_device(s, p, xy, n, flags=ecgpu.EXACT_REFERENCE), reps=2)
    timed("mul (SECRET_SCALARS: ECDH)", cn, lambda: cv.mul_device(s, p, xy, n, flags=ecgpu.SECRET_SCALARS), reps=2)
    keys = torch.empty((n, 2 * nb), **u8); sig = torch.empty((n, 2 * nb), **u8); rec = torch.empty((n,), **u8)
    cv.mul_device(s, None, keys, n)
    fl = cv.default_ecdsa_flags()
    timed("ecdsa sign (CT k G, default)", cn, lambda: cv.ecdsa_sign_device(s, s2, x, sig, rec, f, n, flags=fl), reps=2)
    timed("ecdsa sign (PUBLIC_SCALARS)", cn, lambda: cv.ecdsa_sign_device(s, s2, x, sig, rec, f, n, flags=fl | ecgpu.PUBLIC_SCALARS))
    timed("ecdsa verify", cn, lambda: cv.ecdsa_verify_device(x, sig, keys, f, n, flags=fl))
    ctx.synchronize()
    assert bool(f.all()), "verification of device-made signatures failed"
    timed("ecdsa recover", cn, lambda: lib.ecgpu_ecdsa_recover_batch(h, cid, P(x), P(sig), P(rec), P(xy), P(f2), n, 1, fl))
    ctx.synchronize()
    assert bool(f2.all()) and bool((xy == keys).all()), "recovery did not return the signing keys"
    del s, s2, p, o, o2, q, xy, keys, sig
    torch.cuda.empty_cache()
ctx.close()
