"""Host-side mirror of the reference's trait surface over the libecgpu C ABI (include/ecgpu.h).

The reference is a Rust workspace; no Rust toolchain exists in this image, so the host side
above the C ABI that tests and bench.py drive is this thin ctypes binding.  Names follow the
reference: `Curve.mul_by_generator` (MulByGenerator), `Curve.mul` (`&P * &k`), `Curve.lincomb`
(LinearCombination), `Curve.add / add_mixed / double` (ProjectivePoint), `Curve.batch_normalize`
(BatchNormalize), `Curve.field_*` (FieldElement).  The Rust shim that a maintainer would add is
in ../rust/ (source only) and described in INTEGRATION.md.

The boundary is written down once: `_PROTOTYPES` has one row per symbol of the header (checked against it, type class by type
class, by tests/test_abi_load.py), and every wrapper enters the library through `_call` (the position of every argument of every
wrapper is pinned by tests/test_binding_calls_cpu.py).  A new entry point is its table row and its wrapper.

There is no CPU fallback: if libecgpu.so is missing or no gfx950 device is present, every entry
point raises `EcgpuError`.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

try:  # one HIP runtime per process: let torch's bundled libamdhip64 load first so that libecgpu.so
    import torch  # noqa: F401  binds to the same copy (device pointers / streams are then shared)
except ImportError:  # torch is optional plumbing; the C ABI itself needs only the ROCm runtime
    torch = None

HOST, DEVICE = 0, 1
AFFINE, PROJECTIVE = 0, 1
EXACT_REFERENCE = 1
ECDSA_LOW_S = 2
PUBLIC_SCALARS = 4
SECRET_SCALARS = 8
BATCH_VERDICT_ONLY, BATCH_EQUATION_ALWAYS = 16, 32                     # ecgpu_schnorr_batch_verify*
SHARED_POINTS = 64                                                     # mul / lincomb / ecdsa_verify: `terms` host points (one key) for the whole batch
K256, P256, P384 = 0, 1, 2
CURVE_IDS = {"k256": K256, "p256": P256, "p384": P384}
FIELD_BYTES = {K256: 32, P256: 32, P384: 48}
FE_MUL, FE_SQR, FE_ADD, FE_SUB, FE_NEG, FE_INV, FE_SQRT = range(7)
SC_MUL, SC_SQR, SC_ADD, SC_SUB, SC_NEG, SC_INV, SC_SQRT = range(7)      # ecgpu_scalar_op
SC_BINARY = (SC_MUL, SC_ADD, SC_SUB)
REDUCE_NONZERO = 1
SHA256, SHA384 = 0, 1                                                  # ecgpu_hash
KECCAK256, SHA3_256, SHA3_384 = 16, 17, 18                             # the sponge family (csrc/keccak.hpp); Keccak-256 is Ethereum's hash, not SHA3-256
H2C_RO, H2C_NU = 0, 1                                                  # hash_from_bytes / encode_from_bytes
CURVE_HASH = {K256: SHA256, P256: SHA256, P384: SHA384}                # the hash of the curve's RFC 9380 suite
OKM_BYTES = {K256: 48, P256: 48, P384: 72}                             # FromOkm::Length
DIGEST_BYTES = {SHA256: 32, SHA384: 48, KECCAK256: 32, SHA3_256: 32, SHA3_384: 48}
# ecgpu_option (per-context tuning / test knobs, include/ecgpu.h)
(OPT_FB_WINDOW, OPT_FB_MAX_WINDOW, OPT_MSM_WINDOW_BITS, OPT_MSM_SLAB_TERMS, OPT_MSM_SMALL_PATH, OPT_MSM_ROUNDS, OPT_K256_WAVES, OPT_FB_MEMORY_BUDGET,
 OPT_LINCOMB_TERM_BY_TERM, OPT_SHARED_WINDOW, OPT_SHARED_MIN, OPT_SHARED_TABLE_BUDGET, OPT_SHARED_TABLE_BUILDS) = range(13)

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ECGPU_LIB: another build of the library (A/B measurements of compile-time switches); default: the in-tree build
LIB_PATH = os.environ.get("ECGPU_LIB") or os.path.join(_PKG_ROOT, "lib", "libecgpu.so")


# symbol -> (restype, argtypes): one row per prototype of include/ecgpu.h, in the header's order
vp, sz, i, u8p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
u, i64, u64, cstr = ctypes.c_uint, ctypes.c_int64, ctypes.c_uint64, ctypes.c_char_p
pp, szp, ip = ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(i)
_PROTOTYPES = {
    "ecgpu_create": (i, (pp, i)),
    "ecgpu_destroy": (None, (vp,)),
    "ecgpu_set_stream": (i, (vp, vp)),
    "ecgpu_use_own_stream": (i, (vp,)),
    "ecgpu_synchronize": (i, (vp,)),
    "ecgpu_last_error": (cstr, (vp,)),
    "ecgpu_last_error_copy": (i, (vp, cstr, sz)),
    "ecgpu_set_option": (i, (vp, i, i64)),
    "ecgpu_get_option": (i, (vp, i, ctypes.POINTER(i64))),
    "ecgpu_fb_table_bytes": (i, (vp, i, szp, ip)),
    "ecgpu_version": (cstr, ()),
    "ecgpu_field_bytes": (sz, (i,)),
    "ecgpu_host_alloc": (i, (vp, sz, pp)),
    "ecgpu_host_free": (i, (vp, vp)),
    "ecgpu_host_chunk_schedule": (i, (sz, sz, szp, sz)),
    "ecgpu_debug_workspace": (i, (vp, i, vp, sz, szp)),
    "ecgpu_timer_start": (i, (vp,)),
    "ecgpu_timer_stop": (i, (vp, ctypes.POINTER(ctypes.c_float))),
    "ecgpu_field_op_batch": (i, (vp, i, i, u8p, u8p, u8p, sz, i)),
    "ecgpu_scalar_op_batch": (i, (vp, i, i, u8p, u8p, u8p, u8p, sz, i)),
    "ecgpu_scalar_reduce_batch": (i, (vp, i, u8p, sz, u8p, sz, i, u)),
    "ecgpu_point_add_batch": (i, (vp, i, u8p, u8p, u8p, sz, i)),
    "ecgpu_point_add_mixed_batch": (i, (vp, i, u8p, u8p, u8p, sz, i)),
    "ecgpu_point_double_batch": (i, (vp, i, u8p, u8p, sz, i)),
    "ecgpu_point_eq_batch": (i, (vp, i, u8p, u8p, u8p, sz, i)),
    "ecgpu_batch_normalize": (i, (vp, i, u8p, u8p, u8p, sz, i)),
    "ecgpu_mul_batch": (i, (vp, i, u8p, u8p, i, u8p, i, u8p, sz, i, u)),
    "ecgpu_mul_batch_checked": (i, (vp, i, u8p, u8p, i, u8p, i, u8p, u8p, sz, i, u)),
    "ecgpu_lincomb_batch": (i, (vp, i, u8p, u8p, i, sz, u8p, i, u8p, sz, i, u)),
    "ecgpu_lincomb_batch_checked": (i, (vp, i, u8p, u8p, i, sz, u8p, i, u8p, u8p, sz, i, u)),
    "ecgpu_msm": (i, (vp, i, u8p, u8p, i, sz, u8p, i, i)),
    "ecgpu_validate_scalars": (i, (vp, i, u8p, u8p, sz, i)),
    "ecgpu_validate_points": (i, (vp, i, u8p, u8p, sz, i)),
    "ecgpu_decompress_batch": (i, (vp, i, u8p, u8p, u8p, u8p, sz, i)),
    "ecgpu_to_bytes_batch": (i, (vp, i, u8p, i, u8p, sz, i)),
    "ecgpu_from_bytes_batch": (i, (vp, i, u8p, u8p, u8p, sz, i)),
    "ecgpu_sec1_encode_batch": (i, (vp, i, u8p, i, i, u8p, sz, i)),
    "ecgpu_sec1_decode_batch": (i, (vp, i, u8p, sz, u8p, u8p, sz, i)),
    "ecgpu_ecdsa_verify_batch": (i, (vp, i, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_ecdsa_sign_batch": (i, (vp, i, u8p, u8p, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_rfc6979_nonce_batch": (i, (vp, i, u8p, u8p, u8p, u8p, sz, i)),
    "ecgpu_ecdsa_sign_prehash_batch": (i, (vp, i, u8p, u8p, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_ecdsa_recover_batch": (i, (vp, i, u8p, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_ecdh_batch": (i, (vp, i, u8p, u8p, u8p, u8p, sz, i)),
    "ecgpu_schnorr_verify_batch": (i, (vp, i, u8p, u8p, u8p, u8p, sz, i)),
    "ecgpu_schnorr_verify_prehash_batch": (i, (vp, i, u8p, u8p, u8p, u8p, sz, i)),
    "ecgpu_schnorr_sign_prehash_batch": (i, (vp, i, u8p, u8p, u8p, u8p, u8p, u8p, sz, i)),
    "ecgpu_map_to_curve_batch": (i, (vp, i, u8p, i, u8p, u8p, sz, i)),
    "ecgpu_hash_bytes": (sz, (i,)),
    "ecgpu_expand_message_xmd_batch": (i, (vp, i, u8p, sz, u8p, u8p, sz, u8p, sz, sz, i)),
    "ecgpu_field_from_okm_batch": (i, (vp, i, u8p, u8p, sz, i)),
    "ecgpu_hash_to_curve_batch": (i, (vp, i, u8p, sz, u8p, u8p, sz, i, u8p, u8p, sz, i)),
    "ecgpu_hash_to_scalar_batch": (i, (vp, i, u8p, sz, u8p, u8p, sz, u8p, sz, i)),
    "ecgpu_digest_batch": (i, (vp, i, u8p, sz, u8p, u8p, sz, i)),
    "ecgpu_ecdsa_sign_msg_batch": (i, (vp, i, u8p, u8p, sz, u8p, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_ecdsa_verify_msg_batch": (i, (vp, i, u8p, sz, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_ecdsa_recover_msg_batch": (i, (vp, i, u8p, sz, u8p, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_ecdsa_sign_digest_batch": (i, (vp, i, i, u8p, u8p, sz, u8p, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_ecdsa_verify_digest_batch": (i, (vp, i, i, u8p, sz, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_ecdsa_recover_digest_batch": (i, (vp, i, i, u8p, sz, u8p, u8p, u8p, u8p, u8p, sz, i, u)),
    "ecgpu_schnorr_sign_msg_batch": (i, (vp, i, u8p, u8p, sz, u8p, u8p, u8p, u8p, u8p, sz, i)),
    "ecgpu_schnorr_verify_msg_batch": (i, (vp, i, u8p, u8p, sz, u8p, u8p, u8p, sz, i)),
    "ecgpu_schnorr_batch_verify": (i, (vp, i, u8p, u8p, u8p, u8p, u8p, ip, sz, i, u)),
    "ecgpu_schnorr_batch_verify_prehash": (i, (vp, i, u8p, u8p, u8p, u8p, u8p, ip, sz, i, u)),
    "ecgpu_schnorr_batch_verify_msg": (i, (vp, i, u8p, u8p, sz, u8p, u8p, u8p, u8p, ip, sz, i, u)),
    "ecgpu_group_create": (i, (pp, ip, i, u)),
    "ecgpu_group_destroy": (None, (vp,)),
    "ecgpu_group_size": (i, (vp,)),
    "ecgpu_group_context": (vp, (vp, i)),
    "ecgpu_group_last_error": (cstr, (vp,)),
    "ecgpu_group_gather_path": (cstr, (vp,)),
    "ecgpu_group_synchronize": (i, (vp,)),
    "ecgpu_shard_range": (i, (sz, i, i, szp, szp)),
    "ecgpu_group_mul_batch": (i, (vp, i, u8p, u8p, i, u8p, i, u8p, sz, u)),
    "ecgpu_group_lincomb_batch": (i, (vp, i, u8p, u8p, i, sz, u8p, i, u8p, sz, u)),
    "ecgpu_group_lincomb_sharded": (i, (vp, i, pp, pp, i, sz, pp, i, pp, szp, u)),
    "ecgpu_group_msm": (i, (vp, i, u8p, u8p, i, sz, u8p, i)),
    "ecgpu_group_msm_sharded": (i, (vp, i, pp, pp, i, szp, u8p, i)),
    "ecgpu_synth_scalars": (i, (vp, i, u64, u64, u8p, sz)),
    "ecgpu_synth_points": (i, (vp, i, u64, u64, u8p, sz)),
}
del vp, sz, i, u8p, u, i64, u64, cstr, pp, szp, ip
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)


def host_chunk_schedule(n: int, pass_units: int) -> list:
    """chunk sizes of a host-buffer batch (ecgpu_host_chunk_schedule; no device needed)"""
    lib = load_library()
    cnt = lib.ecgpu_host_chunk_schedule(n, pass_units, None, 0)
    arr = (ctypes.c_size_t * max(cnt, 1))()
    lib.ecgpu_host_chunk_schedule(n, pass_units, arr, cnt)
    return list(arr[:cnt])


def shard_range(n: int, parts: int, index: int) -> tuple:
    """(first, count) of part `index` of n elements cut into `parts` balanced contiguous ranges (ecgpu_shard_range; no device needed)"""
    lib = load_library()
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    if lib.ecgpu_shard_range(n, parts, index, ctypes.byref(a), ctypes.byref(b)) != 0:
        raise ValueError("shard_range(%d, %d, %d)" % (n, parts, index))
    return a.value, b.value


class EcgpuError(RuntimeError):
    pass


_lib = None


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen libecgpu.so and declare every prototype of include/ecgpu.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise EcgpuError(f"{p} not found: build it with `make -C rustcrypto-elliptic-curves_amd` (no CPU fallback exists)")
    lib = ctypes.CDLL(p)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    if path is None:
        _lib = lib
    return lib


def _ptr(x):
    """Host numpy array / bytes -> (pointer, keepalive); torch CUDA tensor or int -> device pointer."""
    if x is None:
        return None, None
    if isinstance(x, int):
        return ctypes.c_void_p(x), None
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("the C ABI takes dense buffers: pass a C-contiguous array")
        return ctypes.c_void_p(x.ctypes.data), x
    if hasattr(x, "data_ptr"):  # torch tensor
        if not x.is_contiguous():
            raise ValueError("the C ABI takes dense buffers: pass a contiguous tensor")
        return ctypes.c_void_p(x.data_ptr()), x
    raise TypeError(type(x))


_AS_IS = (int, np.integer, ctypes._SimpleCData, ctypes.Array, type(ctypes.byref(ctypes.c_int())))


def _call(owner, name: str, *args):
    """The one path into the library: `owner` (a Context or a Group) gives the library, the handle that goes first and the
    check of the status.  Integers (sizes, flags, raw device pointers; Python's or numpy's), None and ctypes objects pass as they
    are, for ctypes to convert; everything else - numpy arrays, torch tensors - goes through _ptr and its checks.  `args` keeps
    the arrays alive until the call has returned."""
    owner.check(getattr(owner.lib, name)(owner.handle, *[a if a is None or isinstance(a, _AS_IS) else _ptr(a)[0] for a in args]))


def _curve_id(curve) -> int:
    return CURVE_IDS[curve] if isinstance(curve, str) else int(curve)


def _point_bytes(fmt: int, nb: int) -> int:
    return (3 if fmt == PROJECTIVE else 2) * nb


def _equal_lengths(what: str, *batches):
    """the batches of one call (arrays or message lists; None: an optional one that is absent) hold the same number of elements"""
    if len({len(b) for b in batches if b is not None}) > 1:
        raise ValueError(what + " batches differ in length")


def _host_messages(msgs: Sequence[bytes], aligned: bool = True) -> tuple:
    """the message arguments of a host batch: (records, or None where every message is empty; stride; lengths)"""
    rec, lens, stride = pack_messages_aligned(msgs) if aligned else pack_messages(msgs)
    return rec if stride else None, stride, lens


def _host_dst(dst: bytes) -> tuple:
    """(domain separation tag, or None for an empty one; its length)"""
    d = np.frombuffer(bytes(dst), dtype=np.uint8)
    return d if len(d) else None, len(d)


class Context:
    """One context per device (include/ecgpu.h: context section)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.handle = ctypes.c_void_p()
        rc = self.lib.ecgpu_create(ctypes.byref(self.handle), device)
        if rc != 0:
            raise EcgpuError(f"ecgpu_create(device={device}) failed with {rc} (no usable gfx950 GPU? there is no CPU fallback)")
        self.device = device
        self._pinned = []

    def close(self):
        if self.handle:
            for p in self._pinned:
                self.lib.ecgpu_host_free(self.handle, p)
            self._pinned = []
            self.lib.ecgpu_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc != 0:
            raise EcgpuError(f"ecgpu error {rc}: {self.lib.ecgpu_last_error(self.handle).decode()}")

    def set_stream(self, stream_handle: int):
        """All later launches go to this hipStream_t; 0 / None is the legacy default stream (PyTorch's default stream)."""
        _call(self, "ecgpu_set_stream", ctypes.c_void_p(stream_handle or None))

    def use_own_stream(self):
        """Back to the context's own (blocking) stream."""
        _call(self, "ecgpu_use_own_stream")

    def set_option(self, option: int, value: int):
        _call(self, "ecgpu_set_option", option, value)

    def get_option(self, option: int) -> int:
        v = ctypes.c_int64()
        _call(self, "ecgpu_get_option", option, ctypes.byref(v))
        return v.value

    def fb_table_bytes(self, curve) -> tuple:
        """(bytes of device memory held by the curve's generator tables, widest window among them)"""
        b, w = ctypes.c_size_t(), ctypes.c_int()
        _call(self, "ecgpu_fb_table_bytes", _curve_id(curve), ctypes.byref(b), ctypes.byref(w))
        return b.value, w.value

    def last_error(self) -> str:
        buf = ctypes.create_string_buffer(512)
        self.lib.ecgpu_last_error_copy(self.handle, buf, 512)
        return buf.value.decode()

    def debug_workspace(self, which: int) -> bytes:
        """contents of one of the context's device workspaces (ecgpu_debug_workspace): 0 table workspace, 1 ECDSA / ECDH
        intermediates, 2 MSM, 3 BIP340 challenges and message digests, 16 + i staging slot i (0 .. 27).  b"" if it does not exist yet."""
        b = ctypes.c_size_t()
        _call(self, "ecgpu_debug_workspace", which, None, 0, ctypes.byref(b))
        if not b.value:
            return b""
        buf = np.empty(b.value, dtype=np.uint8)
        _call(self, "ecgpu_debug_workspace", which, buf, b.value, ctypes.byref(b))
        return buf.tobytes()

    def synchronize(self):
        _call(self, "ecgpu_synchronize")

    def pinned_array(self, shape, dtype=np.uint8) -> np.ndarray:
        """numpy array over page-locked host memory (ecgpu_host_alloc); freed with the context."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        _call(self, "ecgpu_host_alloc", nbytes, ctypes.byref(p))
        self._pinned.append(p)
        buf = (ctypes.c_uint8 * max(nbytes, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def timer_start(self):
        _call(self, "ecgpu_timer_start")

    def timer_stop(self) -> float:
        ms = ctypes.c_float()
        _call(self, "ecgpu_timer_stop", ctypes.byref(ms))
        return ms.value

    def curve(self, name_or_id) -> "Curve":
        return Curve(self, _curve_id(name_or_id))


def _host_out(n: int, width: int) -> np.ndarray:
    return np.zeros((n, width), dtype=np.uint8)


def _host_flags(n: int) -> np.ndarray:
    """one byte per element: ok / inf / eq / recovery id"""
    return np.zeros(n, dtype=np.uint8)


def _as_host(x, width: int) -> np.ndarray:
    """bytes / list of bytes / ndarray -> (n, width) uint8."""
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, width)
    elif isinstance(x, (bytes, bytearray)):
        a = np.frombuffer(bytes(x), dtype=np.uint8).reshape(-1, width).copy()
    else:
        a = np.frombuffer(b"".join(x), dtype=np.uint8).reshape(-1, width).copy()
    return a


def pack_messages(msgs: Sequence[bytes], stride: Optional[int] = None):
    """list of byte strings -> (records (n, stride) uint8, lengths (n,) uint32, stride): the ragged-batch form of the hash entry
    points.  stride defaults to the longest message."""
    lens = np.array([len(m) for m in msgs], dtype=np.uint32)
    if stride is None:
        stride = int(lens.max()) if len(msgs) else 0
    if len(msgs) and int(lens.max()) > stride:
        raise ValueError("a message is longer than the stride (%d > %d)" % (int(lens.max()), stride))
    rec = np.zeros((len(msgs), stride), dtype=np.uint8)
    for k, m in enumerate(msgs):
        rec[k, :len(m)] = np.frombuffer(m, dtype=np.uint8)
    return rec, lens, stride


def pack_messages_aligned(msgs: Sequence[bytes]):
    """pack_messages with the stride padded to a multiple of 16: the records of a host batch are staged from an aligned base, so
    every one of them is 16-byte aligned and its whole blocks are read by words (csrc/sha2.hpp, update_aligned)"""
    longest = max((len(m) for m in msgs), default=0)
    return pack_messages(msgs, (longest + 15) // 16 * 16)


def digest(ctx: "Context", hash_id: int, msgs: Sequence[bytes]) -> np.ndarray:
    """SHA-256 / SHA-384 / Keccak-256 / SHA3-256 / SHA3-384 of every message on the device -> (n, 32 | 48) digests (ecgpu_digest_batch)"""
    m = _host_messages(msgs)
    out = _host_out(len(msgs), DIGEST_BYTES.get(hash_id, 48))
    _call(ctx, "ecgpu_digest_batch", hash_id, *m, out, len(msgs), HOST)
    return out


def digest_device(ctx: "Context", hash_id: int, d_msgs, msg_stride: int, d_msg_len, d_out, n: int):
    """the same over device buffers (d_msg_len may be None: every message is msg_stride bytes; d_out 4-byte aligned)"""
    _call(ctx, "ecgpu_digest_batch", hash_id, d_msgs, msg_stride, d_msg_len, d_out, n, DEVICE)


def expand_message_xmd(ctx: "Context", hash_id: int, msgs: Sequence[bytes], dst: bytes, out_bytes: int) -> np.ndarray:
    """ExpandMsgXmd::expand_message for a batch on the device -> (n, out_bytes) uniform bytes (ecgpu_expand_message_xmd_batch)"""
    m = _host_messages(msgs, aligned=False)
    out = _host_out(len(msgs), out_bytes)
    _call(ctx, "ecgpu_expand_message_xmd_batch", hash_id, *m, *_host_dst(dst), out, out_bytes, len(msgs), HOST)
    return out


class Curve:
    """Batch versions of the reference's per-curve arithmetic surface.

    Host-memory methods take/return numpy uint8 arrays shaped (n, bytes) in the canonical
    big-endian wire format; the `*_device` methods take raw device pointers / torch tensors and
    are asynchronous on the context stream."""

    def __init__(self, ctx: Context, cid: int):
        self.ctx, self.id, self.nb = ctx, cid, FIELD_BYTES[cid]

    def _call(self, name: str, *args):
        _call(self.ctx, name, self.id, *args)

    def _flags(self, flags: Optional[int]) -> int:
        return self.default_ecdsa_flags() if flags is None else flags

    # --- FieldElement -----------------------------------------------------------------------
    def field_op(self, op: int, a, b=None) -> np.ndarray:
        a = _as_host(a, self.nb)
        bb = _as_host(b, self.nb) if b is not None else None
        out = _host_out(len(a), self.nb)
        self._call("ecgpu_field_op_batch", op, a, bb, out, len(a), HOST)
        return out

    # --- Scalar ------------------------------------------------------------------------------
    def scalar_op(self, op: int, a, b=None):
        """Scalar::{mul, square, add, sub, negate, invert, sqrt} on canonical big-endian scalars -> (out, ok); ok[i] = 0 (and
        out[i] = 0) where the reference returns none: an operand >= n, the inverse of 0, the root of a non-residue"""
        a = _as_host(a, self.nb)
        if op in SC_BINARY and b is None:
            raise ValueError("scalar op %d needs b" % op)
        bb = _as_host(b, self.nb) if b is not None and op in SC_BINARY else None
        if bb is not None and len(bb) != len(a):
            raise ValueError("a and b differ in length (%d, %d)" % (len(a), len(bb)))
        out, ok = _host_out(len(a), self.nb), _host_flags(len(a))
        self._call("ecgpu_scalar_op_batch", op, a, bb, out, ok, len(a), HOST)
        return out, ok

    def scalar_op_device(self, op: int, d_a, d_b, d_out, d_ok, n: int):
        """scalar_op on device-resident scalars (torch tensors / device pointers); d_b may be None for unary ops, d_ok may be None"""
        self._check_device(d_a, n * self.nb, "d_a")
        if op in SC_BINARY:
            if d_b is None:
                raise ValueError("scalar op %d needs d_b" % op)
            self._check_device(d_b, n * self.nb, "d_b")
        self._check_device(d_out, n * self.nb, "d_out")
        self._check_device(d_ok, n, "d_ok")
        self._call("ecgpu_scalar_op_batch", op, d_a, d_b if op in SC_BINARY else None, d_out, d_ok, n, DEVICE)

    def scalar_reduce(self, data, nonzero: bool = False, in_bytes: Optional[int] = None) -> np.ndarray:
        """Reduce / ReduceNonZero / FromOkm: big-endian records of in_bytes bytes (1 .. 2 NB; default: the width of a 2-D
        array's rows) -> canonical scalars, int mod n or, with nonzero, int mod (n - 1) + 1"""
        if in_bytes is None:
            if not (isinstance(data, np.ndarray) and data.ndim == 2):
                raise ValueError("in_bytes is needed unless data is an (n, in_bytes) array")
            in_bytes = data.shape[1]
        d = _as_host(data, in_bytes)
        out = _host_out(len(d), self.nb)
        self._call("ecgpu_scalar_reduce_batch", d, in_bytes, out, len(d), HOST, REDUCE_NONZERO if nonzero else 0)
        return out

    # --- ProjectivePoint::{add, add_mixed, double}, BatchNormalize ------------------------------
    def add(self, p_xyz, q_xyz) -> np.ndarray:
        p, q = _as_host(p_xyz, 3 * self.nb), _as_host(q_xyz, 3 * self.nb)
        out = _host_out(len(p), 3 * self.nb)
        self._call("ecgpu_point_add_batch", p, q, out, len(p), HOST)
        return out

    def add_mixed(self, p_xyz, q_xy) -> np.ndarray:
        p, q = _as_host(p_xyz, 3 * self.nb), _as_host(q_xy, 2 * self.nb)
        out = _host_out(len(p), 3 * self.nb)
        self._call("ecgpu_point_add_mixed_batch", p, q, out, len(p), HOST)
        return out

    def double(self, p_xyz) -> np.ndarray:
        p = _as_host(p_xyz, 3 * self.nb)
        out = _host_out(len(p), 3 * self.nb)
        self._call("ecgpu_point_double_batch", p, out, len(p), HOST)
        return out

    def batch_normalize(self, p_xyz):
        p = _as_host(p_xyz, 3 * self.nb)
        out, inf = _host_out(len(p), 2 * self.nb), _host_flags(len(p))
        self._call("ecgpu_batch_normalize", p, out, inf, len(p), HOST)
        return out, inf

    def add_device(self, d_p_xyz, d_q_xyz, d_out_xyz, n: int):
        """complete addition on device-resident projective points (torch tensors / device pointers)"""
        for t, nm in ((d_p_xyz, "d_p_xyz"), (d_q_xyz, "d_q_xyz"), (d_out_xyz, "d_out_xyz")):
            self._check_device(t, n * 3 * self.nb, nm)
        self._call("ecgpu_point_add_batch", d_p_xyz, d_q_xyz, d_out_xyz, n, DEVICE)

    def batch_normalize_device(self, d_p_xyz, d_out_xy, d_out_inf, n: int):
        self._check_device(d_p_xyz, n * 3 * self.nb, "d_p_xyz")
        self._check_device(d_out_xy, n * 2 * self.nb, "d_out_xy")
        self._check_device(d_out_inf, n, "d_out_inf")
        self._call("ecgpu_batch_normalize", d_p_xyz, d_out_xy, d_out_inf, n, DEVICE)

    def point_eq(self, p_xyz, q_xyz) -> np.ndarray:
        """ProjectivePoint == ProjectivePoint (ct_eq) per element -> uint8 flags"""
        p, q = _as_host(p_xyz, 3 * self.nb), _as_host(q_xyz, 3 * self.nb)
        _equal_lengths("point", p, q)
        eq = _host_flags(len(p))
        self._call("ecgpu_point_eq_batch", p, q, eq, len(p), HOST)
        return eq

    # --- Mul<Scalar>, MulByGenerator, LinearCombination -----------------------------------------
    def lincomb(self, scalars, points, terms: int = 1, point_format: int = AFFINE, out_format: int = AFFINE, flags: int = 0,
                out=None, out_inf=None, checked: bool = False):
        """out / out_inf: optional preallocated result arrays (e.g. Context.pinned_array) instead of fresh ones.
        checked=True also returns scalar_ok (Scalar::from_repr: 0 where a scalar of the element is >= n).
        flags & SHARED_POINTS: `points` holds exactly `terms` affine points that every element uses (include/ecgpu.h)."""
        s = _as_host(scalars, self.nb)
        if terms < 1 or len(s) % terms:
            raise ValueError("the number of scalars is not a multiple of `terms`")
        n = len(s) // terms
        ow = _point_bytes(out_format, self.nb)
        p = _as_host(points, _point_bytes(point_format, self.nb)) if points is not None else None
        if flags & SHARED_POINTS:
            if p is None or point_format != AFFINE or len(p) != terms:
                raise ValueError("SHARED_POINTS takes exactly `terms` affine points (%d terms, %s points)" % (terms, "no" if p is None else len(p)))
        elif p is not None and len(p) != n * terms:
            raise ValueError("scalars and points differ in count (%d scalars, %d points)" % (len(s), len(p)))
        out = _host_out(n, ow) if out is None else out
        inf = _host_flags(n) if out_inf is None else out_inf
        if (out.shape != (n, ow) or out.dtype != np.uint8 or not out.flags.c_contiguous
                or inf.shape != (n,) or inf.dtype != np.uint8 or not inf.flags.c_contiguous):
            raise ValueError("out / out_inf have the wrong shape, dtype or layout")
        if checked:
            ok = _host_flags(n)
            self._call("ecgpu_lincomb_batch_checked", s, p, point_format, terms, out, out_format, inf, ok, n, HOST, flags)
            return (out, inf, ok) if out_format == AFFINE else (out, ok)
        self._call("ecgpu_lincomb_batch", s, p, point_format, terms, out, out_format, inf, n, HOST, flags)
        return (out, inf) if out_format == AFFINE else out

    def mul(self, scalars, points, point_format: int = AFFINE, out_format: int = AFFINE, flags: int = 0, out=None, out_inf=None):
        return self.lincomb(scalars, points, 1, point_format, out_format, flags, out, out_inf)

    def mul_by_generator(self, scalars, out_format: int = AFFINE, flags: int = 0):
        return self.lincomb(scalars, None, 1, AFFINE, out_format, flags)

    def diffie_hellman(self, secret_scalars, public_keys_xy) -> np.ndarray:
        """elliptic_curve::ecdh::diffie_hellman for a batch: SharedSecret = x((public * secret).to_affine())
        (k256/src/ecdh.rs:41-45).  Inputs are what the reference's types guarantee: non-zero scalars, valid keys.
        The scalars are secret: the multiplication runs on the constant-time variable-base kernels (csrc/varbase_ct.hpp on
        P-256 / P-384, csrc/varbase_ct_k256.hpp on secp256k1)."""
        shared, ok = self.ecdh(secret_scalars, public_keys_xy)
        if not ok.all():
            raise ValueError("diffie_hellman: element %d is not a NonZeroScalar / PublicKey pair" % int(np.argmin(ok)))
        return shared

    def ecdh(self, secret_scalars, public_keys_xy):
        """ecgpu_ecdh_batch -> (shared_x (n, NB), ok (n,)): ok = 0 and zeros for a zero / out-of-range secret or an invalid key"""
        d, q = _as_host(secret_scalars, self.nb), _as_host(public_keys_xy, 2 * self.nb)
        _equal_lengths("secret and public-key", d, q)
        out, ok = _host_out(len(d), self.nb), _host_flags(len(d))
        self._call("ecgpu_ecdh_batch", d, q, out, ok, len(d), HOST)
        return out, ok

    def ecdh_device(self, d_secret, d_pubkeys_xy, d_shared_x, d_ok, n: int):
        self._check_device(d_secret, n * self.nb, "d_secret")
        self._check_device(d_pubkeys_xy, n * 2 * self.nb, "d_pubkeys_xy")
        self._check_device(d_shared_x, n * self.nb, "d_shared_x")
        self._check_device(d_ok, n, "d_ok")
        self._call("ecgpu_ecdh_batch", d_secret, d_pubkeys_xy, d_shared_x, d_ok, n, DEVICE)

    def _check_device(self, t, need_bytes: int, what: str):
        """size check for torch tensors handed to the *_device methods (raw integer pointers cannot be checked)"""
        if t is not None and hasattr(t, "numel") and t.numel() * t.element_size() < need_bytes:
            raise ValueError("%s holds %d bytes, the call needs %d" % (what, t.numel() * t.element_size(), need_bytes))

    def mul_device(self, d_scalars, d_points, d_out, n: int, point_format: int = AFFINE, out_format: int = AFFINE,
                   d_out_inf=None, flags: int = 0):
        """flags & SHARED_POINTS: d_points is ONE affine point in HOST memory (bytes or a numpy array), whatever its name says."""
        self._check_device(d_scalars, n * self.nb, "d_scalars")
        if flags & SHARED_POINTS:
            d_points = _as_host(d_points, 2 * self.nb)
            if point_format != AFFINE or len(d_points) != 1:
                raise ValueError("SHARED_POINTS takes exactly one affine point in host memory")
        else:
            self._check_device(d_points, n * _point_bytes(point_format, self.nb), "d_points")
        self._check_device(d_out, n * _point_bytes(out_format, self.nb), "d_out")
        self._check_device(d_out_inf, n, "d_out_inf")
        self._call("ecgpu_mul_batch", d_scalars, d_points, point_format, d_out, out_format, d_out_inf, n, DEVICE, flags)

    def msm(self, scalars, points, point_format: int = AFFINE, out_format: int = AFFINE) -> np.ndarray:
        s = _as_host(scalars, self.nb)
        p = _as_host(points, _point_bytes(point_format, self.nb))
        if len(p) != len(s):
            raise ValueError("scalars and points differ in count (%d scalars, %d points)" % (len(s), len(p)))
        out = _host_out(1, _point_bytes(out_format, self.nb))
        self._call("ecgpu_msm", s, p, point_format, len(s), out, out_format, HOST)
        return out[0]

    def msm_device(self, d_scalars, d_points, n: int, d_out, point_format: int = AFFINE, out_format: int = AFFINE):
        self._check_device(d_scalars, n * self.nb, "d_scalars")
        self._check_device(d_points, n * _point_bytes(point_format, self.nb), "d_points")
        self._check_device(d_out, _point_bytes(out_format, self.nb), "d_out")
        self._call("ecgpu_msm", d_scalars, d_points, point_format, n, d_out, out_format, DEVICE)

    # --- decoding ---------------------------------------------------------------------------------
    def validate_scalars(self, scalars) -> np.ndarray:
        s = _as_host(scalars, self.nb)
        ok = _host_flags(len(s))
        self._call("ecgpu_validate_scalars", s, ok, len(s), HOST)
        return ok

    def validate_points(self, points_xy) -> np.ndarray:
        p = _as_host(points_xy, 2 * self.nb)
        ok = _host_flags(len(p))
        self._call("ecgpu_validate_points", p, ok, len(p), HOST)
        return ok

    def decompress(self, xs, y_is_odd):
        x = _as_host(xs, self.nb)
        odd = np.ascontiguousarray(y_is_odd, dtype=np.uint8)
        out, ok = _host_out(len(x), 2 * self.nb), _host_flags(len(x))
        self._call("ecgpu_decompress_batch", x, odd, out, ok, len(x), HOST)
        return out, ok

    # --- GroupEncoding::{to_bytes, from_bytes} ------------------------------------------------------
    def to_bytes(self, points, point_format: int = AFFINE) -> np.ndarray:
        p = _as_host(points, _point_bytes(point_format, self.nb))
        out = _host_out(len(p), self.nb + 1)
        self._call("ecgpu_to_bytes_batch", p, point_format, out, len(p), HOST)
        return out

    def from_bytes(self, encoded):
        e = _as_host(encoded, self.nb + 1)
        out, ok = _host_out(len(e), 2 * self.nb), _host_flags(len(e))
        self._call("ecgpu_from_bytes_batch", e, out, ok, len(e), HOST)
        return out, ok

    # --- ToEncodedPoint::to_encoded_point / FromEncodedPoint::from_encoded_point (fixed-width records) -------------
    def sec1_encode(self, points, compress: bool = False, point_format: int = AFFINE) -> np.ndarray:
        p = _as_host(points, _point_bytes(point_format, self.nb))
        out = _host_out(len(p), 1 + (1 if compress else 2) * self.nb)
        self._call("ecgpu_sec1_encode_batch", p, point_format, int(bool(compress)), out, len(p), HOST)
        return out

    def sec1_decode(self, encoded, record_bytes: Optional[int] = None):
        rb = record_bytes or (1 + 2 * self.nb)
        e = _as_host(encoded, rb)
        out, ok = _host_out(len(e), 2 * self.nb), _host_flags(len(e))
        self._call("ecgpu_sec1_decode_batch", e, rb, out, ok, len(e), HOST)
        return out, ok

    # --- ECDSA: VerifyPrimitive::verify_prehashed / SignPrimitive::try_sign_prehashed ------------------
    def default_ecdsa_flags(self) -> int:
        """secp256k1 is used with low-s rules in the reference (k256/src/ecdsa.rs:182-207), the NIST curves are not."""
        return ECDSA_LOW_S if self.id == K256 else 0

    def ecdsa_verify(self, prehash, sig_rs, pubkeys_xy, flags: Optional[int] = None) -> np.ndarray:
        """flags & SHARED_POINTS: pubkeys_xy is ONE key that every signature is checked against."""
        z, sg, q = _as_host(prehash, self.nb), _as_host(sig_rs, 2 * self.nb), _as_host(pubkeys_xy, 2 * self.nb)
        if self._flags(flags) & SHARED_POINTS:
            if len(q) != 1:
                raise ValueError("SHARED_POINTS takes exactly one public key (%d given)" % len(q))
            _equal_lengths("prehash and signature", z, sg)
        else:
            _equal_lengths("prehash, signature and public-key", z, sg, q)
        ok = _host_flags(len(z))
        self._call("ecgpu_ecdsa_verify_batch", z, sg, q, ok, len(z), HOST, self._flags(flags))
        return ok

    def ecdsa_verify_device(self, d_prehash, d_sig_rs, d_pubkeys_xy, d_ok, n: int, flags: Optional[int] = None):
        """flags & SHARED_POINTS: d_pubkeys_xy is ONE key in HOST memory (bytes or a numpy array), whatever its name says."""
        if self._flags(flags) & SHARED_POINTS:
            d_pubkeys_xy = _as_host(d_pubkeys_xy, 2 * self.nb)
            if len(d_pubkeys_xy) != 1:
                raise ValueError("SHARED_POINTS takes exactly one public key in host memory (%d given)" % len(d_pubkeys_xy))
        self._call("ecgpu_ecdsa_verify_batch", d_prehash, d_sig_rs, d_pubkeys_xy, d_ok, n, DEVICE, self._flags(flags))

    def map_to_curve(self, u, count: int = 1):
        """MapToCurve::map_to_curve (count = 1) or Q0 + Q1 of hash_from_bytes (count = 2) -> (points_xy, inf)"""
        uu = _as_host(u, self.nb)
        n = len(uu) // count
        out, inf = _host_out(n, 2 * self.nb), _host_flags(n)
        self._call("ecgpu_map_to_curve_batch", uu, count, out, inf, n, HOST)
        return out, inf

    # --- GroupDigest / FromOkm: everything that starts from bytes (SHA-2, expand_message_xmd and the reductions run on the device)
    def hash_to_curve(self, msgs: Sequence[bytes], dst: bytes, mode: int = H2C_RO):
        """GroupDigest::hash_from_bytes (H2C_RO) / encode_from_bytes (H2C_NU), one message per element -> (points_xy, inf)"""
        m = _host_messages(msgs, aligned=False)
        n = len(msgs)
        out, inf = _host_out(n, 2 * self.nb), _host_flags(n)
        self._call("ecgpu_hash_to_curve_batch", *m, *_host_dst(dst), mode, out, inf, n, HOST)
        return out, inf

    def hash_to_scalar(self, msgs: Sequence[bytes], dst: bytes) -> np.ndarray:
        """GroupDigest::hash_to_scalar -> (n, NB) canonical scalars"""
        m = _host_messages(msgs, aligned=False)
        out = _host_out(len(msgs), self.nb)
        self._call("ecgpu_hash_to_scalar_batch", *m, *_host_dst(dst), out, len(msgs), HOST)
        return out

    def field_from_okm(self, okm) -> np.ndarray:
        """FromOkm for FieldElement: big-endian records of L bytes (48, p384: 72) -> canonical field elements okm mod p"""
        o = _as_host(okm, OKM_BYTES[self.id])
        out = _host_out(len(o), self.nb)
        self._call("ecgpu_field_from_okm_batch", o, out, len(o), HOST)
        return out

    def expand_message_xmd(self, msgs: Sequence[bytes], dst: bytes, out_bytes: int) -> np.ndarray:
        """expand_message_xmd on the curve's own hash"""
        return expand_message_xmd(self.ctx, CURVE_HASH[self.id], msgs, dst, out_bytes)

    def schnorr_verify_prehash(self, pubkeys_x, sig_rs, prehashes) -> np.ndarray:
        """VerifyingKey::verify_prehash for a batch: the BIP340 challenge hashes are computed on the device as well"""
        x, sg, m = _as_host(pubkeys_x, self.nb), _as_host(sig_rs, 2 * self.nb), _as_host(prehashes, 32)
        _equal_lengths("key, signature and prehash", x, sg, m)
        ok = _host_flags(len(x))
        self._call("ecgpu_schnorr_verify_prehash_batch", x, sg, m, ok, len(x), HOST)
        return ok

    def ecdsa_recover(self, prehash, sig_rs, recovery_id, flags: Optional[int] = None):
        """VerifyingKey::recover_from_prehash for a batch -> (pubkeys_xy, ok)"""
        z, sg = _as_host(prehash, self.nb), _as_host(sig_rs, 2 * self.nb)
        rid = np.ascontiguousarray(recovery_id, dtype=np.uint8).reshape(-1)
        _equal_lengths("prehash, signature and recovery-id", z, sg, rid)
        out, ok = _host_out(len(z), 2 * self.nb), _host_flags(len(z))
        self._call("ecgpu_ecdsa_recover_batch", z, sg, rid, out, ok, len(z), HOST, self._flags(flags))
        return out, ok

    def ecdsa_recover_device(self, d_prehash, d_sig_rs, d_recid, d_pubkeys_xy, d_ok, n: int, flags: Optional[int] = None):
        self._call("ecgpu_ecdsa_recover_batch", d_prehash, d_sig_rs, d_recid, d_pubkeys_xy, d_ok, n, DEVICE, self._flags(flags))

    def schnorr_verify(self, pubkeys_x, sig_rs, challenges) -> np.ndarray:
        """EC part of BIP340 verification; challenges = tagged challenge hashes (ecgpu.schnorr computes them)."""
        x, sg, e = _as_host(pubkeys_x, self.nb), _as_host(sig_rs, 2 * self.nb), _as_host(challenges, self.nb)
        _equal_lengths("key, signature and challenge", x, sg, e)
        ok = _host_flags(len(x))
        self._call("ecgpu_schnorr_verify_batch", x, sg, e, ok, len(x), HOST)
        return ok

    def schnorr_verify_device(self, d_pubkeys_x, d_sig_rs, d_challenges, d_ok, n: int):
        self._call("ecgpu_schnorr_verify_batch", d_pubkeys_x, d_sig_rs, d_challenges, d_ok, n, DEVICE)

    def ecdsa_sign(self, secret_d, nonce_k, prehash, flags: Optional[int] = None):
        """-> (sig_rs, recovery_id, ok)"""
        d, k, z = _as_host(secret_d, self.nb), _as_host(nonce_k, self.nb), _as_host(prehash, self.nb)
        _equal_lengths("key, nonce and prehash", d, k, z)
        sig, rec, ok = _host_out(len(d), 2 * self.nb), _host_flags(len(d)), _host_flags(len(d))
        self._call("ecgpu_ecdsa_sign_batch", d, k, z, sig, rec, ok, len(d), HOST, self._flags(flags))
        return sig, rec, ok

    def ecdsa_sign_device(self, d_secret, d_nonce, d_prehash, d_sig_rs, d_recid, d_ok, n: int, flags: Optional[int] = None):
        self._call("ecgpu_ecdsa_sign_batch", d_secret, d_nonce, d_prehash, d_sig_rs, d_recid, d_ok, n, DEVICE, self._flags(flags))

    # --- deterministic signing: the nonce is derived on the device (RFC 6979 / BIP340) -------------------
    def rfc6979_nonce(self, secret_d, prehash, extra=None) -> np.ndarray:
        """the nonces SigningKey::sign_prehash derives (RFC 6979 on the curve's digest; `extra`: the additional data of the
        randomized forms, field-sized) -> (n, NB); zeros for a key outside [1, n-1]"""
        d, z = _as_host(secret_d, self.nb), _as_host(prehash, self.nb)
        x = None if extra is None else _as_host(extra, self.nb)
        _equal_lengths("key, prehash and additional-data", d, z, x)
        k = _host_out(len(d), self.nb)
        self._call("ecgpu_rfc6979_nonce_batch", d, z, x, k, len(d), HOST)
        return k

    def rfc6979_nonce_device(self, d_secret, d_prehash, d_extra, d_out_k, n: int):
        self._call("ecgpu_rfc6979_nonce_batch", d_secret, d_prehash, d_extra, d_out_k, n, DEVICE)

    def ecdsa_sign_prehash(self, secret_d, prehash, extra=None, flags: Optional[int] = None):
        """PrehashSigner::sign_prehash (extra=None) / RandomizedPrehashSigner (extra given) for a batch -> (sig_rs, recovery_id, ok)"""
        d, z = _as_host(secret_d, self.nb), _as_host(prehash, self.nb)
        x = None if extra is None else _as_host(extra, self.nb)
        _equal_lengths("key, prehash and additional-data", d, z, x)
        sig, rec, ok = _host_out(len(d), 2 * self.nb), _host_flags(len(d)), _host_flags(len(d))
        self._call("ecgpu_ecdsa_sign_prehash_batch", d, z, x, sig, rec, ok, len(d), HOST, self._flags(flags))
        return sig, rec, ok

    def ecdsa_sign_prehash_device(self, d_secret, d_prehash, d_extra, d_sig_rs, d_recid, d_ok, n: int, flags: Optional[int] = None):
        self._call("ecgpu_ecdsa_sign_prehash_batch", d_secret, d_prehash, d_extra, d_sig_rs, d_recid, d_ok, n, DEVICE, self._flags(flags))

    def schnorr_sign_prehash(self, secret_keys, prehashes, aux_rands):
        """BIP340 SigningKey::sign_prehash_with_aux_rand for a batch (secp256k1) -> (sig_rs, pubkeys_x, ok)"""
        d, m, a = _as_host(secret_keys, self.nb), _as_host(prehashes, 32), _as_host(aux_rands, 32)
        _equal_lengths("key, prehash and aux_rand", d, m, a)
        sig, px, ok = _host_out(len(d), 2 * self.nb), _host_out(len(d), self.nb), _host_flags(len(d))
        self._call("ecgpu_schnorr_sign_prehash_batch", d, m, a, sig, px, ok, len(d), HOST)
        return sig, px, ok

    def schnorr_sign_prehash_device(self, d_secret, d_prehash, d_aux, d_sig_rs, d_pubkeys_x, d_ok, n: int):
        self._call("ecgpu_schnorr_sign_prehash_batch", d_secret, d_prehash, d_aux, d_sig_rs, d_pubkeys_x, d_ok, n, DEVICE)

    # --- from message bytes: the curve's own digest runs on the device, then the prehash pipeline -------------
    def digest(self, msgs: Sequence[bytes]) -> np.ndarray:
        """the curve's own digest of every message (SHA-256; P-384: SHA-384) -> (n, NB)"""
        return digest(self.ctx, CURVE_HASH[self.id], msgs)

    def ecdsa_sign_msg(self, secret_d, msgs: Sequence[bytes], extra=None, flags: Optional[int] = None):
        """Signer::sign (extra=None) / RandomizedSigner::sign_with_rng (extra given) for a batch -> (sig_rs, recovery_id, ok)"""
        return self._ecdsa_sign_msgs("ecgpu_ecdsa_sign_msg_batch", (), secret_d, msgs, extra, flags)

    def _ecdsa_sign_msgs(self, name: str, hash_arg: tuple, secret_d, msgs, extra, flags):
        """the message-level signing calls: on the curve's own digest (hash_arg empty) or on a chosen one (hash_arg = (hash_id,))"""
        d = _as_host(secret_d, self.nb)
        x = None if extra is None else _as_host(extra, self.nb)
        _equal_lengths("key, message and additional-data", d, msgs, x)
        m = _host_messages(msgs)
        sig, rid, ok = _host_out(len(d), 2 * self.nb), _host_flags(len(d)), _host_flags(len(d))
        self._call(name, *hash_arg, d, *m, x, sig, rid, ok, len(d), HOST, self._flags(flags))
        return sig, rid, ok

    def ecdsa_sign_msg_device(self, d_secret, d_msgs, msg_stride: int, d_msg_len, d_extra, d_sig_rs, d_recid, d_ok, n: int, flags: Optional[int] = None):
        self._call("ecgpu_ecdsa_sign_msg_batch", d_secret, d_msgs, msg_stride, d_msg_len, d_extra, d_sig_rs, d_recid, d_ok, n, DEVICE, self._flags(flags))

    def ecdsa_verify_msg(self, msgs: Sequence[bytes], sig_rs, pubkeys_xy, flags: Optional[int] = None) -> np.ndarray:
        """Verifier::verify for a batch -> ok"""
        return self._ecdsa_verify_msgs("ecgpu_ecdsa_verify_msg_batch", (), msgs, sig_rs, pubkeys_xy, flags)

    def _ecdsa_verify_msgs(self, name: str, hash_arg: tuple, msgs, sig_rs, pubkeys_xy, flags):
        sg, q = _as_host(sig_rs, 2 * self.nb), _as_host(pubkeys_xy, 2 * self.nb)
        _equal_lengths("message, signature and public-key", msgs, sg, q)
        m = _host_messages(msgs)
        ok = _host_flags(len(sg))
        self._call(name, *hash_arg, *m, sg, q, ok, len(sg), HOST, self._flags(flags))
        return ok

    def ecdsa_verify_msg_device(self, d_msgs, msg_stride: int, d_msg_len, d_sig_rs, d_pubkeys_xy, d_ok, n: int, flags: Optional[int] = None):
        self._call("ecgpu_ecdsa_verify_msg_batch", d_msgs, msg_stride, d_msg_len, d_sig_rs, d_pubkeys_xy, d_ok, n, DEVICE, self._flags(flags))

    def ecdsa_recover_msg(self, msgs: Sequence[bytes], sig_rs, recovery_id, flags: Optional[int] = None):
        """VerifyingKey::recover_from_msg for a batch -> (pubkeys_xy, ok)"""
        return self._ecdsa_recover_msgs("ecgpu_ecdsa_recover_msg_batch", (), msgs, sig_rs, recovery_id, flags)

    def _ecdsa_recover_msgs(self, name: str, hash_arg: tuple, msgs, sig_rs, recovery_id, flags):
        sg = _as_host(sig_rs, 2 * self.nb)
        rid = np.ascontiguousarray(recovery_id, dtype=np.uint8).reshape(-1)
        _equal_lengths("message, signature and recovery-id", msgs, sg, rid)
        m = _host_messages(msgs)
        out, ok = _host_out(len(sg), 2 * self.nb), _host_flags(len(sg))
        self._call(name, *hash_arg, *m, sg, rid, out, ok, len(sg), HOST, self._flags(flags))
        return out, ok

    # --- DigestSigner / DigestVerifier / recover_from_digest: the message-level calls on a chosen digest of the field's size ---
    def ecdsa_sign_digest(self, hash_id: int, secret_d, msgs: Sequence[bytes], extra=None, flags: Optional[int] = None):
        """DigestSigner::sign_digest / sign_digest_recoverable (extra=None) / RandomizedDigestSigner (extra given) for a batch, the
        messages hashed with hash_id on the device -> (sig_rs, recovery_id, ok).  The RFC 6979 nonce keeps the curve's own hash."""
        return self._ecdsa_sign_msgs("ecgpu_ecdsa_sign_digest_batch", (hash_id,), secret_d, msgs, extra, flags)

    def ecdsa_sign_digest_device(self, hash_id: int, d_secret, d_msgs, msg_stride: int, d_msg_len, d_extra, d_sig_rs, d_recid, d_ok, n: int,
                                 flags: Optional[int] = None):
        self._call("ecgpu_ecdsa_sign_digest_batch", hash_id, d_secret, d_msgs, msg_stride, d_msg_len, d_extra, d_sig_rs, d_recid, d_ok, n, DEVICE,
                   self._flags(flags))

    def ecdsa_verify_digest(self, hash_id: int, msgs: Sequence[bytes], sig_rs, pubkeys_xy, flags: Optional[int] = None) -> np.ndarray:
        """DigestVerifier::verify_digest for a batch -> ok"""
        return self._ecdsa_verify_msgs("ecgpu_ecdsa_verify_digest_batch", (hash_id,), msgs, sig_rs, pubkeys_xy, flags)

    def ecdsa_verify_digest_device(self, hash_id: int, d_msgs, msg_stride: int, d_msg_len, d_sig_rs, d_pubkeys_xy, d_ok, n: int, flags: Optional[int] = None):
        self._call("ecgpu_ecdsa_verify_digest_batch", hash_id, d_msgs, msg_stride, d_msg_len, d_sig_rs, d_pubkeys_xy, d_ok, n, DEVICE, self._flags(flags))

    def ecdsa_recover_digest(self, hash_id: int, msgs: Sequence[bytes], sig_rs, recovery_id, flags: Optional[int] = None):
        """VerifyingKey::recover_from_digest for a batch -> (pubkeys_xy, ok)"""
        return self._ecdsa_recover_msgs("ecgpu_ecdsa_recover_digest_batch", (hash_id,), msgs, sig_rs, recovery_id, flags)

    def ecdsa_recover_digest_device(self, hash_id: int, d_msgs, msg_stride: int, d_msg_len, d_sig_rs, d_recid, d_pubkeys_xy, d_ok, n: int,
                                    flags: Optional[int] = None):
        self._call("ecgpu_ecdsa_recover_digest_batch", hash_id, d_msgs, msg_stride, d_msg_len, d_sig_rs, d_recid, d_pubkeys_xy, d_ok, n, DEVICE,
                   self._flags(flags))

    def schnorr_sign_msg(self, secret_keys, msgs: Sequence[bytes], aux_rands=None):
        """BIP340 Signer::try_sign (aux_rands=None: 32 zero bytes) / try_sign_with_rng over SHA256(msg) for a batch (secp256k1)
        -> (sig_rs, pubkeys_x, ok)"""
        d = _as_host(secret_keys, self.nb)
        a = None if aux_rands is None else _as_host(aux_rands, 32)
        _equal_lengths("key, message and aux_rand", d, msgs, a)
        m = _host_messages(msgs)
        sig, px, ok = _host_out(len(d), 2 * self.nb), _host_out(len(d), self.nb), _host_flags(len(d))
        self._call("ecgpu_schnorr_sign_msg_batch", d, *m, a, sig, px, ok, len(d), HOST)
        return sig, px, ok

    def schnorr_verify_msg(self, pubkeys_x, msgs: Sequence[bytes], sig_rs) -> np.ndarray:
        """BIP340 Verifier::verify over SHA256(msg) for a batch (secp256k1) -> ok"""
        x, sg = _as_host(pubkeys_x, self.nb), _as_host(sig_rs, 2 * self.nb)
        _equal_lengths("key, message and signature", x, sg, msgs)
        m = _host_messages(msgs)
        ok = _host_flags(len(x))
        self._call("ecgpu_schnorr_verify_msg_batch", x, *m, sg, ok, len(x), HOST)
        return ok

    # --- BIP340 batch verification: one equation per batch (include/ecgpu.h).  seed=None: the library draws one per call -------
    @staticmethod
    def _batch_seed(seed):
        if seed is None:
            return None
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("the seed of a batch verification is 32 bytes")
        return np.frombuffer(seed, dtype=np.uint8)

    def _schnorr_batch_host(self, name: str, pubkeys_x, sig_rs, third, seed, flags: int):
        x, sg, t = _as_host(pubkeys_x, self.nb), _as_host(sig_rs, 2 * self.nb), _as_host(third, 32)
        _equal_lengths("key, signature and challenge / prehash", x, sg, t)
        ok, all_valid, sd = _host_flags(len(x)), ctypes.c_int(0), self._batch_seed(seed)
        self._call(name, x, sg, t, sd, ok, ctypes.byref(all_valid), len(x), HOST, flags)
        return ok, bool(all_valid.value)

    def schnorr_batch_verify(self, pubkeys_x, sig_rs, challenges, seed=None, flags: int = 0):
        """BIP340 batch verification from the challenge hashes -> (ok, all_valid)"""
        return self._schnorr_batch_host("ecgpu_schnorr_batch_verify", pubkeys_x, sig_rs, challenges, seed, flags)

    def schnorr_batch_verify_prehash(self, pubkeys_x, sig_rs, prehashes, seed=None, flags: int = 0):
        """BIP340 batch verification from the 32-byte digests -> (ok, all_valid); ok as schnorr_verify_prehash gives it"""
        return self._schnorr_batch_host("ecgpu_schnorr_batch_verify_prehash", pubkeys_x, sig_rs, prehashes, seed, flags)

    def schnorr_batch_verify_prehash_device(self, d_pubkeys_x, d_sig_rs, d_prehash, d_ok, n: int, seed=None, flags: int = 0):
        """device-resident batch (d_ok may be None with BATCH_VERDICT_ONLY) -> (d_ok, all_valid); the call synchronises the stream"""
        all_valid, sd = ctypes.c_int(0), self._batch_seed(seed)
        self._call("ecgpu_schnorr_batch_verify_prehash", d_pubkeys_x, d_sig_rs, d_prehash, sd, d_ok, ctypes.byref(all_valid), n, DEVICE, flags)
        return d_ok, bool(all_valid.value)

    def schnorr_batch_verify_msg(self, pubkeys_x, msgs: Sequence[bytes], sig_rs, seed=None, flags: int = 0):
        """BIP340 batch verification over SHA256(msg) -> (ok, all_valid)"""
        x, sg = _as_host(pubkeys_x, self.nb), _as_host(sig_rs, 2 * self.nb)
        _equal_lengths("key, message and signature", x, sg, msgs)
        m = _host_messages(msgs)
        ok, all_valid, sd = _host_flags(len(x)), ctypes.c_int(0), self._batch_seed(seed)
        self._call("ecgpu_schnorr_batch_verify_msg", x, *m, sg, sd, ok, ctypes.byref(all_valid), len(x), HOST, flags)
        return ok, bool(all_valid.value)

    # --- synthetic inputs (device buffers) ---------------------------------------------------------
    def synth_scalars_device(self, d_out, n: int, seed: int, first_index: int = 0):
        self._call("ecgpu_synth_scalars", seed, first_index, d_out, n)

    def synth_points_device(self, d_out, n: int, seed: int, first_index: int = 0):
        self._call("ecgpu_synth_points", seed, first_index, d_out, n)


GROUP_NO_RCCL = 1


class _BorrowedContext(Context):
    """a group member's context (owned by the group: never destroyed from here)"""

    def __init__(self, lib, handle, device):
        self.lib, self.handle, self.device, self._pinned = lib, ctypes.c_void_p(handle), device, []

    def close(self):
        for p in self._pinned:
            self.lib.ecgpu_host_free(self.handle, p)
        self._pinned = []
        self.handle = ctypes.c_void_p()


class Group:
    """Device group (include/ecgpu.h, "device groups"): the single-call entry points split over several GPUs - contiguous index
    ranges for independent batches (no collective), per-device bucket method + all-gather of one point per device + fold for one
    split sum.  `devices` may repeat a device (two contexts on one card)."""

    def __init__(self, devices: Sequence[int], flags: int = 0):
        self.lib = load_library()
        self.handle = ctypes.c_void_p()
        arr = (ctypes.c_int * len(devices))(*devices)
        rc = self.lib.ecgpu_group_create(ctypes.byref(self.handle), arr, len(devices), flags)
        if rc != 0:
            raise EcgpuError(f"ecgpu_group_create({list(devices)}) failed with {rc} (no usable gfx950 GPU? there is no CPU fallback)")
        self.devices = list(devices)
        self.size = len(devices)
        self.members = [_BorrowedContext(self.lib, self.lib.ecgpu_group_context(self.handle, i), d) for i, d in enumerate(devices)]

    def close(self):
        if self.handle:
            for m in self.members:
                m.close()
            self.lib.ecgpu_group_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc != 0:
            raise EcgpuError(f"ecgpu group error {rc}: {self.lib.ecgpu_group_last_error(self.handle).decode()}")

    def context(self, index: int) -> Context:
        return self.members[index]

    def gather_path(self) -> str:
        return self.lib.ecgpu_group_gather_path(self.handle).decode()

    def synchronize(self):
        _call(self, "ecgpu_group_synchronize")

    def lincomb(self, curve, scalars, points, terms: int = 1, point_format: int = AFFINE, out_format: int = AFFINE, flags: int = 0, out=None, out_inf=None):
        if flags & SHARED_POINTS:
            raise ValueError("SHARED_POINTS is for the single-context calls: the group forms take per-element points")
        cid = _curve_id(curve)
        nb = FIELD_BYTES[cid]
        s = _as_host(scalars, nb)
        n = len(s) // terms
        p = _as_host(points, _point_bytes(point_format, nb)) if points is not None else None
        if len(s) % terms or (p is not None and len(p) != n * terms):
            raise ValueError("scalars and points differ in count")
        out = _host_out(n, _point_bytes(out_format, nb)) if out is None else out
        inf = _host_flags(n) if out_inf is None else out_inf
        _call(self, "ecgpu_group_lincomb_batch", cid, s, p, point_format, terms, out, out_format, inf, n, flags)
        return (out, inf) if out_format == AFFINE else out

    def mul(self, curve, scalars, points, **kw):
        return self.lincomb(curve, scalars, points, 1, **kw)

    def msm(self, curve, scalars, points, point_format: int = AFFINE, out_format: int = AFFINE) -> np.ndarray:
        cid = _curve_id(curve)
        nb = FIELD_BYTES[cid]
        s = _as_host(scalars, nb)
        p = _as_host(points, _point_bytes(point_format, nb))
        if len(p) != len(s):
            raise ValueError("scalars and points differ in count")
        out = _host_out(1, _point_bytes(out_format, nb))
        _call(self, "ecgpu_group_msm", cid, s, p, point_format, len(s), out, out_format)
        return out[0]

    @staticmethod
    def _ptr_array(xs):
        return (ctypes.c_void_p * len(xs))(*[(_ptr(x)[0].value if x is not None else None) for x in xs])

    def lincomb_sharded(self, curve, d_scalars, d_points, d_out, counts, terms: int = 1, point_format: int = AFFINE, out_format: int = AFFINE, d_out_inf=None,
                        flags: int = 0):
        """device-resident shards (lists of torch tensors / device pointers, one per member); asynchronous: Group.synchronize()"""
        cnt = (ctypes.c_size_t * self.size)(*counts)
        _call(self, "ecgpu_group_lincomb_sharded", _curve_id(curve), self._ptr_array(d_scalars), self._ptr_array(d_points) if d_points is not None else None,
                   point_format, terms, self._ptr_array(d_out), out_format, self._ptr_array(d_out_inf) if d_out_inf is not None else None, cnt, flags)

    def msm_sharded(self, curve, d_scalars, d_points, counts, point_format: int = AFFINE, out_format: int = AFFINE) -> np.ndarray:
        cid = _curve_id(curve)
        cnt = (ctypes.c_size_t * self.size)(*counts)
        out = _host_out(1, _point_bytes(out_format, FIELD_BYTES[cid]))
        _call(self, "ecgpu_group_msm_sharded", cid, self._ptr_array(d_scalars), self._ptr_array(d_points), point_format, cnt, out, out_format)
        return out[0]
