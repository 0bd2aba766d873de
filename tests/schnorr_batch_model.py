"""Model of BIP340 batch verification (csrc/schnorr_batch_kernels.hpp, include/ecgpu.h "batch verification"): the coefficients with
hashlib, the term list of a batch, and the equation evaluated with the oracle's affine arithmetic.  Independent of the library."""
import hashlib
import struct

from oracle import ecmodel as M

C = M.K256
N, P = C.n, C.p
G = (C.gx, C.gy)
TAG = hashlib.sha256(b"ecgpu/BIP340/batch-coefficient").digest()


def coefficient(seed: bytes, index: int) -> int:
    """a_i: the first 16 bytes, big-endian, of SHA256(tag || tag || seed32 || be64(i)); 0 becomes 1"""
    assert len(seed) == 32
    a = int.from_bytes(hashlib.sha256(TAG + TAG + seed + struct.pack(">Q", index)).digest()[:16], "big")
    return a or 1


def challenge(px: bytes, prehash: bytes, sig: bytes) -> bytes:
    return M._tagged_hash(b"BIP0340/challenge", sig[:32], px, prehash)


def lift_x(x: int):
    """the curve point with this x and an even y, or None"""
    if x >= P:
        return None
    return M.decompress(C, x, 0)


def decodes(px: bytes, sig: bytes) -> bool:
    """the decode flag: r in [1, p) an x-coordinate, s in [1, n), a key with a curve point"""
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    return 0 < r < P and 0 < s < N and lift_x(int.from_bytes(px, "big")) is not None and lift_x(r) is not None


def terms(pubkeys_x, sigs, challenges, seed: bytes, first_index: int = 0):
    """-> (dec, [(k_j, Q_j)] of 2u + 1 terms): 2i = (a_i, R_i), 2i + 1 = (a_i e_i mod n, P_i), 2u = (n - sum a_i s_i mod n, G); a
    left-out element is (0, G), (0, G)"""
    dec, out, t = [], [], 0
    for i, (px, sig, e) in enumerate(zip(pubkeys_x, sigs, challenges)):
        ok = decodes(px, sig)
        dec.append(1 if ok else 0)
        if not ok:
            out += [(0, G), (0, G)]
            continue
        a = coefficient(seed, first_index + i)
        ee = int.from_bytes(e, "big") % N
        out += [(a, lift_x(int.from_bytes(sig[:32], "big"))), (a * ee % N, lift_x(int.from_bytes(px, "big")))]
        t += a * int.from_bytes(sig[32:], "big")
    out.append(((N - t % N) % N, G))
    return dec, out


def combination(term_list):
    """sum k_j Q_j in the oracle's affine model (None: the identity)"""
    acc = None
    for k, q in term_list:
        acc = M.affine_add(C, acc, M.affine_mul(C, k, q))
    return acc


def equation_holds(pubkeys_x, sigs, challenges, seed: bytes, first_index: int = 0) -> bool:
    return combination(terms(pubkeys_x, sigs, challenges, seed, first_index)[1]) is None


def parse_terms(scalars: bytes, points: bytes):
    """the wire layout (32-byte big-endian scalars, 64-byte x || y points) -> [(k, (x, y))]"""
    cnt = len(scalars) // 32
    assert len(points) == 64 * cnt
    return [(int.from_bytes(scalars[32 * j:32 * j + 32], "big"),
             (int.from_bytes(points[64 * j:64 * j + 32], "big"), int.from_bytes(points[64 * j + 32:64 * j + 64], "big"))) for j in range(cnt)]
