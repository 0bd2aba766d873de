"""BIP340 Schnorr over secp256k1 for batches: host side of k256/src/schnorr/{signing,verifying}.rs.

Host: tagged SHA-256 hashes (challenge, aux, nonce: k256/src/schnorr.rs:180-186, signing.rs:80-118) and scalar
arithmetic mod n (Python integers).  Device: every elliptic-curve operation - `Curve.schnorr_verify` for verification,
`Curve.mul_by_generator` for the public keys and nonce points of signing.  No CPU curve arithmetic exists here."""
from __future__ import annotations

import hashlib
from typing import Sequence

import numpy as np

from . import K256, Curve

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def tagged_hash(tag: bytes, *parts: bytes) -> bytes:
    t = hashlib.sha256(tag).digest()
    h = hashlib.sha256(t + t)
    for p in parts:
        h.update(p)
    return h.digest()


def challenges(pubkeys_x: Sequence[bytes], prehashes: Sequence[bytes], sigs: Sequence[bytes]) -> bytes:
    return b"".join(tagged_hash(b"BIP0340/challenge", s[:32], px, m) for px, m, s in zip(pubkeys_x, prehashes, sigs))


def verify_batch(curve: Curve, pubkeys_x: Sequence[bytes], prehashes: Sequence[bytes], sigs: Sequence[bytes]) -> np.ndarray:
    """ok[i] = 1 iff sigs[i] (64 bytes r || s) verifies over the 32-byte prehashes[i] under the x-only key."""
    if curve.id != K256:
        raise ValueError("BIP340 is defined over secp256k1")
    if any(len(m) != 32 for m in prehashes):
        raise ValueError("verify_prehash takes 32-byte digests")     # verifying.rs:68
    return curve.schnorr_verify(b"".join(pubkeys_x), b"".join(sigs), challenges(pubkeys_x, prehashes, sigs))


def verify_batch_device(curve: Curve, pubkeys_x: Sequence[bytes], prehashes: Sequence[bytes], sigs: Sequence[bytes]) -> np.ndarray:
    """verify_batch with the challenge hashes computed on the device too (ecgpu_schnorr_verify_prehash_batch)."""
    if curve.id != K256:
        raise ValueError("BIP340 is defined over secp256k1")
    if any(len(m) != 32 for m in prehashes):
        raise ValueError("verify_prehash takes 32-byte digests")     # verifying.rs:68
    return curve.schnorr_verify_prehash(b"".join(pubkeys_x), b"".join(sigs), b"".join(prehashes))


def batch_verify_device(curve: Curve, pubkeys_x: Sequence[bytes], prehashes: Sequence[bytes], sigs: Sequence[bytes], seed: bytes | None = None,
                        flags: int = 0):
    """BIP340 batch verification (ecgpu_schnorr_batch_verify_prehash): one multi-scalar multiplication for the batch instead of two
    multiplications per signature -> (ok, all_valid), ok as verify_batch_device gives it.  seed=None lets the library draw the 32
    bytes the coefficients come from; a caller's seed must be unpredictable to whoever made the signatures."""
    if curve.id != K256:
        raise ValueError("BIP340 is defined over secp256k1")
    if any(len(m) != 32 for m in prehashes):
        raise ValueError("verify_prehash takes 32-byte digests")     # verifying.rs:68
    return curve.schnorr_batch_verify_prehash(b"".join(pubkeys_x), b"".join(sigs), b"".join(prehashes), seed=seed, flags=flags)


def sign_batch(curve: Curve, secret_keys: Sequence[bytes], prehashes: Sequence[bytes], aux_rands: Sequence[bytes]):
    """sign_prehash_with_aux_rand (signing.rs:80-131) for a batch -> (signatures, public keys x-only)."""
    if curve.id != K256:
        raise ValueError("BIP340 is defined over secp256k1")
    n = len(secret_keys)
    d0 = [int.from_bytes(k, "big") for k in secret_keys]
    if any(not (0 < d < N) for d in d0):
        raise ValueError("secret key out of range")
    P, _ = curve.mul_by_generator(b"".join(secret_keys))                       # device
    d = [(N - x) if (P[i][63] & 1) else x for i, x in enumerate(d0)]            # SigningKey::from: even-y key
    px = [bytes(P[i][:32]) for i in range(n)]
    ks = []
    for i in range(n):
        t = (d[i] ^ int.from_bytes(tagged_hash(b"BIP0340/aux", aux_rands[i]), "big")).to_bytes(32, "big")
        k0 = int.from_bytes(tagged_hash(b"BIP0340/nonce", t, px[i], prehashes[i]), "big") % N
        if k0 == 0:
            raise ValueError("zero nonce")
        ks.append(k0)
    R, _ = curve.mul_by_generator(b"".join(k.to_bytes(32, "big") for k in ks))  # device
    sigs = []
    for i in range(n):
        k = (N - ks[i]) if (R[i][63] & 1) else ks[i]
        r = bytes(R[i][:32])
        e = int.from_bytes(tagged_hash(b"BIP0340/challenge", r, px[i], prehashes[i]), "big") % N
        s = (k + e * d[i]) % N
        if s == 0:
            raise ValueError("zero s")
        sigs.append(r + s.to_bytes(32, "big"))
    return sigs, px


def sign_batch_device(curve: Curve, secret_keys: Sequence[bytes], prehashes: Sequence[bytes], aux_rands: Sequence[bytes]):
    """sign_batch with the tagged hashes and the arithmetic mod n on the device too (ecgpu_schnorr_sign_prehash_batch: one call,
    no round trip) -> (signatures, public keys x-only).  Like the reference, and unlike sign_batch, a nonce hash outside
    [1, n-1] is an error, not reduced (NonZeroScalar::try_from, signing.rs:105-108)."""
    if curve.id != K256:
        raise ValueError("BIP340 is defined over secp256k1")
    if any(len(m) != 32 for m in prehashes):
        raise ValueError("sign_prehash takes 32-byte digests")
    sig, px, ok = curve.schnorr_sign_prehash(b"".join(secret_keys), b"".join(prehashes), b"".join(aux_rands))
    if not ok.all():
        raise ValueError("signing failed for element %d (secret key out of range, or a zero nonce or s)" % int(np.argmin(ok)))
    return [bytes(r) for r in sig], [bytes(r) for r in px]


def sign_msg_batch_device(curve: Curve, secret_keys: Sequence[bytes], messages: Sequence[bytes], aux_rands: Sequence[bytes] | None = None):
    """Signer::try_sign (aux_rands=None: 32 zero bytes, signing.rs:214-218) / try_sign_with_rng for a batch of messages of any
    length: SHA256(msg) on the device, then as sign_batch_device (ecgpu_schnorr_sign_msg_batch) -> (signatures, public keys x-only).
    This is the reference's BIP340 over the digest of the message, not BIP340 with a variable-length message."""
    if curve.id != K256:
        raise ValueError("BIP340 is defined over secp256k1")
    sig, px, ok = curve.schnorr_sign_msg(b"".join(secret_keys), list(messages), None if aux_rands is None else b"".join(aux_rands))
    if not ok.all():
        raise ValueError("signing failed for element %d (secret key out of range, or a zero nonce or s)" % int(np.argmin(ok)))
    return [bytes(r) for r in sig], [bytes(r) for r in px]


def verify_msg_batch_device(curve: Curve, pubkeys_x: Sequence[bytes], messages: Sequence[bytes], sigs: Sequence[bytes]) -> np.ndarray:
    """Verifier::verify (verifying.rs:94-98) for a batch: verify_prehash over SHA256(msg), the digest computed on the device too
    (ecgpu_schnorr_verify_msg_batch)."""
    if curve.id != K256:
        raise ValueError("BIP340 is defined over secp256k1")
    return curve.schnorr_verify_msg(b"".join(pubkeys_x), list(messages), b"".join(sigs))
