"""Batched ECDSA verification of DER-encoded signatures over messages: the shape of the reference's
`VerifyingKey::verify(msg, &Signature::from_der(..)?)` call (k256/src/ecdsa.rs:366-387), for a batch.

Host side: DER decoding (der.py), hashing (the curve's DigestPrimitive: SHA-256 for k256 / p256, SHA-384 for
p384 - k256/src/ecdsa.rs:177-180, p256/src/ecdsa.rs:66-69, p384/src/ecdsa.rs:63-66) and bits2field.  Device
side: `Curve.ecdsa_verify` (ecgpu_ecdsa_verify_batch).  No CPU verification path exists here."""
from __future__ import annotations

import hashlib
from typing import Sequence

import numpy as np

from . import K256, P256, P384, Curve
from .der import decode_signature

DIGEST = {K256: hashlib.sha256, P256: hashlib.sha256, P384: hashlib.sha384}


def bits2field(nb: int, digest: bytes) -> bytes:
    if len(digest) < nb // 2:
        raise ValueError("digest too short")
    return digest[:nb] if len(digest) >= nb else bytes(nb - len(digest)) + digest


def verify_der_batch(curve: Curve, pubkeys_xy: Sequence[bytes], messages: Sequence[bytes], der_sigs: Sequence[bytes],
                     normalize_s: bool = False) -> np.ndarray:
    """ok[i] = 1 iff der_sigs[i] decodes and verifies over messages[i] under pubkeys_xy[i] (affine x || y).
    normalize_s=True first maps s to the low half, as the k256 Wycheproof runner does (k256/src/ecdsa.rs:377)."""
    nb = curve.nb
    n = len(der_sigs)
    order = ORDER[curve.id]
    z = bytearray(n * nb)
    sig = bytearray(n * 2 * nb)
    decoded = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        rs = decode_signature(der_sigs[i], nb)
        if rs is None:
            continue                       # Signature::from_der -> Err
        r, s = rs
        if normalize_s and s > order // 2 and s < order:
            s = order - s
        decoded[i] = 1
        sig[2 * nb * i:2 * nb * (i + 1)] = r.to_bytes(nb, "big") + s.to_bytes(nb, "big")
        z[nb * i:nb * (i + 1)] = bits2field(nb, DIGEST[curve.id](messages[i]).digest())
    ok = curve.ecdsa_verify(bytes(z), bytes(sig), b"".join(pubkeys_xy))
    return ok & decoded


def sign_prehash(curve: Curve, secret_keys: Sequence[bytes], digests: Sequence[bytes], extra: Sequence[bytes] | None = None, flags=None):
    """PrehashSigner::sign_prehash for a batch of digests of any admissible length: bits2field on the host, then
    `Curve.ecdsa_sign_prehash` (ecgpu_ecdsa_sign_prehash_batch: RFC 6979 nonces and signatures on the device)
    -> (sig_rs, recovery_id, ok).  `extra`: per-signature additional data of field size (RandomizedPrehashSigner)."""
    z = b"".join(bits2field(curve.nb, bytes(h)) for h in digests)
    return curve.ecdsa_sign_prehash(b"".join(secret_keys), z, None if extra is None else b"".join(extra), flags)


def verify_der_batch_device(curve: Curve, pubkeys_xy: Sequence[bytes], messages: Sequence[bytes], der_sigs: Sequence[bytes],
                            normalize_s: bool = False) -> np.ndarray:
    """verify_der_batch with the messages hashed on the device (ecgpu_ecdsa_verify_msg_batch: Verifier::verify): DER decoding stays
    on the host, the digests never exist there.  A signature that does not decode keeps a zero r || s, which never verifies."""
    nb = curve.nb
    n = len(der_sigs)
    order = ORDER[curve.id]
    sig = bytearray(n * 2 * nb)
    decoded = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        rs = decode_signature(der_sigs[i], nb)
        if rs is None:
            continue                       # Signature::from_der -> Err
        r, s = rs
        if normalize_s and s > order // 2 and s < order:
            s = order - s
        decoded[i] = 1
        sig[2 * nb * i:2 * nb * (i + 1)] = r.to_bytes(nb, "big") + s.to_bytes(nb, "big")
    ok = curve.ecdsa_verify_msg(list(messages), bytes(sig), b"".join(pubkeys_xy))
    return ok & decoded


def sign_msg(curve: Curve, secret_keys: Sequence[bytes], messages: Sequence[bytes], extra: Sequence[bytes] | None = None, flags=None):
    """Signer::sign (extra=None) / RandomizedSigner::sign_with_rng for a batch of messages: the curve's own digest, the RFC 6979
    nonces and the signatures all on the device (ecgpu_ecdsa_sign_msg_batch) -> (sig_rs, recovery_id, ok)"""
    return curve.ecdsa_sign_msg(b"".join(secret_keys), list(messages), None if extra is None else b"".join(extra), flags)


def verify_msg(curve: Curve, pubkeys_xy: Sequence[bytes], messages: Sequence[bytes], sigs_rs: Sequence[bytes], flags=None) -> np.ndarray:
    """Verifier::verify for a batch of fixed-width r || s signatures (ecgpu_ecdsa_verify_msg_batch)"""
    return curve.ecdsa_verify_msg(list(messages), b"".join(sigs_rs), b"".join(pubkeys_xy), flags)


def recover_from_msg(curve: Curve, messages: Sequence[bytes], sigs_rs: Sequence[bytes], recovery_ids: Sequence[int], flags=None):
    """VerifyingKey::recover_from_msg for a batch (ecgpu_ecdsa_recover_msg_batch) -> (pubkeys_xy, ok)"""
    return curve.ecdsa_recover_msg(list(messages), b"".join(sigs_rs), np.array(list(recovery_ids), dtype=np.uint8), flags)


def sign_digest(curve: Curve, hash_id: int, secret_keys: Sequence[bytes], messages: Sequence[bytes], extra: Sequence[bytes] | None = None, flags=None):
    """DigestSigner::sign_digest / sign_digest_recoverable (extra=None) / RandomizedDigestSigner for a batch of messages hashed with
    hash_id (ecgpu.KECCAK256: Keccak256::new_with_prefix(msg), the reference's Ethereum example) on the device
    (ecgpu_ecdsa_sign_digest_batch) -> (sig_rs, recovery_id, ok).  The digest must be of the curve's field size."""
    return curve.ecdsa_sign_digest(hash_id, b"".join(secret_keys), list(messages), None if extra is None else b"".join(extra), flags)


def verify_digest(curve: Curve, hash_id: int, pubkeys_xy: Sequence[bytes], messages: Sequence[bytes], sigs_rs: Sequence[bytes], flags=None) -> np.ndarray:
    """DigestVerifier::verify_digest for a batch of fixed-width r || s signatures (ecgpu_ecdsa_verify_digest_batch)"""
    return curve.ecdsa_verify_digest(hash_id, list(messages), b"".join(sigs_rs), b"".join(pubkeys_xy), flags)


def recover_digest(curve: Curve, hash_id: int, messages: Sequence[bytes], sigs_rs: Sequence[bytes], recovery_ids: Sequence[int], flags=None):
    """VerifyingKey::recover_from_digest for a batch (ecgpu_ecdsa_recover_digest_batch) -> (pubkeys_xy, ok)"""
    return curve.ecdsa_recover_digest(hash_id, list(messages), b"".join(sigs_rs), np.array(list(recovery_ids), dtype=np.uint8), flags)


def eth_addresses(ctx, pubkeys_xy) -> np.ndarray:
    """Ethereum addresses of secp256k1 public keys: the last 20 bytes of Keccak-256 over each 64-byte x || y (what a caller of
    recovery wants) -> (n, 20).  It is ecgpu_digest_batch on the records as they lie, 64 bytes apart, and a slice."""
    from . import HOST, KECCAK256, _as_host, _call, _host_out
    q = _as_host(pubkeys_xy, 64)
    out = _host_out(len(q), 32)
    _call(ctx, "ecgpu_digest_batch", KECCAK256, q, 64, None, out, len(q), HOST)
    return np.ascontiguousarray(out[:, 12:])


ORDER = {
    K256: 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
    P256: 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551,
    P384: 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973,
}
