"""RFC 6979 section 3.2 (deterministic nonces, HMAC-DRBG) on hmac / hashlib: the expectation of the device and host-twin
tests.  tests/test_hosttwin_signing.py pins it first: with oracle.ecmodel.ecdsa_sign_prehashed it reproduces the six signatures of
tests/golden/rfc6979_sign.json."""
import hashlib
import hmac

CURVE_HASH = {"k256": "sha256", "p256": "sha256", "p384": "sha384"}


def generate_k(q: int, hash_name: str, x: bytes, h1: bytes, extra: bytes = b""):
    """steps b to h -> (k, rejections).  x: the key, h1: bits2octets of the digest, both of the hash's length (hlen = qlen on
    the three curves, so bits2int of a candidate is the candidate); extra: the additional data k' of section 3.6, or empty."""
    hlen = hashlib.new(hash_name).digest_size
    assert len(x) == hlen and len(h1) == hlen and len(extra) in (0, hlen)

    def mac(key, msg):
        return hmac.new(key, msg, hash_name).digest()

    K, V = bytes(hlen), b"\x01" * hlen
    for sep in (b"\x00", b"\x01"):
        K = mac(K, V + sep + x + h1 + extra)
        V = mac(K, V)
    rejections = 0
    while True:
        V = mac(K, V)
        k = int.from_bytes(V, "big")
        if 0 < k < q:
            return k, rejections
        rejections += 1
        K = mac(K, V + b"\x00")
        V = mac(K, V)


def nonce(c, d: int, z: bytes, extra: bytes = b""):
    """the nonce of SigningKey::sign_prehash on curve c (oracle.ecmodel.Curve) for the field-sized prehash z; 0 for a key outside
    [1, n - 1] (the batched call's convention)"""
    if not 0 < d < c.n:
        return 0
    h1 = (int.from_bytes(z, "big") % c.n).to_bytes(c.nbytes, "big")
    return generate_k(c.n, CURVE_HASH[c.name], d.to_bytes(c.nbytes, "big"), h1, extra)[0]
