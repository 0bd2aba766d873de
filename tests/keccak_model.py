"""The Keccak-f[1600] sponge in plain Python with the (rate, domain byte, digest bytes) parameters of csrc/keccak.hpp: the expectation
of the host-twin and device tests for Keccak-256, which hashlib does not have.  tests/test_keccak_model.py pins it first, against
hashlib's SHA-3 on every length 0 .. 300 and against known Keccak-256 answers.  One permutation costs about half a millisecond:
keep an expectation to a few hundred blocks."""

MASK = (1 << 64) - 1
KECCAK256, SHA3_256, SHA3_384 = 16, 17, 18                       # ecgpu_hash
PARAMS = {KECCAK256: (136, 0x01, 32), SHA3_256: (136, 0x06, 32), SHA3_384: (104, 0x06, 48)}


def _round_constants():
    """iota's constants from the degree-8 LFSR of FIPS 202, algorithm 5"""
    out, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            if r & 1:
                rc |= 1 << ((1 << j) - 1)
            r <<= 1
            if r & 0x100:
                r ^= 0x171
        out.append(rc)
    return out


def _rho_offsets():
    rho, x, y = [0] * 25, 1, 0
    for t in range(24):
        rho[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rho


RC = _round_constants()
RHO = _rho_offsets()


def _rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def permute(a):
    """Keccak-f[1600] on 25 lanes a[x + 5 y], in place"""
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        for x in range(5):
            d = c[(x + 4) % 5] ^ _rotl(c[(x + 1) % 5], 1)
            for y in range(0, 25, 5):
                a[x + y] ^= d
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rotl(a[x + 5 * y], RHO[x + 5 * y])
        for y in range(0, 25, 5):
            for x in range(5):
                a[x + y] = b[x + y] ^ (~b[(x + 1) % 5 + y] & MASK & b[(x + 2) % 5 + y])
        a[0] ^= rc


def sponge(rate: int, domain: int, digest_bytes: int, msg: bytes) -> bytes:
    pad = bytearray(rate - len(msg) % rate)
    pad[0] ^= domain
    pad[-1] ^= 0x80
    data = bytes(msg) + bytes(pad)
    a = [0] * 25
    for off in range(0, len(data), rate):
        for j in range(rate // 8):
            a[j] ^= int.from_bytes(data[off + 8 * j:off + 8 * j + 8], "little")
        permute(a)
    return b"".join(v.to_bytes(8, "little") for v in a)[:digest_bytes]


def digest(hash_id: int, msg: bytes) -> bytes:
    return sponge(*PARAMS[hash_id], msg)


def keccak256(msg: bytes) -> bytes:
    return sponge(136, 0x01, 32, msg)


def eth_address(pubkey_xy: bytes) -> bytes:
    """the last 20 bytes of Keccak-256 over the 64-byte x || y"""
    assert len(pubkey_xy) == 64
    return keccak256(pubkey_xy)[12:]
