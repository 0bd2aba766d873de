"""The sponge digests on the host twin (csrc/keccak.hpp digest_words over update_aligned, compiled for the host by
tests/hosttwin/hosttwin_keccak.cpp) against hashlib (SHA3-256, SHA3-384) and tests/keccak_model.py (Keccak-256): every length
0 .. 300 at every record alignment 0 .. 15, the record embedded in 0xA5 bytes, so that both the word path (whole blocks of a 4-byte
aligned record) and the byte path (everything else) see every block and padding boundary - 134/135/136/137 and 271/272/273 for the
rate 136, 102/103/104/105 and 207/208/209 for the rate 104, among them the lengths rate - 1 mod rate where the domain byte and the
final 0x80 share a byte; extreme fills; one long message; and the incremental use where the word path follows a byte-path update."""
import ctypes
import hashlib
import random

import pytest

import keccak_model as K
from hosttwin_util import lib, outbuf

HASHES = {16: ("keccak256", 136, 32), 17: ("sha3_256", 136, 32), 18: ("sha3_384", 104, 48)}
GUARD = 32


def _want(h, msg):
    return K.digest(h, msg) if h == 16 else hashlib.new(HASHES[h][0], msg).digest()


def _embedded(msg: bytes, align: int):
    """a buffer of 0xA5 bytes with msg inside it at an address that is `align` mod 16 -> (buffer, offset)"""
    raw = (ctypes.c_uint8 * (len(msg) + 2 * GUARD + 16))()
    ctypes.memset(raw, 0xA5, len(raw))
    off = GUARD + (align - (ctypes.addressof(raw) + GUARD)) % 16
    ctypes.memmove(ctypes.addressof(raw) + off, msg, len(msg))
    assert (ctypes.addressof(raw) + off) % 16 == align
    return raw, off


def _digest(h, msg, align):
    raw, off = _embedded(msg, align)
    out = outbuf(HASHES[h][2])
    assert lib().ht_keccak(h, raw, ctypes.c_size_t(off), ctypes.c_size_t(len(msg)), out) == 0
    # the surroundings are read-only for the digest
    assert bytes(raw[:off]) == b"\xa5" * off and bytes(raw[off + len(msg):]) == b"\xa5" * (len(raw) - off - len(msg))
    return bytes(out)


@pytest.mark.parametrize("h", [16, 17, 18])
def test_every_length_at_every_alignment(h):
    _, rate, _ = HASHES[h]
    rng = random.Random(0xCECC + h)
    words = 0
    for n in range(301):
        msg = rng.randbytes(n)
        want = _want(h, msg)
        for align in range(16):
            assert _digest(h, msg, align) == want, (n, align)
            raw, off = _embedded(msg, align)
            words += lib().ht_keccak_takes_words(h, raw, ctypes.c_size_t(off), ctypes.c_size_t(n))
    assert words == 4 * (301 - rate)        # the word path ran for every whole block of the 4-byte aligned records


@pytest.mark.parametrize("h", [16, 17, 18])
def test_the_public_condition_is_address_and_length(h):
    _, rate, _ = HASHES[h]
    raw, off = _embedded(bytes(300), 0)
    for align in range(16):
        for n in (0, rate - 1, rate, 300):
            assert lib().ht_keccak_takes_words(h, raw, ctypes.c_size_t(off + align), ctypes.c_size_t(n)) == int(align % 4 == 0 and n >= rate)
    assert lib().ht_keccak_takes_words(2, raw, ctypes.c_size_t(off), ctypes.c_size_t(300)) == -1
    assert lib().ht_keccak(2, raw, ctypes.c_size_t(off), ctypes.c_size_t(0), outbuf(48)) == -1


@pytest.mark.parametrize("h", [16, 17, 18])
def test_extreme_bytes(h):
    _, rate, _ = HASHES[h]
    for n in (rate - 1, rate, 2 * rate, 2 * rate + 1):
        for fill in (b"\x00", b"\xff", b"\x80"):
            want = _want(h, fill * n)
            for align in (0, 1):
                assert _digest(h, fill * n, align) == want, (n, fill, align)


@pytest.mark.parametrize("h", [16, 17, 18])
def test_word_path_behind_a_byte_path_update(h):
    """update (bytes) takes the first `split` bytes, update_aligned the rest.  Where the byte path left the block part-filled the
    rest stays on the byte path; where it ended on a block boundary and the rest starts 4-byte aligned, the word path takes over
    from a state the byte path built; a rest that starts unaligned stays on the byte path whatever the fill."""
    _, rate, db = HASHES[h]
    rng = random.Random(0x5B11 + h)
    out = outbuf(db)
    for total in (3 * rate + 17, 4 * rate):
        msg = rng.randbytes(total)
        want = _want(h, msg)
        for align in (0, 1, 2, 3, 4):
            raw, off = _embedded(msg, align)
            for split in list(range(0, 2 * rate + 2)) + [total - 1, total]:
                assert lib().ht_keccak_split(h, raw, ctypes.c_size_t(off), ctypes.c_size_t(total), ctypes.c_size_t(split), out) == 0
                assert bytes(out) == want, (total, align, split)
    assert lib().ht_keccak_split(h, raw, ctypes.c_size_t(off), ctypes.c_size_t(4), ctypes.c_size_t(5), out) == -1


@pytest.mark.parametrize("h", [16, 17, 18])
@pytest.mark.parametrize("align", [0, 4, 1, 2, 3])
def test_ten_thousand_bytes(h, align):
    msg = random.Random(0x10000 + h).randbytes(10000)
    if h == 16:
        want = _TEN_THOUSAND.setdefault("d", K.keccak256(msg))      # 74 blocks of the model, once
    else:
        want = hashlib.new(HASHES[h][0], msg).digest()
    assert _digest(h, msg, align) == want


_TEN_THOUSAND = {}
