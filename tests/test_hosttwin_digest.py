"""The plain digest on the host twin (csrc/h2c_hash.hpp digest_words over csrc/sha2.hpp update_aligned, compiled for the host by
tests/hosttwin/hosttwin_digest.cpp) against hashlib: every length 0 .. 300 at every record alignment 0 .. 15, the record embedded
in 0xA5 bytes, so that both the word path (whole blocks of a 4-byte aligned record) and the byte path (everything else) see every
block and padding boundary; one long message; and the incremental use where the word path follows a byte-path update."""
import ctypes
import hashlib
import random

import pytest

from hosttwin_util import lib, outbuf

HASHES = {0: ("sha256", 64), 1: ("sha384", 128)}
GUARD = 32


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
    out = outbuf(hashlib.new(HASHES[h][0]).digest_size)
    assert lib().ht_digest(h, raw, ctypes.c_size_t(off), ctypes.c_size_t(len(msg)), out) == 0
    # the surroundings are read-only for the digest
    assert bytes(raw[:off]) == b"\xa5" * off and bytes(raw[off + len(msg):]) == b"\xa5" * (len(raw) - off - len(msg))
    return bytes(out)


@pytest.mark.parametrize("h", [0, 1])
def test_every_length_at_every_alignment(h):
    name, bb = HASHES[h]
    rng = random.Random(0xD16E57 + h)
    words = 0
    for n in range(301):
        msg = rng.randbytes(n)
        want = hashlib.new(name, msg).digest()
        for align in range(16):
            assert _digest(h, msg, align) == want, (n, align)
            words += align % 4 == 0 and n >= bb
    assert words == 4 * (301 - bb)          # the word path ran for every whole block of the 4-byte aligned records


@pytest.mark.parametrize("h", [0, 1])
def test_the_public_condition_is_address_and_length(h):
    _, bb = HASHES[h]
    raw, off = _embedded(bytes(300), 0)
    for align in range(16):
        for n in (0, bb - 1, bb, 300):
            assert lib().ht_digest_takes_words(h, raw, ctypes.c_size_t(off + align), ctypes.c_size_t(n)) == int(align % 4 == 0 and n >= bb)


@pytest.mark.parametrize("h", [0, 1])
@pytest.mark.parametrize("align", [0, 4, 1, 2, 3])
def test_ten_thousand_bytes(h, align):
    msg = random.Random(0x10000 + h).randbytes(10000)
    assert _digest(h, msg, align) == hashlib.new(HASHES[h][0], msg).digest()


@pytest.mark.parametrize("h", [0, 1])
def test_extreme_bytes(h):
    name, bb = HASHES[h]
    for n in (bb - 9, bb - 8, bb, 2 * bb, 2 * bb + 1, 300):
        for fill in (b"\x00", b"\xff", b"\x80"):
            assert _digest(h, fill * n, 0) == hashlib.new(name, fill * n).digest(), (n, fill)


@pytest.mark.parametrize("h", [0, 1])
def test_word_path_behind_a_byte_path_update(h):
    """update (bytes) takes the first `split` bytes, update_aligned the rest.  Where the byte path left the block part-filled the
    rest stays on the byte path; where it ended on a block boundary and the rest starts 4-byte aligned, the word path takes over
    from a state the byte path built; a rest that starts unaligned stays on the byte path whatever the fill."""
    name, bb = HASHES[h]
    rng = random.Random(0x5B11 + h)
    out = outbuf(hashlib.new(name).digest_size)
    for total in (3 * bb + 17, 4 * bb, 300):
        msg = rng.randbytes(total)
        want = hashlib.new(name, msg).digest()
        for align in (0, 1, 2, 3, 4):
            raw, off = _embedded(msg, align)
            for split in list(range(0, 2 * bb + 2)) + [total - 1, total]:
                assert lib().ht_digest_split(h, raw, ctypes.c_size_t(off), ctypes.c_size_t(total), ctypes.c_size_t(split), out) == 0
                assert bytes(out) == want, (total, align, split)
