"""The workspace carver (csrc/ws_carver.hpp: the arithmetic every multi-kernel launcher lays its device workspace out with), host
build (tests/hosttwin/hosttwin_carver.cpp): one layout of mixed sizes through the sizing pass and the pointer pass."""
import ctypes

import numpy as np
import pytest

from hosttwin_util import lib

ALIGN = 256
# every size around the alignment, a multi-megabyte one, and one past 2^32 (a 32-bit byte count would truncate it to 0)
SIZES = [0, 1, 255, 256, 257, 0, (5 << 20) + 3, 3 << 32, 0, 7]


def carve(base, sizes):
    s = np.array(sizes, dtype=np.uint64)
    size_ptrs = np.full(len(sizes), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    ptrs = np.full(len(sizes), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    totals = np.zeros(2, dtype=np.uint64)
    f = lib().ht_carve
    f.restype = None
    f.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    f(base, s.ctypes.data, len(sizes), size_ptrs.ctypes.data, ptrs.ctypes.data, totals.ctypes.data)
    return [int(x) for x in size_ptrs], [int(x) for x in ptrs], int(totals[0]), int(totals[1])


def rounded(b):
    return (b + ALIGN - 1) // ALIGN * ALIGN


@pytest.mark.parametrize("base", [1 << 40, (0x7F12 << 32) + 5 * ALIGN])
@pytest.mark.parametrize("sizes", [SIZES, SIZES[::-1], [3 << 32, 3 << 32], [0], [1]])
def test_two_passes_agree(base, sizes):
    size_ptrs, ptrs, size_total, end = carve(base, sizes)
    # the sizing pass hands out null pointers only (never null + offset)
    assert size_ptrs == [0] * len(sizes)
    # its total is the end offset of the pointer pass, and every byte count is kept in full
    assert size_total == end == sum(rounded(b) for b in sizes)
    # aligned relative to the base, in declaration order, disjoint; a zero-byte sub-buffer occupies nothing
    at = base
    for b, p in zip(sizes, ptrs):
        assert (p - base) % ALIGN == 0
        assert p == at
        at = p + rounded(b)
        assert at >= p + b and (b != 0 or at == p)
    assert at == base + end


def test_large_size_is_not_truncated():
    _, ptrs, total, _ = carve(1 << 40, [3 << 32, 1])
    assert ptrs[1] - ptrs[0] == 3 << 32 and total == (3 << 32) + ALIGN
