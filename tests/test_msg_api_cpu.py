"""What the message-level calls (include/ecgpu.h, "from message bytes") check without a device: the six symbols are exported and
declared, a call without a context is refused before anything else, the Python wrappers refuse batches of unequal length, and the
record packing pads the stride to a multiple of 16 while pack_messages keeps its behaviour."""
import ctypes
import os

import numpy as np
import pytest

import ecgpu

NEW = ("ecgpu_digest_batch", "ecgpu_ecdsa_sign_msg_batch", "ecgpu_ecdsa_verify_msg_batch", "ecgpu_ecdsa_recover_msg_batch",
       "ecgpu_schnorr_sign_msg_batch", "ecgpu_schnorr_verify_msg_batch")
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(ecgpu.LIB_PATH):
        pytest.skip("libecgpu.so not built")
    return ecgpu.load_library()


def test_symbols_exported_and_declared(lib):
    for name in NEW:
        assert name in ecgpu.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None


def test_null_context_is_refused(lib):
    z = np.zeros(256, dtype=np.uint8)
    p = ctypes.c_void_p(z.ctypes.data)
    assert lib.ecgpu_digest_batch(None, 0, p, 16, None, p, 2, 0) == ERR_ARG
    assert lib.ecgpu_ecdsa_sign_msg_batch(None, 0, p, p, 16, None, None, p, None, p, 2, 0, 0) == ERR_ARG
    assert lib.ecgpu_ecdsa_verify_msg_batch(None, 0, p, 16, None, p, p, p, 2, 0, 0) == ERR_ARG
    assert lib.ecgpu_ecdsa_recover_msg_batch(None, 0, p, 16, None, p, p, p, p, 2, 0, 0) == ERR_ARG
    assert lib.ecgpu_schnorr_sign_msg_batch(None, 0, p, p, 16, None, None, p, None, p, 2, 0) == ERR_ARG
    assert lib.ecgpu_schnorr_verify_msg_batch(None, 0, p, p, 16, None, p, p, 2, 0) == ERR_ARG
    assert not z.any()


def test_aligned_packing():
    msgs = [b"", b"abc", bytes(range(33))]
    rec, lens, stride = ecgpu.pack_messages_aligned(msgs)
    assert stride == 48 and rec.shape == (3, 48) and list(lens) == [0, 3, 33]
    assert bytes(rec[1, :3]) == b"abc" and bytes(rec[2, :33]) == bytes(range(33)) and not rec[2, 33:].any()
    for longest, want in ((0, 0), (1, 16), (16, 16), (17, 32), (200, 208)):
        assert ecgpu.pack_messages_aligned([bytes(longest)])[2] == want
    assert ecgpu.pack_messages_aligned([])[0].shape == (0, 0)
    # pack_messages itself: the stride is the longest message unless the caller names one
    assert ecgpu.pack_messages(msgs)[2] == 33 and ecgpu.pack_messages(msgs, 40)[2] == 40
    with pytest.raises(ValueError):
        ecgpu.pack_messages(msgs, 32)


@pytest.mark.parametrize("cid", [ecgpu.K256, ecgpu.P384])
def test_wrappers_refuse_unequal_batches(cid):
    """the length checks come before any call into the library: a curve without a context reaches them"""
    cv = ecgpu.Curve(None, cid)
    nb = cv.nb
    two = [b"a", b"bc"]
    with pytest.raises(ValueError):
        cv.ecdsa_sign_msg(bytes(3 * nb), two)
    with pytest.raises(ValueError):
        cv.ecdsa_sign_msg(bytes(2 * nb), two, extra=bytes(nb))
    with pytest.raises(ValueError):
        cv.ecdsa_verify_msg(two, bytes(2 * 2 * nb), bytes(3 * 2 * nb))
    with pytest.raises(ValueError):
        cv.ecdsa_recover_msg(two, bytes(2 * 2 * nb), [0])
    with pytest.raises(ValueError):
        cv.schnorr_sign_msg(bytes(2 * nb), two, aux_rands=bytes(32))
    with pytest.raises(ValueError):
        cv.schnorr_verify_msg(bytes(nb), two, bytes(2 * 2 * nb))


def test_schnorr_helpers_are_secp256k1_only():
    from ecgpu import schnorr as S
    cv = ecgpu.Curve(None, ecgpu.P256)
    with pytest.raises(ValueError, match="secp256k1"):
        S.sign_msg_batch_device(cv, [bytes(32)], [b"m"])
    with pytest.raises(ValueError, match="secp256k1"):
        S.verify_msg_batch_device(cv, [bytes(32)], [b"m"], [bytes(64)])
