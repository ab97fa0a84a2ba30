"""CPU: verdict_cases.wide_digest, the expected value of every wide-length GPU
test, checked two independent ways -- against hashlib for ordinary messages,
and against the reference's own sha.c (oracle/_ref/libref_sha1.so) continued
from a context whose totalLength and hash were set by hand, for every (prefix,
tail) pair the GPU tests use.  A helper that is wrong about the high word of
the bit count would make those tests pin the wrong digests.
"""
import ctypes
import hashlib
import os
import struct

import pytest

import verdict_cases as vc


class RefContext(ctypes.Structure):  # sha.h:39-50
    _fields_ = [("totalLength", ctypes.c_uint64), ("hash", ctypes.c_uint32 * 5),
                ("bufferLength", ctypes.c_uint32), ("buffer", ctypes.c_uint8 * 64)]


def load_ref_sha(oracle):
    if not os.path.exists(oracle.REF_SO):
        return None
    ref = ctypes.CDLL(oracle.REF_SO)
    ref.SHA1Init.argtypes = [ctypes.POINTER(RefContext)]
    ref.SHA1Update.argtypes = [ctypes.POINTER(RefContext), ctypes.c_void_p, ctypes.c_uint32]
    ref.SHA1Final.argtypes = [ctypes.POINTER(RefContext), ctypes.c_void_p]
    return ref


def ref_continue(ref, state, prefix, tail):
    """sha.c from a context that has seen `prefix` bytes and holds `state`:
    SHA1Update(tail), SHA1Final.  (digest, totalLength before SHA1Final)."""
    ctx = RefContext()
    ref.SHA1Init(ctypes.byref(ctx))
    ctx.totalLength = 8 * prefix
    for k in range(5):
        ctx.hash[k] = state[k]
    buf = (ctypes.c_uint8 * max(1, len(tail))).from_buffer_copy(tail or b"\0")
    ref.SHA1Update(ctypes.byref(ctx), buf, len(tail))
    bits = ctx.totalLength
    out = (ctypes.c_uint8 * 20)()
    ref.SHA1Final(ctypes.byref(ctx), out)
    return bytes(out), bits


def test_pad_blocks_layout():
    for n in range(0, 131):
        blk = vc.pad_blocks(bytes(n), 2**40 + n)
        assert len(blk) == 64 * (n // 64 + (2 if n % 64 >= 56 else 1)), n
        assert blk[n] == 0x80 and not any(blk[n + 1:-8]), n
        assert struct.unpack(">II", blk[-8:]) == ((8 * (2**40 + n)) >> 32, (8 * (2**40 + n)) & 0xFFFFFFFF), n


def test_wide_digest_equals_hashlib_without_a_prefix(oracle):
    for n in range(0, 131):
        msg = bytes(oracle.fill_synthetic(n, n, 0xAD))
        assert vc.wide_digest(oracle, vc.IV, 0, msg) == hashlib.sha1(msg).digest(), n
    # a materialised prefix: the state after it, then the tail alone
    msg = bytes(oracle.fill_synthetic(64 * 5 + 77, 3, 0xAD))
    mid = oracle.compress_blocks(vc.IV, msg[:256])
    assert vc.wide_digest(oracle, mid, 256, msg[256:]) == hashlib.sha1(msg).digest()


def test_wide_digest_equals_the_reference_continued_from_a_set_context(oracle):
    ref = load_ref_sha(oracle)
    if ref is None:
        pytest.skip("oracle/_ref not built (reference absent)")
    cases = vc.grid_cases(oracle)
    assert len(cases) == 64 and {p for p, _, _ in cases} == set(vc.PREFIXES)
    counts = set()
    for p, tail, state in cases:
        got, bits = ref_continue(ref, state, p, tail)
        assert bits == 8 * (p + len(tail)) % 2**64  # uint64_t totalLength, sha.h:40
        counts.add(bits)
        assert vc.wide_digest(oracle, state, p, tail) == got, (p, len(tail))
    # the grid holds what it is meant to hold: a count of exactly 2^32, the one
    # just below it, and one whose high word is all ones
    assert 2**32 in counts and 2**32 - 8 in counts and max(counts) >> 32 == 0xFFFFFFFF
    # the column tests' pairs: the tail is a whole column, msg_len = P + width
    rng_state = cases[0][2]
    for msg_len in vc.COLUMN_MSG_LENS:
        for width in vc.COLUMN_WIDTHS:
            col = bytes(oracle.fill_synthetic(width, width, 0xC0))
            got, bits = ref_continue(ref, rng_state, msg_len - width, col)
            assert bits == 8 * msg_len
            assert vc.wide_digest(oracle, rng_state, msg_len - width, col) == got, (msg_len, width)
    # the streaming test's pairs: 129 bytes after P
    for p in vc.STREAM_PREFIXES:
        tail = bytes(oracle.fill_synthetic(129, 9, 0xC0))
        assert vc.wide_digest(oracle, rng_state, p, tail) == ref_continue(ref, rng_state, p, tail)[0], p
