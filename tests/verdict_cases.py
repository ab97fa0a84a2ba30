"""Shared by tests/test_gpu_verdict_bits.py, tests/test_gpu_wide_lengths.py and
tests/test_padding_reference.py.

1. The verdict batch.  A fused compare answers "these 20 bytes equal those 20
   bytes"; a compare that skips a byte, drops a mask or shifts wrongly answers
   yes where one bit differs.  The batch has N = 168 messages: expectation i
   < 160 is the true digest with bit i flipped (byte i // 8, mask 1 << i % 8),
   so each of the 160 bit positions is the only difference exactly once;
   messages 160 .. 167 carry exact expectations.  A launch of n >= N messages
   plants the batch on its last N (the partly filled last workgroup); every
   earlier expectation is exact.  problems() names the bits whose flip was
   accepted, not just how many verdicts differ.

2. Digests of messages that are never materialised.  SHA-1 resumes at every
   64-byte boundary, so the digest of (P bytes already compressed into state
   S) + tail t depends on P only through the 64-bit bit count of the padding
   (sha.c:536-543): wide_digest() = compress_blocks(S, t | 0x80 | zeros |
   be64(8 * (P + len t))).  With P >= 2^29 the high word of that count is not
   zero, which no message the suite can afford to hash reaches.
"""
import random
import struct

import numpy as np

N = 168  # messages of the verdict batch
NBITS = 160  # bits of a digest: message i < NBITS has bit i of its expectation flipped
IV = (0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0)


# ---------------------------------------------------------------------------
# 1. The verdict batch
# ---------------------------------------------------------------------------
def expectations(digests, exact=False):
    """Expectations for the n = len(digests) / 20 messages of a launch, as a
    (n, 20) uint8 array: the true digests, and unless `exact` the verdict batch
    planted on the last N of them."""
    exp = np.frombuffer(bytes(digests), dtype=np.uint8).reshape(-1, 20).copy()
    n = exp.shape[0]
    assert n >= N
    if not exact:
        for i in range(NBITS):
            exp[n - N + i, i // 8] ^= 1 << (i % 8)
    return exp


def want_ok(n, exact=False):
    ok = np.ones(n, dtype=np.uint8)
    if not exact:
        ok[n - N:n - N + NBITS] = 0
    return ok


def ranges(idx):
    """Sorted integers as text: [0, 1, 2, 7, 9, 10] -> '0-2, 7, 9-10'."""
    out, idx = [], sorted(idx)
    i = 0
    while i < len(idx):
        j = i
        while j + 1 < len(idx) and idx[j + 1] == idx[j] + 1:
            j += 1
        out.append(str(idx[i]) if i == j else f"{idx[i]}-{idx[j]}")
        i = j + 1
    return ", ".join(out)


def problems(got_ok, exact=False):
    """What differs from want_ok in the n verdicts `got_ok` (any sequence of
    0 / 1 / bool): the flipped bits that were accepted, by bit index, and the
    messages with an exact expectation that were rejected (or hold neither 0
    nor 1)."""
    got = np.asarray([int(x) for x in got_ok], dtype=np.int64)
    n = got.size
    want = want_ok(n, exact)
    bad = []
    if not exact:
        accepted = [i for i in range(NBITS) if got[n - N + i] != 0]
        if accepted:
            bad.append(f"{len(accepted)} one-bit differences not rejected: digest bits {ranges(accepted)} "
                       f"(bytes {ranges({i // 8 for i in accepted})})")
    rejected = [int(i) for i in np.nonzero((want == 1) & (got != 1))[0]]
    if rejected:
        bad.append(f"{len(rejected)} exact expectations not accepted, messages {rejected[:20]} of {n}: "
                   f"ok = {[int(got[i]) for i in rejected[:20]]}")
    return bad


def digest_problems(got, want, what="digests"):
    """got, want: n x 20 bytes.  The entries that differ, by index."""
    g = np.frombuffer(bytes(got), dtype=np.uint8).reshape(-1, 20)
    w = np.frombuffer(bytes(want), dtype=np.uint8).reshape(-1, 20)
    if g.shape != w.shape:
        return [f"{what}: {g.shape[0]} entries for {w.shape[0]}"]
    wrong = [int(i) for i in np.nonzero((g != w).any(axis=1))[0]]
    return [f"{what}: {len(wrong)} of {w.shape[0]} differ, entries {wrong[:20]}"] if wrong else []


# ---------------------------------------------------------------------------
# 2. Wide lengths
# ---------------------------------------------------------------------------
def pad_blocks(tail, total_bytes):
    """tail | 0x80 | zeros to 56 mod 64 | be64(8 * total_bytes): sha.c:536-543
    for a message of total_bytes whose last len(tail) bytes are `tail`.  The
    count is sha.c's uint64_t totalLength, so it wraps at 2^64 (one pair of
    GRID does: 2^61 - 128 + 129 bytes are 8 bits mod 2^64)."""
    tail = bytes(tail)
    bits = (8 * total_bytes) % (1 << 64)
    zeros = (55 - len(tail)) % 64
    out = tail + b"\x80" + bytes(zeros) + struct.pack(">Q", bits)
    assert len(out) % 64 == 0
    return out


def wide_digest(orc, state, prefix, tail):
    """Digest of a message whose first `prefix` bytes (a multiple of 64, never
    materialised) left the chaining state `state`, and whose last bytes are `tail`."""
    assert prefix % 64 == 0
    h = orc.compress_blocks(state, pad_blocks(tail, prefix + len(tail)))
    return struct.pack(">5I", *h)


# Bit counts of exactly 2^32 (P = 2^29 - 64 with the 64-byte tail: low word 0, high word 1), of
# 2^32 - 8 (the same P with the 63-byte tail: high word still 0), high words of 1, 7, 8, 9, 2^11
# and, at P = 2^61 - 128, 2^32 - 1 (counts just below 2^64; with the 129-byte tail the count wraps to 8).
PREFIXES = (2**29 - 64, 2**29, 2**29 + 64, 2**32 - 64, 2**32, 2**33 + 2**29, 2**40, 2**61 - 128)
TAILS = (1, 55, 56, 63, 64, 119, 120, 129)  # r < 56, r >= 56 (a length-only block), with and without a whole block
GRID = [(p, t) for p in PREFIXES for t in TAILS]
# k_sha1_lat's column LAST: msg_len is an argument, the column the last `width` bytes of the message
COLUMN_MSG_LENS = (2**29, 2**29 + 64, 2**32, 2**61 - 64)
COLUMN_WIDTHS = (64, 128)
# the streaming context: 63 + 1 + 65 bytes after P, the count exactly 2^32 and 2^35 after the second call
STREAM_PREFIXES = (2**29 - 64, 2**32 - 64)


def seeded_state(rng):
    """Five random words: a chaining state that is never the IV."""
    st = tuple(rng.getrandbits(32) for _ in range(5))
    assert st != IV
    return st


def grid_cases(orc, seed=0x51DE):
    """[(P, tail bytes, state)] for every pair of GRID, the same on every call."""
    rng = random.Random(seed)
    out = []
    for k, (p, t) in enumerate(GRID):
        out.append((p, bytes(orc.fill_synthetic(t, 1000 + k, seed)), seeded_state(rng)))
    return out


FLIP_BIT = 37  # wide-length launches with the fused compare: every fifth expectation has this bit flipped


def flip_every_fifth(digests):
    """(expectations as an (n, 20) array, wanted verdicts) for the wide-length compares."""
    exp = np.frombuffer(bytes(digests), dtype=np.uint8).reshape(-1, 20).copy()
    exp[::5, FLIP_BIT // 8] ^= 1 << (FLIP_BIT % 8)
    ok = np.ones(exp.shape[0], dtype=np.uint8)
    ok[::5] = 0
    return exp, ok
