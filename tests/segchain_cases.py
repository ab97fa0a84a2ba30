"""Batches for the chain form of whole segment lists (k_sha1_gather_chain;
test_gpu_segchain.py, test_gpu_segchain_barriers.py), in gather_cases' format,
with hashlib's digests of the concatenations, and the kernel's window / piece
plan worked out on the host from the segment lengths alone.

Every batch is built once per process and never changed."""
import random

import numpy as np

import gather_cases as gc

SEED = 0x5E6C
WINDOW = 1024          # non-empty segments per window (kGatherWindow)
PIECE = 1 << 31        # the production piece
PAD_TOTALS = (1, 55, 56, 63, 64, 65, 119, 120, 128, 1484)
WINDOW_COUNTS = (1023, 1024, 1025, 2048, 2049, 3000)
EMPTY_DIGEST = bytes.fromhex("da39a3ee5e6b4b0d3255bfef95601890afd80709")

_cache = {}


def cut(rng, total, pieces):
    """`total` bytes cut at random places into at most `pieces` non-empty lengths."""
    marks = sorted(rng.sample(range(1, total), min(pieces - 1, total - 1))) if total > 1 else []
    return [b - a for a, b in zip([0] + marks, marks + [total])]


def padding_batch(orc):
    """The padding edges: message 0 lists nothing, message 1 three empty
    segments; then one message per PAD_TOTALS length, cut at random places into
    up to five segments that lie in descending address order at every residue
    mod 16; two messages that share a segment; one whose two segments overlap;
    last a 512 KiB chunk as 354 datagrams in shuffled arrival order."""
    if "padding" in _cache:
        return _cache["padding"]
    rng = random.Random(SEED)
    b = gc.Builder(SEED + 1)
    b.message([])
    b.message_of([0, 0, 0])
    for total in PAD_TOTALS:
        b.message_of(cut(rng, total, 5))
    s1, s2, s3 = b.place(70), b.place(45), b.place(85)
    b.message([s1, s2])
    b.message([s2, s3])
    off, _ = b.place(150)
    b.message([(off, 100), (off + 50, 100)])
    chunk = bytes(orc.fill_synthetic(gc.CHUNK, 77, SEED))
    segs = gc.datagram_chunk(b, chunk, rng)
    assert len(segs) == 354 and segs[-1][1] == gc.LAST_PAYLOAD
    b.message(segs)
    out = b.done()
    assert out["n"] == 2 + len(PAD_TOTALS) + 4 and out["want"][:40] == EMPTY_DIGEST * 2
    assert out["want"][-20:] == orc.sha1(chunk)
    _cache["padding"] = out
    return out


def small_segments(b, rng, pool, count):
    """`count` segments of 1 .. 3 bytes anywhere in the pool (off, len): any alignment, any order, overlapping."""
    off, size = pool
    return [(off + rng.randrange(size - 3), rng.randint(1, 3)) for _ in range(count)]


def sprinkle(rng, segs, empties, run):
    """`empties` zero-length segments put into the list, `run` of them in a row."""
    out = list(segs)
    at = rng.randrange(1, len(out))
    out[at:at] = [(rng.randrange(1 << 20), 0)] * run  # an empty segment's offset is never used
    for _ in range(empties - run):
        out.insert(rng.randrange(len(out) + 1), (0, 0))
    return out


def window_batch():
    """The window edges.  Messages 0..5: WINDOW_COUNTS segments of 1 .. 3
    bytes (a block spans dozens of them, a window ends inside a block);
    6..11: the same lists with 1500 empty segments put in, 1100 of them in a
    row; 12: 60 bytes, 1100 empty segments, then 100 small segments."""
    if "window" in _cache:
        return _cache["window"]
    rng = random.Random(SEED + 2)
    b = gc.Builder(SEED + 3)
    pool = b.place(4096)
    lists = [small_segments(b, rng, pool, c) for c in WINDOW_COUNTS]
    for segs in lists:
        b.message(segs)
    for segs in lists:
        b.message(sprinkle(rng, segs, 1500, 1100))
    b.message([(pool[0] + 5, 60)] + [(7, 0)] * 1100 + small_segments(b, rng, pool, 100))
    out = b.done()
    assert out["n"] == 13
    _cache["window"] = out
    return out


def piece_batch():
    """Message 0: 10 KiB in 37 segments; message 1: 2500 segments of 1 .. 3 bytes."""
    if "piece" in _cache:
        return _cache["piece"]
    rng = random.Random(SEED + 4)
    b = gc.Builder(SEED + 5)
    b.message_of(cut(rng, 10240, 37))
    assert b.count[0] == 37
    b.message(small_segments(b, rng, b.place(4096), 2500))
    out = b.done()
    _cache["piece"] = out
    return out


def mixed_batch(n=65):
    """n messages of mixed lengths, empties among them: every third lists
    nothing or only empty segments, the others 1 .. 700 bytes in up to six
    segments with an empty one between."""
    key = ("mixed", n)
    if key in _cache:
        return _cache[key]
    rng = random.Random(SEED + 6)
    b = gc.Builder(SEED + 7)
    for k in range(n):
        if k % 3 == 1:
            b.message_of([0] * (k % 4))
        else:
            lens = cut(rng, rng.randint(1, 700), 6)
            lens.insert(rng.randrange(len(lens) + 1), 0)
            b.message_of(lens, descending=bool(k & 1))
    out = b.done()
    _cache[key] = out
    return out


def lengths(batch, i):
    """Segment lengths of message i of a batch."""
    first, count = int(batch["first"][i]), int(batch["count"][i])
    return [n for _, n in batch["seg_list"][first:first + count]]


def plan(lens, piece=PIECE, window=WINDOW):
    """What k_sha1_gather_chain does with a message of these segment lengths:
    [(from, len, total)] per window built -- total 0 for an advance, None for
    the empty message, whose one window calls nothing.  The walk as the kernel's
    comment states it: the next `window` non-empty segments from entry k, A =
    their bytes - skip, a finish when the list ended there and A <= piece, else
    an advance over min(A, piece) & ~63 bytes and a slide."""
    k, skip, done, out = 0, 0, 0, []
    while True:
        kept, used = [], 0  # kept: (list index, len)
        while len(kept) < window and k + used < len(lens):
            if lens[k + used]:
                kept.append((k + used, lens[k + used]))
            used += 1
        a = sum(n for _, n in kept) - skip
        if k + used == len(lens) and a <= piece:
            out.append((skip, a, done + a) if done + a else None)
            return out
        step = min(a, piece) & ~63
        assert step >= 64, (a, piece)
        out.append((skip, step, 0))
        t, done, pos = skip + step, done + step, 0
        k, skip = k + used, 0  # the piece ended with the window, unless a kept segment holds byte t
        for idx, n in kept:
            if pos <= t < pos + n:
                k, skip = idx, t - pos
                break
            pos += n


def barriers(lens, piece=PIECE):
    """(waves checked, barriers counted) per wave of the message's workgroup in
    the barrier-accounting build: one check and one barrier per window, and per
    body call one check and nbatch + 1 barriers, nbatch = ceil(nb / 64) with
    nb = len >> 6 for an advance, (len >> 6) + ((len & 63) >= 56 ? 2 : 1) for
    the finish."""
    p = plan(lens, piece)
    checks, bars = 1, len(p)
    for call in p:
        if call is None:
            continue
        _, n, total = call
        nb = (n >> 6) + ((2 if (n & 63) >= 56 else 1) if total else 0)
        checks += 1
        bars += -(-nb // 64) + 1
    return checks, bars

