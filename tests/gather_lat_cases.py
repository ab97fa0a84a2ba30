"""Batches for the latency-form gather tests (test_gpu_gather_lat.py,
test_gpu_gather_lat_barriers.py), built with gather_cases' builders: once per
process, never changed."""
import hashlib
import random

import numpy as np

import gather_cases as gc

SEED = 0x1A7
_cache = {}


def mixed_batch():
    """130 messages.  0..128: the host walk's cases in turn (empty messages,
    r < 56 and r >= 56, cuts in every quad, segments under 16 bytes, three and
    more segments in a block, empty segments), two of them sharing a segment;
    segments of a message in descending address order.  129: the longest, four
    datagram payloads (1484 x 3 + 436 bytes = 77 blocks) behind 16-byte headers
    in shuffled arrival order with a duplicate."""
    if "mixed" in _cache:
        return _cache["mixed"]
    b = gc.Builder(SEED)
    k = 0
    while len(b.first) < 127:
        b.message_of(gc.WALK_CASES[(11 * k) % len(gc.WALK_CASES)], descending=not (k % 3 == 2))
        k += 1
    s1, s2, s3 = b.place(70), b.place(45), b.place(85)
    b.message([s1, s2])
    b.message([s2, s3])
    rng = random.Random(SEED + 1)
    data = rng.randbytes(3 * gc.PAYLOAD + gc.LAST_PAYLOAD)
    b.message(gc.datagram_chunk(b, data, rng, window=4))
    out = b.done()
    assert out["n"] == 130
    shared = set(out["seg_list"][int(out["first"][127]):][:2]) & set(out["seg_list"][int(out["first"][128]):][:2])
    assert len(shared) == 1  # messages 127 and 128 list one segment both
    out["lens"] = [sum(n for _, n in out["seg_list"][f:f + c]) for f, c in zip(out["first"], out["count"])]
    assert 0 in out["lens"] and max(out["lens"][:129]) <= 200 and out["lens"][129] == 4888
    _cache["mixed"] = out
    return out


def pick(batch, idx):
    """The batch's tables for messages idx (any order, repeats allowed)."""
    idx = np.asarray(idx, dtype=np.int64)
    want = b"".join(batch["want"][20 * i:20 * i + 20] for i in idx)
    return batch["first"][idx], batch["count"][idx], want, [batch["lens"][i] for i in idx]


def longest_last(batch, n):
    """n messages of mixed_batch with the longest one in lane n - 1: the last
    lane of a workgroup (n = 64) or a lane past which n ends."""
    idx = list(range(n))
    idx[n - 1] = 129
    return pick(batch, idx)


def small_batch():
    """256 messages of 100..300 bytes in one to three segments, for tiling up
    to the smallest three-slot grid."""
    if "small" in _cache:
        return _cache["small"]
    b = gc.Builder(SEED + 2)
    rng = random.Random(SEED + 3)
    for k in range(256):
        total = 100 + (k * 201) // 256 if k < 255 else 300
        parts = 1 + k % 3
        cuts = sorted(rng.randrange(1, total) for _ in range(parts - 1))
        b.message_of([hi - lo for lo, hi in zip([0] + cuts, cuts + [total])], descending=bool(k & 1))
    out = b.done()
    out["lens"] = [sum(n for _, n in out["seg_list"][f:f + c]) for f, c in zip(out["first"], out["count"])]
    assert min(out["lens"]) == 100 and max(out["lens"]) == 300
    _cache["small"] = out
    return out


def tiled(batch, n):
    reps = -(-n // batch["n"])
    return (np.tile(batch["first"], reps)[:n], np.tile(batch["count"], reps)[:n], (batch["want"] * reps)[:20 * n],
            (batch["lens"] * reps)[:n])


def tiled_with_seams(batch, n):
    """tiled(), with seam shapes swapped in: every 97th message (from 5) and
    the last one, alone in its workgroup, are EMPTY (seg_count 0), every 89th
    (from 11) is cut down to its first segment (1 .. 299 bytes)."""
    if ("seams", n) in _cache:
        return _cache[("seams", n)]
    first, count, want, lens = tiled(batch, n)
    count, want, lens = count.copy(), bytearray(want), list(lens)
    blob = batch["blob"].tobytes()
    for i in list(range(5, n, 97)) + [n - 1]:
        count[i], lens[i], want[20 * i:20 * i + 20] = 0, 0, hashlib.sha1(b"").digest()
    for i in range(11, n - 1, 89):
        if count[i] == 0:
            continue
        off, length = batch["seg_list"][int(first[i])]
        count[i], lens[i], want[20 * i:20 * i + 20] = 1, length, hashlib.sha1(blob[off:off + length]).digest()
    assert lens.count(0) >= 3 and min(x for x in lens if x) < 100 and lens[n - 1] == 0
    _cache[("seams", n)] = (first, count, bytes(want), lens)
    return _cache[("seams", n)]


def blocks(length):
    return (length >> 6) + (2 if length & 63 >= 56 else 1)


def barrier_want(lens, slots):
    """(waves checked, barriers counted) of one launch over messages of these
    lengths: 2 waves per workgroup, each nbmax + SLOTS - 1 barriers."""
    waves = bars = 0
    for w in range(0, len(lens), 64):
        nbmax = max(blocks(x) for x in lens[w:w + 64])
        waves += 2
        bars += 2 * (nbmax + slots - 1)
    return waves, bars
