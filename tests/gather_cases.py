"""Batches for the scatter-gather tests (test_gpu_gather.py): messages given as
lists of segments of one byte image, with the digests hashlib gives for their
concatenations.

A batch is built once per process and never changed:
  blob    the byte image (numpy uint8)
  segs    (nseg, 2) uint64 rows (off, len | reserved << 32): the bt_sha1_seg table
  first   uint64 per message, count uint32 per message
  want    20 * n digest bytes
"""
import hashlib
import random

import numpy as np

SEED = 0x6A7E
DGRAM, HEADER, PAYLOAD, LAST_PAYLOAD = 1500, 16, 1484, 436
CHUNK = 512 * 1024


def ones(n):
    return [1] * n


# The host walk's cases (tests/native/gather_walk_check.cpp), each at most 200 bytes.
WALK_CASES = (
    [[cut, 64 - cut] for cut in range(1, 64)]
    + [[20, 20, 24], [90, 7, 90], ones(64), [68] + ones(64) + [68]]
    + [[0, 130], [70, 0, 70], [100, 0, 0, 100], [130, 0], [0, 0, 0], [0, 33, 0, 0, 31, 0, 64, 0, 5, 0]]
    + [[128, 72], [64, 10], [64, 64, 64], [16] * 12, [15] * 13, [17] * 11]
    + [c for tail in (0, 1, 55, 56, 63) for c in ([128 + tail] if tail < 56 else [64 + tail],
                                                   [tail] if tail else [64],
                                                   [66, tail // 2, 62 + tail - tail // 2] if tail > 1 else [64, 64],
                                                   [100, 28 + tail],
                                                   ones(64 + tail))]
    + [[]]
)


class Builder:
    """Segments are carved out of one image with a gap in front of each, so
    that consecutive segments start at consecutive residues mod 16."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.blob = bytearray()
        self.segs, self.first, self.count, self.want = [], [], [], []
        self.residue = 0

    def place(self, length):
        """A new segment of `length` random bytes: (off, len)."""
        pad = (self.residue - len(self.blob)) % 16 + 16
        self.blob += bytes([0xEE]) * pad
        self.residue = (self.residue + 1) % 16
        off = len(self.blob)
        self.blob += self.rng.randbytes(length)
        return (off, length)

    def message(self, segments):
        """One message listing these (off, len) segments, in this order."""
        self.first.append(len(self.segs))
        self.count.append(len(segments))
        self.segs += segments
        self.want.append(hashlib.sha1(b"".join(bytes(self.blob[o:o + n]) for o, n in segments)).digest())

    def message_of(self, lens, descending=True):
        """A message of fresh segments with these lengths; descending: the
        list runs against the address order."""
        placed = [self.place(n) for n in (reversed(lens) if descending else lens)]
        self.message(list(reversed(placed)) if descending else placed)

    def done(self):
        seg = np.zeros((max(len(self.segs), 1), 2), dtype=np.uint64)
        for k, (o, n) in enumerate(self.segs):
            seg[k] = (o, n | (0xABCD << 32))  # `reserved` is not read
        return {"blob": np.frombuffer(bytes(self.blob) + bytes(16), dtype=np.uint8), "segs": seg,
                "first": np.array(self.first, dtype=np.uint64), "count": np.array(self.count, dtype=np.uint32),
                "want": b"".join(self.want), "n": len(self.first), "seg_list": list(self.segs)}


_cache = {}


def straddle_batch():
    """320 messages.  0..63: 200 bytes each, message k cut after byte k + 1 of
    its second block (cuts 1..63 and the block-aligned 64, one per lane of one
    wave).  64..255: the host walk's cases, then two messages that share a
    segment, then mixed repeats.  256..319: a workgroup of empty messages.
    Segments of a message lie in descending address order; their offsets take
    every residue mod 16."""
    if "straddle" in _cache:
        return _cache["straddle"]
    b = Builder(SEED)
    for k in range(64):
        b.message_of([64 + k + 1, 200 - (64 + k + 1)])
    for lens in WALK_CASES:
        assert sum(lens) <= 200
        b.message_of(lens)
    s1, s2, s3 = b.place(70), b.place(45), b.place(85)
    b.message([s1, s2])
    b.message([s2, s3])
    k = 0
    while len(b.first) < 256:
        b.message_of(WALK_CASES[(7 * k) % len(WALK_CASES)], descending=bool(k & 1))
        k += 1
    for _ in range(64):
        b.message([])
    out = b.done()
    assert out["n"] == 320 and len({o % 16 for o, n in out["seg_list"] if n}) == 16
    _cache["straddle"] = out
    return out


def datagram_chunk(b, data, rng, window=8):
    """`data` as DATA datagrams (16-byte header starting with the sequence
    number, then up to 1484 bytes) landed in a shuffled arrival order within
    windows of `window`, one of them duplicated after its original.  Returns the
    segment list by sequence number, the duplicate not listed."""
    pays = [data[i:i + PAYLOAD] for i in range(0, len(data), PAYLOAD)]
    order = []
    for w in range(0, len(pays), window):
        grp = list(range(w, min(w + window, len(pays))))
        rng.shuffle(grp)
        order += grp
    dup_at = rng.randrange(1, len(order) + 1)
    order.insert(dup_at, order[rng.randrange(0, dup_at)])
    base = (len(b.blob) + 15) // 16 * 16
    b.blob += bytes(base - len(b.blob))
    where = {}
    for arrival, seq in enumerate(order):
        pkt = seq.to_bytes(4, "little") + bytes([0xD6]) * 12 + pays[seq]
        b.blob += pkt + bytes([0xEE]) * (DGRAM - len(pkt))
        where.setdefault(seq, base + arrival * DGRAM + HEADER)
    return [(where[seq], len(pays[seq])) for seq in range(len(pays))]


def datagram_batch(orc):
    """8 chunks of 512 KiB as 354 datagrams, then 56 chunks of 3 datagrams and
    a 436-byte last payload; want = the oracle's digests of the contiguous chunks."""
    if "dgram" in _cache:
        return _cache["dgram"]
    b = Builder(SEED + 1)
    rng = random.Random(SEED + 2)
    chunks = [bytes(orc.fill_synthetic(CHUNK, 40 + k, SEED)) for k in range(8)]
    chunks += [bytes(orc.fill_synthetic(3 * PAYLOAD + LAST_PAYLOAD, 90 + k, SEED)) for k in range(56)]
    for data in chunks:
        segs = datagram_chunk(b, data, rng)
        assert len(segs) == (354 if len(data) == CHUNK else 4) and segs[-1][1] == LAST_PAYLOAD
        b.message(segs)
    out = b.done()
    out["want"] = b"".join(orc.sha1(c) for c in chunks)
    assert out["want"] == b"".join(b.want)
    _cache["dgram"] = out
    return out
