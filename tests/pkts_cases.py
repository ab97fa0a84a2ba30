"""Batches for the packet-buffer tests (test_gpu_pkts.py): messages held as the
payloads of equal-sized packet buffers (bt_sha1_pkt_geom), with the oracle's
digests of the assembled messages.  tests/native/pkt_walk_check.cpp walks the
same geometries, lengths and orders on the host.

A batch is built once per geometry and process and never changed:
  blob         the slots, one per base message (numpy uint8); every byte
               outside a listed payload is poison: headers, slack, unused
               buffers, and one duplicate datagram that holds other bytes
  slot_off     uint64 per message, len uint32 per message
  order        the order tables, one after the other (uint32)
  order_first  uint64 per message
  segs/first/count   the segment lists the orders imply (bt_sha1_seg rows)
  want         20 * n digest bytes
The first BASE entries are the base messages, one per (length, order); the
entries after them repeat base messages (messages may share slots) so that a
launch of any n <= N mixes lengths inside every wave, with the longest message
in lane 0 and in lane 63 of the first wave.
"""
import random

import numpy as np

SEED = 0x9C75
GEOMETRIES = [(1500, 16, 1484), (76, 4, 68), (64, 0, 64), (144, 16, 128)]  # stride, header, payload
SLOT_PKTS = 24
ORDERS = ("identity", "reversed", "permuted", "one buffer")
N = 257
POISON = 0xEE


def lengths(payload):
    p = payload
    return [0, 1, 55, 56, 63, 64, 65, p - 1, p, p + 1, p + 55, p + 56,
            17 * p, 17 * p + 4, 17 * p + 55, 17 * p + 56, 17 * p + 63, 3 * p - 1]


def npkt(length, payload):
    return -(-length // payload)


def make_order(kind, count, rng):
    if kind == "identity":
        return list(range(count))
    if kind == "reversed":
        return list(range(count - 1, -1, -1))
    if kind == "permuted":  # over more buffers than the message has datagrams
        return rng.sample(range(SLOT_PKTS), count)
    return [SLOT_PKTS // 2] * count  # legal: the message repeats that buffer


def fill_slot(geom, length, order, rng):
    """One slot holding a message of `length` bytes in the buffers `order`
    names; returns (slot bytes, the message as the slot holds it)."""
    stride, header, payload = geom
    slot = bytearray([POISON]) * (SLOT_PKTS * stride)
    for k, j in enumerate(order):
        nbytes = min(payload, length - k * payload)
        at = j * stride + header
        slot[at:at + nbytes] = rng.randbytes(nbytes)
    unused = [j for j in range(SLOT_PKTS - 1) if j not in order]
    if unused and order:  # a duplicate datagram that was dropped: same header, other bytes
        at = unused[0] * stride
        slot[at:at + header + payload] = bytes([0xD6]) * header + rng.randbytes(payload)
    if SLOT_PKTS - 1 not in order:  # what a clamped out-of-range entry reads (clamped_want)
        at = (SLOT_PKTS - 1) * stride + header
        slot[at:at + payload] = rng.randbytes(payload)
    msg = b"".join(bytes(slot[j * stride + header:j * stride + header + min(payload, length - k * payload)])
                   for k, j in enumerate(order))
    assert len(msg) == length
    return slot, msg


_cache = {}


def batch(orc, geom):
    if geom in _cache:
        return _cache[geom]
    stride, header, payload = geom
    rng = random.Random(SEED + stride)
    blob, slot_off, lens, order, order_first, want, segs, first, count = bytearray(), [], [], [], [], [], [], [], []
    for length in lengths(payload):
        for kind in ORDERS:
            o = make_order(kind, npkt(length, payload), rng)
            slot, msg = fill_slot(geom, length, o, rng)
            slot_off.append(len(blob))
            blob += slot
            lens.append(length)
            order_first.append(len(order))
            first.append(len(segs))
            count.append(len(o))
            segs += [(slot_off[-1] + j * stride + header, min(payload, length - k * payload)) for k, j in enumerate(o)]
            order += o
            want.append(orc.sha1(msg))
    base = len(lens)
    longest = max(range(base), key=lambda i: (lens[i], ORDERS[i % 4] == "permuted"))
    # n entries in all: the longest message in lanes 0 and 63, between and
    # after them the base messages in a stride that mixes lengths in a wave.
    pick = [longest] + [(7 * k) % base for k in range(62)] + [longest]
    pick += [(11 * k + 3) % base for k in range(N - len(pick))]
    # every base message appears: the first `base` entries after lane 63 cover them
    pick[64:64 + base] = list(range(base))
    idx = np.array(pick[:N])
    seg = np.zeros((len(segs), 2), dtype=np.uint64)
    for k, (o, n) in enumerate(segs):
        seg[k] = (o, n)
    out = {"geom": geom, "n": N, "base": base, "blob": np.frombuffer(bytes(blob), dtype=np.uint8),
           "slot_off": np.array(slot_off, dtype=np.uint64)[idx], "len": np.array(lens, dtype=np.uint32)[idx],
           "order": np.array(order + [0xFFFFFFFF], dtype=np.uint32),  # never empty; the last entry is never read
           "order_first": np.array(order_first, dtype=np.uint64)[idx],
           "segs": seg, "first": np.array(first, dtype=np.uint64)[idx], "count": np.array(count, dtype=np.uint32)[idx],
           "want": b"".join(want[i] for i in idx)}
    assert len(set(pick[:N])) == base and out["len"][0] == out["len"][63] == max(lens)
    _cache[geom] = out
    return out


def clamped_want(orc, b):
    """Digests of batch b's messages when every order entry is out of range:
    each position then reads buffer SLOT_PKTS - 1 of the message's slot."""
    stride, header, payload = b["geom"]
    out = []
    for off, length in zip(b["slot_off"], b["len"]):
        at = int(off) + (SLOT_PKTS - 1) * stride + header
        buf = bytes(b["blob"][at:at + payload])
        out.append(orc.sha1((buf * (int(length) // payload + 1))[:int(length)]))
    return b"".join(out)
