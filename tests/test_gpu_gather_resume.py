"""GPU: the chain-form gather kernel in its array form
(bt_sha1_gather_resume_dev -> k_sha1_gather_resume) on device memory, against
the oracle: every cut of a block across two segments in one launch, resuming
at the loader-batch seams, the listed prefix as the read bound, the fused
compare, and a chunk received as shuffled datagrams advanced in steps."""
import random

import numpy as np
import pytest

import gather_cases as gc
import gather_resume_cases as grc
from conftest import load_btsha1
from resume_cases import FINISH_R, IV, SENT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    assert torch.cuda.is_available()
    return load_btsha1(), torch, oracle


def _collect():
    cases = []
    return cases, lambda name, launches, problems: cases.append((name, launches, problems))


def test_every_cut_in_one_launch(env):
    """All non-empty messages of straddle_batch, each ONE finishing entry from
    the IV: cuts 1..64, tiny and empty segments, shared segments, descending
    address order.  (total == 0 means advance, so the empty messages cannot be
    finished and are left out.)"""
    bt, torch, orc = env
    batch = gc.straddle_batch()
    t = grc.from_batch(torch, batch)
    lens = [sum(n for _, n in batch["seg_list"][int(f):int(f) + int(c)]) for f, c in zip(batch["first"], batch["count"])]
    keep = [i for i, n in enumerate(lens) if n]
    assert len(keep) >= 250 and len(keep) < batch["n"]
    states, dig, _, clean = t.launch(bt, [batch["first"][i] for i in keep], [batch["count"][i] for i in keep],
                                     [0] * len(keep), [lens[i] for i in keep], [lens[i] for i in keep],
                                     [IV] * len(keep))
    bad = [i for e, i in enumerate(keep) if dig[e] != batch["want"][20 * i:20 * i + 20]]
    assert not bad and clean, bad
    assert states == [IV] * len(keep)  # a finish writes no state back


@pytest.mark.parametrize("mixed", [False, True])
def test_resume_at_the_loader_batch_seams(env, mixed):
    bt, torch, orc = env
    cases, report = _collect()
    grc.run_seams(bt, torch, orc, report, mixed=mixed)
    assert len(cases) == (3 if mixed else 2)
    assert not [c for c in cases if c[2]], [c for c in cases if c[2]]


def test_only_the_listed_prefix_is_read(env):
    """Entry p lists the first p segments of one message and advances, then
    finishes, the message that those p segments are.  The descriptor and pos
    rows after them are valid but point at other bytes of the blob; the filler
    between segments is 0xEE in one run and 0x11 in the other.  A kernel that
    read a descriptor past the listed ones, or a byte outside a segment, would
    give another state or digest in at least one run."""
    bt, torch, orc = env
    rng = random.Random(5)
    data = bytes(orc.fill_synthetic(64 * 20 + 37, 500, gc.SEED))
    lens = grc.carve(len(data), (100, 3, 0, 61, 1, 200))
    results = []
    for filler in (0xEE, 0x11):
        blob, real, at, o = bytearray(), [], 0, 0
        for k, n in enumerate(lens):
            blob += bytes([filler]) * (16 + k % 16)
            real.append((len(blob), n))
            blob += data[o:o + n]
            o += n
        blob += bytes([filler]) * 64
        nseg = len(real)
        rows, pos, first, count, totals = [], [], [], [], []
        for p in range(1, nseg + 1):
            first.append(len(rows))
            count.append(p)
            at = 0
            for k in range(nseg):
                if k < p:
                    rows.append(real[k])
                    pos.append(at)
                    at += real[k][1]
                else:  # decoys: in bounds, other bytes, positions that would attract the seek
                    rows.append((rng.randrange(0, len(blob) - 64), 64))
                    pos.append(rng.randrange(0, at + 1))
            totals.append(at)
        keep = [e for e, tot in enumerate(totals) if tot]
        first, count, totals = ([x[e] for e in keep] for x in (first, count, totals))
        seg_rows = np.array(rows, dtype=np.uint64)
        t = grc.Tables(torch, np.frombuffer(bytes(blob), dtype=np.uint8), seg_rows, np.array(pos, dtype=np.uint64))
        n = len(first)
        whole = [tot & ~63 for tot in totals]
        states, _, _, clean = t.launch(bt, first, count, [0] * n, whole, [0] * n, [IV] * n)
        assert clean
        assert states == [orc.compress_blocks(IV, data[:w]) for w in whole]
        after, dig, _, clean = t.launch(bt, first, count, whole, [tot - w for tot, w in zip(totals, whole)], totals,
                                        states)
        assert clean and after == states
        assert dig == [orc.sha1(data[:tot]) for tot in totals]
        results.append((states, dig))
    assert results[0] == results[1]


def test_fused_compare_right_and_wrong_in_the_first_and_last_bit(env):
    bt, torch, orc = env
    batch = grc.seam_batch(orc)
    t = grc.from_batch(torch, batch)
    want = batch["want"][:20]
    flip = lambda bit: bytes(b ^ (0x80 >> (bit % 8) if k == bit // 8 else 0) for k, b in enumerate(want))
    expected = [want, flip(0), flip(159), bytes([0x5A]) * 20]
    n = len(expected)
    total = len(batch["msgs"][0])
    totals = [total, total, total, 0]  # the last entry advances: its verdict and digest stay untouched
    states, dig, oks, clean = t.launch(bt, [batch["first"][0]] * n, [batch["count"][0]] * n, [0] * n, [total] * n,
                                       totals, [IV] * n, expected=expected)
    assert clean and oks == [1, 0, 0, SENT]
    assert dig == [want, want, want, bytes([SENT]) * 20]
    # digests may be NULL with the compare
    _, dig, oks, clean = t.launch(bt, [batch["first"][0]] * 3, [batch["count"][0]] * 3, [0] * 3, [total] * 3,
                                  [total] * 3, [IV] * 3, expected=expected[:3], digests=False)
    assert clean and oks == [1, 0, 0] and dig == [bytes([SENT]) * 20] * 3


def test_datagram_chunk_advanced_in_steps_and_a_short_one_at_once(env):
    """One 512 KiB chunk as 354 shuffled datagrams with a duplicate, advanced in
    eight 64 KiB steps, each listing only the segments that cover it, then
    finished (len == 0: the padding alone); and a chunk of 3 x 1484 + 436 bytes
    in one finishing entry."""
    bt, torch, orc = env
    b = gc.Builder(gc.SEED + 11)
    rng = random.Random(gc.SEED + 12)
    big = bytes(orc.fill_synthetic(gc.CHUNK, 600, gc.SEED))
    small = bytes(orc.fill_synthetic(3 * gc.PAYLOAD + gc.LAST_PAYLOAD, 601, gc.SEED))
    for data in (big, small):
        b.message(gc.datagram_chunk(b, data, rng))
    batch = b.done()
    assert list(batch["count"]) == [354, 4]
    t = grc.from_batch(torch, batch)
    state = IV
    step = 64 << 10
    for j in range(8):
        listed = -(-step * (j + 1) // gc.PAYLOAD)  # segments that cover the first 64 KiB x (j + 1)
        (state,), _, _, clean = t.launch(bt, [0], [listed], [step * j], [step], [0], [state])
        assert clean and state == orc.compress_blocks(IV, big[:step * (j + 1)]), j
    _, dig, _, clean = t.launch(bt, [0, batch["first"][1]], [354, 4], [gc.CHUNK, 0], [0, len(small)],
                                [gc.CHUNK, len(small)], [state, IV])
    assert clean and dig == [orc.sha1(big), orc.sha1(small)]
