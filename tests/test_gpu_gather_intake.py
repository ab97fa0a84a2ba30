"""GPU: the gather intake (bt_sha1_intake_create_gather / _append /
_commit_gather -> k_sha1_gather_resume_table): chunks received as datagrams
into pinned slots and hashed in place over the in-sequence prefix, against the
oracle, with the bookkeeping (bt_sha1_intake_stats) checked exactly."""
import ctypes
import random

import pytest

import gather_cases as gc
import gather_resume_cases as grc
from conftest import load_btsha1
from resume_cases import NEVER

pytestmark = pytest.mark.gpu
SHORT = 3 * gc.PAYLOAD + gc.LAST_PAYLOAD
LONG = 64 * 129 + 63


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    assert torch.cuda.is_available()
    return load_btsha1(), oracle


def _datagram(seq, part):
    return seq.to_bytes(4, "little") + bytes([0xD6]) * 12 + part


def _arrival(n, rng, window=4):
    order = []
    for w in range(0, n, window):
        grp = list(range(w, min(w + window, n)))
        rng.shuffle(grp)
        order += grp
    return order


@pytest.mark.parametrize("stride", [4096, NEVER])
def test_eight_slots_of_shuffled_datagrams(env, stride):
    """Every turn each chunk gets its next datagram (shuffled within windows
    of 4) where the last one ended; payloads are appended as gaps fill; the turn
    ends with kick + sync, after which the stats moved by exactly what the
    slots that were due predict."""
    bt, orc = env
    rng = random.Random(31)
    sizes = [SHORT] * 7 + [LONG]
    chunks = [bytes(orc.fill_synthetic(n, 700 + j, gc.SEED)) for j, n in enumerate(sizes)]
    want = [orc.sha1(c) for c in chunks]
    expected = list(want)
    expected[3] = bytes(20)  # one planted mismatch
    pays = [[c[o:o + gc.PAYLOAD] for o in range(0, len(c), gc.PAYLOAD)] for c in chunks]
    orders = [_arrival(len(p), rng) for p in pays]
    rx = bt.Intake(chunk_len=gc.DGRAM * 8, nslots=8, stride=stride, gather=True, max_segs=8)
    try:
        slots = [rx.slot() for _ in chunks]
        where = [dict() for _ in chunks]
        listed_segs = [0] * 8
        listed, hashed = [0] * 8, [0] * 8
        committed = set()
        for turn in range(max(len(o) for o in orders) + 1):
            due_adv, due_fin = {}, set()
            for j, order in enumerate(orders):
                if turn < len(order):
                    seq = order[turn]
                    pkt = _datagram(seq, pays[j][seq])
                    ctypes.memmove(slots[j] + turn * gc.DGRAM, pkt, len(pkt))
                    where[j][seq] = (turn * gc.DGRAM + gc.HEADER, len(pays[j][seq]))
                    ready = []
                    while listed_segs[j] in where[j]:
                        ready.append(where[j][listed_segs[j]])
                        listed_segs[j] += 1
                    if ready:
                        rx.append(slots[j], ready)
                        listed[j] += sum(n for _, n in ready)
                        whole = listed[j] & ~63
                        if whole > hashed[j] and whole - hashed[j] >= stride:
                            due_adv[j] = whole - hashed[j]
                if listed_segs[j] == len(pays[j]) and j not in committed:
                    rx.commit_gather(slots[j], expected[j], 100 + j)
                    committed.add(j)
                    due_fin.add(j)
                    due_adv.pop(j, None)  # a committed slot gets ONE finishing entry over everything left
            before = rx.stats()
            n = rx.kick()
            rx.sync()
            after = rx.stats()
            assert n == len(due_adv) + len(due_fin), (turn, n, due_adv, due_fin)
            assert after["entries"] - before["entries"] == n
            assert after["launches"] - before["launches"] == (1 if n else 0)
            assert after["advanced_bytes"] - before["advanced_bytes"] == sum(due_adv.values()), turn
            assert after["deferred"] == before["deferred"]
            for j, nbytes in due_adv.items():
                hashed[j] += nbytes
        assert len(committed) == 8
        if stride == NEVER:
            assert rx.stats()["advanced_bytes"] == 0
        else:
            assert rx.stats()["advanced_bytes"] > 0
        got = sorted(rx.drain())
        assert got == [(100 + j, j != 3, want[j]) for j in range(8)]
        assert rx.pending() == 0
    finally:
        rx.close()


def test_append_during_a_launch(env):
    """A 512 KiB chunk: half of it is appended and kicked, and while that
    launch may still be running the rest is appended and kicked again: the slot
    is deferred or advanced, never wrong."""
    bt, orc = env
    data = bytes(orc.fill_synthetic(gc.CHUNK, 720, gc.SEED))
    rx = bt.Intake(chunk_len=gc.DGRAM * 360, nslots=2, stride=64, gather=True, max_segs=360)
    try:
        p = rx.slot()
        segs, _ = grc.land(p, data, grc.carve(len(data), (gc.PAYLOAD,)))
        half = len(segs) // 2
        rx.append(p, segs[:half])
        assert rx.kick() == 1
        before = rx.stats()
        rx.append(p, segs[half:])
        n = rx.kick()
        after = rx.stats()
        assert n in (0, 1) and (after["deferred"] - before["deferred"]) + n == 1
        rx.sync()
        rx.commit_gather(p, orc.sha1(data), 9)
        assert rx.drain() == [(9, True, orc.sha1(data))]
        assert rx.stats()["advanced_bytes"] == (half * gc.PAYLOAD & ~63) + (n * ((len(data) & ~63) - (half * gc.PAYLOAD & ~63)))
    finally:
        rx.close()


def test_refused_appends_leave_the_slot_intact(env):
    bt, orc = env
    data = bytes(orc.fill_synthetic(SHORT, 730, gc.SEED))
    slot_len = 1 << 20
    rx = bt.Intake(chunk_len=slot_len, nslots=3, stride=64, gather=True, max_segs=40)
    try:
        p = rx.slot()
        segs, _ = grc.land(p, data, grc.carve(len(data), (gc.PAYLOAD,)))
        rx.append(p, segs[:2])
        with pytest.raises(bt.BtSha1Error, match="exceed max_segs 40"):
            rx.append(p, [segs[2]] * 39)
        with pytest.raises(bt.BtSha1Error, match="reaches past slot_len"):
            rx.append(p, [segs[2], (slot_len - 10, 11)])
        with pytest.raises(bt.BtSha1Error, match="reaches past slot_len"):
            rx.append(p, [(1 << 40, 1)])
        assert rx.kick() == 1  # the two payloads listed before the refusals
        rx.sync()
        rx.append(p, segs[2:])
        rx.commit_gather(p, orc.sha1(data), 1)
        # a running total above 32 MiB: the same 1 MiB listed 33 times
        q = rx.slot()
        ctypes.memmove(q, data, len(data))
        rx.append(q, [(0, slot_len)] * 32)
        with pytest.raises(bt.BtSha1Error, match="exceed 32 MiB"):
            rx.append(q, [(0, 1)])
        with pytest.raises(bt.BtSha1Error, match="no bytes listed"):
            _commit_empty(rx)
        rx.release(q)
        assert rx.drain() == [(1, True, orc.sha1(data))]
    finally:
        rx.close()


def _commit_empty(rx):
    """commit_gather on a slot with nothing listed is refused; the slot goes back."""
    q = rx.slot()
    try:
        rx.commit_gather(q, bytes(20), 0)
    finally:
        rx.release(q)


def test_release_mid_chunk_and_reuse(env):
    bt, orc = env
    a = bytes(orc.fill_synthetic(LONG, 740, gc.SEED))
    b = bytes(orc.fill_synthetic(SHORT, 741, gc.SEED))
    rx = bt.Intake(chunk_len=gc.DGRAM * 8, nslots=1, stride=64, gather=True, max_segs=8)
    try:
        p = rx.slot()
        segs, _ = grc.land(p, a, grc.carve(len(a), (gc.PAYLOAD,)))
        rx.append(p, segs[:3])
        assert rx.kick() == 1
        rx.release(p)  # waits for the launch in flight; the list is empty and the state the IV again
        order = [1, 0, 0, 3, 2]  # out of order, with a duplicate
        q = rx.receive_datagrams(b, order, orc.sha1(b), 77, each=lambda s: rx.kick())
        assert q == p
        assert rx.drain() == [(77, True, orc.sha1(b))]
        assert rx.stats()["released"] == 1
    finally:
        rx.close()


def test_the_two_kinds_refuse_each_others_calls(env):
    bt, orc = env
    plain = bt.Intake(chunk_len=4096, nslots=1)
    gather = bt.Intake(chunk_len=4096, nslots=1, gather=True, max_segs=4)
    try:
        p, g = plain.slot(), gather.slot()
        with pytest.raises(bt.BtSha1Error, match="needs a gather intake"):
            plain.append(p, [(0, 64)])
        with pytest.raises(bt.BtSha1Error, match="needs a gather intake"):
            plain.commit_gather(p, bytes(20), 0)
        with pytest.raises(bt.BtSha1Error, match="refused on a gather intake"):
            gather.advance(g, 64)
        with pytest.raises(bt.BtSha1Error, match="refused on a gather intake"):
            gather.commit(g, bytes(20), 0, 64)
        # both still work
        data = bytes(orc.fill_synthetic(4096, 750, gc.SEED))
        ctypes.memmove(p, data, 4096)
        ctypes.memmove(g, data, 4096)
        plain.advance(p, 4096)
        plain.commit(p, orc.sha1(data), 1)
        gather.append(g, [(0, 4096)])
        gather.commit_gather(g, orc.sha1(data), 2)
        assert plain.drain() == [(1, True, orc.sha1(data))] and gather.drain() == [(2, True, orc.sha1(data))]
    finally:
        plain.close()
        gather.close()
