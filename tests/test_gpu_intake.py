"""GPU: bt_sha1_intake, progressive receive for many chunks at once: advance
and commit only record, and one kick advances (or finishes) every due slot in a
single launch of the table-driven resumable chain kernel.

Every count asserted here is taken after sync(), so none depends on how fast a
launch runs; where a race is possible the assertion is one that holds on both
sides of it.
"""
import ctypes
import os

import pytest

import intake_cases as ic
import resume_cases as rc
from conftest import GOLDEN, c_tar_bytes, load_btsha1

pytestmark = pytest.mark.gpu
TABLES = 8  # bt_intake.cpp kTables: launches that may be in flight at once


@pytest.fixture(scope="module")
def bt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    m = load_btsha1()
    assert m.device_count() >= 1
    return m


def collect():
    cases = []

    def report(name, launches, problems):
        print(name, len(launches), "entries", problems)
        cases.append((name, launches, problems))
    return cases, report


@pytest.mark.parametrize("nslots", [5, 65])  # 65: past the receiver's 64
def test_one_launch_serves_many_slots(bt, oracle, nslots):
    chunk_len, stride = 4160, 1024
    data = [ic.chunk(oracle, chunk_len, 10 + k) for k in range(nslots)]
    want = [oracle.sha1(d) for d in data]
    ix = bt.Intake(chunk_len=chunk_len, nslots=nslots, stride=stride)
    try:
        slots = [ix.slot() for _ in range(nslots)]
        assert len(set(slots)) == nslots
        for p, d in zip(slots, data):
            ic.put(p, d, 0, 2 * stride)
            ix.advance(p, 2 * stride)
        before = ix.stats()
        assert before["launches"] == 0 and before["kicks"] == 0  # advance records only
        assert ix.kick() == nslots
        ix.sync()
        d = ic.delta(ix, before)
        assert d["kicks"] == 1 and d["launches"] == 1 and d["entries"] == nslots and d["deferred"] == 0
        assert ix.stats()["max_entries"] == nslots and d["advanced_bytes"] == 2 * stride * nslots
        assert ix.kick() == 0 and ix.stats()["launches"] == 1  # nothing due
        for k, (p, dd) in enumerate(zip(slots, data)):
            ic.put(p, dd, 2 * stride)
            ix.commit(p, want[k], 1000 + k)
        assert ix.stats()["launches"] == 1 and ix.pending() == nslots  # commit records only
        assert sorted(ix.drain()) == [(1000 + k, True, want[k]) for k in range(nslots)]
        s = ix.stats()
        assert s["launches"] == 2 and s["entries"] == 2 * nslots and s["committed"] == nslots and ix.pending() == 0
    finally:
        ix.close()


@pytest.mark.parametrize("stride", [rc.NEVER, 64])
def test_finish_entries_of_every_padding_shape_in_one_launch(bt, oracle, stride):
    cases, report = collect()
    ic.run_padding_shapes(bt, oracle, report, stride)
    assert len(cases) == (1 if stride == rc.NEVER else 2)
    assert len(cases[-1][1]) == len(ic.SHAPES) == 29
    assert not [c for c in cases if c[2]], [c[2] for c in cases]


def test_advance_and_finish_entries_mixed_in_one_table(bt, oracle):
    cases, report = collect()
    ic.run_mixed(bt, oracle, report)
    assert len(cases) == 2 and {t != 0 for _, t in cases[0][1]} == {True, False}
    assert not [c for c in cases if c[2]], [c[2] for c in cases]


def test_nothing_at_or_past_filled_is_read(bt, oracle):
    """Bytes past `filled` hold 0xFF at the kick and other garbage before the
    sync: a launch that used one would hash either.  chunk_len is a 64-byte
    multiple, so the second slot's last span ends on the last byte of the
    pinned allocation."""
    chunk_len = 4160
    short = 3001  # r = 57: two padding blocks
    a_data, b_data = ic.chunk(oracle, short, 41), ic.chunk(oracle, chunk_len, 42)
    ix = bt.Intake(chunk_len=chunk_len, nslots=2, stride=64)
    try:
        a, b = ix.slot(), ix.slot()
        assert b == a + chunk_len
        for p in (a, b):
            ctypes.memset(p, 0xFF, chunk_len)
        ic.put(a, a_data, 0, 1000)
        ic.put(b, b_data, 0, 2000)
        ix.advance(a, 1000)
        ix.advance(b, 2000)
        assert ix.kick() == 2  # spans [0, 960) and [0, 1984)
        ctypes.memset(a + 1000, 0x11, chunk_len - 1000)
        ctypes.memset(b + 2000, 0x22, chunk_len - 2000)
        ix.sync()
        ic.put(a, a_data, 1000)
        ic.put(b, b_data, 2000)
        ix.commit(a, oracle.sha1(a_data), 1, length=short)
        ix.commit(b, oracle.sha1(b_data), 2)
        assert ix.kick() == 2  # [960, 3001) with its tail read byte by byte; [1984, 4160) up to the allocation's end
        ctypes.memset(a + short, 0x33, chunk_len - short)
        ix.sync()
        assert sorted(ix.drain()) == [(1, True, oracle.sha1(a_data)), (2, True, oracle.sha1(b_data))]
        assert ix.stats()["entries"] == 4 and ix.stats()["advanced_bytes"] == 960 + 1984
    finally:
        ix.close()


def test_a_slot_is_never_in_two_launches(bt, oracle):
    chunk_len, n = 4160, 3
    data = [ic.chunk(oracle, chunk_len, 50 + k) for k in range(2 * n)]
    want = [oracle.sha1(d) for d in data]
    ix = bt.Intake(chunk_len=chunk_len, nslots=n, stride=64)
    try:
        # 1. kick, sync, kick: every slot is idle at the second kick, nothing is deferred
        slots = [ix.slot() for _ in range(n)]
        for upto in (1000, 2000):
            for p, d in zip(slots, data):
                ic.put(p, d, 0, upto)
                ix.advance(p, upto)
            assert ix.kick() == n
            assert ix.stats()["deferred"] == 0
            ix.sync()
        for k, (p, d) in enumerate(zip(slots, data)):
            ic.put(p, d, 2000)
            ix.commit(p, want[k], k)
        assert sorted(ix.drain()) == [(k, True, want[k]) for k in range(n)]
        s = ix.stats()
        assert s["deferred"] == 0 and s["entries"] == 3 * n and s["launches"] == 3
        # 2. commit while the advance may still be in flight.  Whichever way that
        # race goes, a slot is taken by a kick only when it is idle, so each slot
        # is in exactly two (slot, kick) pairs -- its advance and ONE finishing
        # entry over the rest -- and a slot a kick skipped shows in `deferred`.
        slots = [ix.slot() for _ in range(n)]
        for p, d in zip(slots, data[n:]):
            ic.put(p, d, 0, 1000)
            ix.advance(p, 1000)
        assert ix.kick() == n
        for k, (p, d) in enumerate(zip(slots, data[n:])):
            ic.put(p, d, 1000)
            ix.commit(p, want[n + k], n + k)
        assert sorted(ix.drain()) == [(n + k, True, want[n + k]) for k in range(n)]
        d = ic.delta(ix, s)
        assert d["entries"] == 2 * n and d["deferred"] >= 0 and 2 <= d["launches"] <= 1 + n
        assert d["advanced_bytes"] == 960 * n  # the finishing entries took [960, 4160) whole
    finally:
        ix.close()


def test_table_ring_wraps(bt, oracle):
    """More launches than the ring has tables, first with a sync after each,
    then without any (the kick that finds the ring full waits for the oldest)."""
    chunk_len, n, steps = 12 * 1024 + 192, 2, TABLES + 4
    data = [ic.chunk(oracle, chunk_len, 60 + k) for k in range(n)]
    ix = bt.Intake(chunk_len=chunk_len, nslots=n, stride=64)
    try:
        slots = [ix.slot() for _ in range(n)]
        for step in range(1, steps + 1):
            for p, d in zip(slots, data):
                ic.put(p, d, 1000 * (step - 1), 1000 * step)
                ix.advance(p, 1000 * step)
            assert ix.kick() == n
            ix.sync()
        s = ix.stats()
        assert s["launches"] == steps > TABLES and s["entries"] == n * steps and s["deferred"] == 0
        assert s["advanced_bytes"] == n * ((1000 * steps) & ~63)
        for k, (p, d) in enumerate(zip(slots, data)):
            ic.put(p, d, 1000 * steps)
            ix.commit(p, oracle.sha1(d), k)
        assert sorted(ix.drain()) == [(k, True, oracle.sha1(data[k])) for k in range(n)]
    finally:
        ix.close()
    many = TABLES + 3
    small = [ic.chunk(oracle, 4160, 70 + k) for k in range(many)]
    ix = bt.Intake(chunk_len=4160, nslots=many, stride=rc.NEVER)
    try:
        for k, d in enumerate(small):  # one launch per slot, none waited for
            p = ix.slot()
            ic.put(p, d)
            ix.commit(p, oracle.sha1(d), k)
            assert ix.kick() == 1
        assert sorted(ix.drain()) == [(k, True, oracle.sha1(small[k])) for k in range(many)]
        assert ix.stats()["launches"] == many and ix.stats()["max_entries"] == 1
    finally:
        ix.close()


def test_release_and_reuse(bt, oracle):
    chunk_len = 4160
    data = [ic.chunk(oracle, chunk_len, 80 + k) for k in range(4)]
    ix = bt.Intake(chunk_len=chunk_len, nslots=2, stride=64)
    try:
        a, b = ix.slot(), ix.slot()
        ic.put(a, data[0], 0, 1000)
        ix.advance(a, 1000)  # due, never launched
        ix.release(a)
        assert ix.kick() == 0 and ix.stats()["launches"] == 0  # the span was dropped with the slot
        ic.put(b, data[1], 0, 3000)
        ix.advance(b, 3000)
        assert ix.kick() == 1  # in flight (or already finished) when released
        ix.release(b)
        assert ix.stats()["released"] == 2
        again = [ix.slot(), ix.slot()]  # at once, and from the IV
        assert again == [a, b]
        for k, p in enumerate(again):
            ic.put(p, data[2 + k])
            ix.advance(p, chunk_len)
            ix.commit(p, oracle.sha1(data[2 + k]), k)
        assert sorted(ix.drain()) == [(k, True, oracle.sha1(data[2 + k])) for k in range(2)]
        s = ix.stats()
        assert s["released"] == 2 and s["committed"] == 2 and s["entries"] == 3 and ix.pending() == 0
    finally:
        ix.close()


def test_all_slots_outstanding_and_misuse(bt, oracle):
    ix = bt.Intake(chunk_len=4160, nslots=2, stride=64)
    try:
        a, b = ix.slot(), ix.slot()
        with pytest.raises(bt.BtSha1Error, match="all 2 slots are outstanding"):
            ix.slot()
        ix.advance(a, 1000)
        with pytest.raises(bt.BtSha1Error, match="must not decrease"):
            ix.advance(a, 999)
        with pytest.raises(bt.BtSha1Error, match="exceed chunk_len"):
            ix.advance(a, 4161)
        assert ix.kick() == 1
        ix.sync()
        with pytest.raises(bt.BtSha1Error, match="already hashed"):
            ix.commit(a, bytes(20), 0, length=900)  # 960 bytes are hashed
        with pytest.raises(bt.BtSha1Error, match="not an outstanding slot"):
            ix.advance(a + 64, 1000)
        ix.release(a)
        with pytest.raises(bt.BtSha1Error, match="not an outstanding slot"):
            ix.release(a)
        ix.release(b)
        assert ix.poll() == [] and ix.drain() == [] and ix.pending() == 0
    finally:
        ix.close()


def test_reference_fixture_chunks_through_receive_all(bt, oracle):
    """The four chunks of tests/golden/C.tar.xz fed round-robin in 1484-byte
    payloads with one poll per turn, at the default 64 KiB stride, against the
    digests the reference's make-chunks wrote; one corrupted delivery fails."""
    img = c_tar_bytes()
    ref = [bytes.fromhex(l.split()[1]) for l in open(os.path.join(GOLDEN, "ref_C.chunks")).read().splitlines()[2:]]
    n = len(ref)
    assert n == 4 and len(img) == n * bt.CHUNK
    bad = bytearray(img[:bt.CHUNK])
    bad[400000] ^= 1
    chunks = [img[k * bt.CHUNK:(k + 1) * bt.CHUNK] for k in range(n)] + [bytes(bad)]
    ix = bt.Intake(nslots=8)
    try:
        got = ix.receive_all(chunks, ref + [ref[0]], list(range(n)) + [99])
        assert sorted(got) == [(k, True, ref[k]) for k in range(n)] + [(99, False, oracle.sha1(bytes(bad)))]
        s = ix.stats()
        assert s["committed"] == n + 1 and s["max_entries"] == n + 1 and s["deferred"] >= 0
        # Hashed before the commit: a slot is due once 64 KiB are unhashed, and a
        # deferred one is taken whole by a later poll, so only a launch that
        # outlasts the delivery of 190 KiB could leave more than half a chunk.
        # The chunk's last payload is committed in the turn it arrives, never advanced.
        assert (n + 1) * (bt.CHUNK // 2) <= s["advanced_bytes"] <= (n + 1) * (bt.CHUNK - 64)
    finally:
        ix.close()


def test_512_slots(bt, oracle):
    """The widest launch: every slot gets one payload per turn and every turn
    ends with one poll (its kick takes all 512 on the first turn)."""
    chunk_len, n = 4160, 512
    data = [ic.chunk(oracle, chunk_len, 1000 + k) for k in range(n)]
    want = [oracle.sha1(d) for d in data]
    ix = bt.Intake(chunk_len=chunk_len, nslots=n, stride=64)
    try:
        got = ix.receive_all(data, want, list(range(n)))
        assert sorted(got) == [(k, True, want[k]) for k in range(n)]
        s = ix.stats()
        assert s["max_entries"] == n and s["committed"] == n and ix.pending() == 0
        assert 2 * n <= s["entries"] <= 3 * n  # per slot: at least an advance and the finish, at most one entry per turn
    finally:
        ix.close()
