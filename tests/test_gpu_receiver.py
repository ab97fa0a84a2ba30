"""GPU: bt_sha1_receiver, the progressive replacement of util.c:250-337 for
in-order receive: chunks delivered in 1484-byte payloads (util.c:275) with an
advance after each, hashed by the resumable chain kernel while they arrive.

The launch counters must equal what the stride rule predicts
(resume_cases.stride_rule): that is the proof that the prefix was hashed
before the commit, not at it.
"""
import ctypes
import os

import pytest

import resume_cases as rc
from conftest import GOLDEN, c_tar_bytes, load_btsha1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bt():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    m = load_btsha1()
    assert m.device_count() >= 1
    return m


def chunk(orc, n, seed):
    return bytes(orc.fill_synthetic(n, seed, 0x4EC))


@pytest.mark.parametrize("stride", [64, 4096, rc.NEVER])
@pytest.mark.parametrize("chunk_len", [12 * 1024 + 192, 4160])
def test_delivery_matrix(bt, oracle, chunk_len, stride):
    data = chunk(oracle, chunk_len, chunk_len + stride % 1000)
    want = oracle.sha1(data)
    rx = bt.Receiver(chunk_len=chunk_len, nslots=2, stride=stride)
    try:
        for tag, expected in ((1, want), (2, bytes(20))):
            before = rx.stats()
            rx.receive(data, expected, tag)
            assert rx.pending() == 1
            assert rx.drain() == [(tag, expected == want, want)]
            assert rx.pending() == 0
            s = rx.stats()
            launches, nadv, nbytes = rc.stride_rule(chunk_len, stride)
            assert s["advance_launches"] - before["advance_launches"] == nadv
            assert s["advanced_bytes"] - before["advanced_bytes"] == nbytes
            assert s["launches"] - before["launches"] == len(launches)
            if stride == rc.NEVER:
                assert nadv == 0 and nbytes == 0
            else:
                assert nbytes >= chunk_len - rc.PIECE - stride - 63  # the prefix was hashed before the commit
        assert rx.stats()["committed"] == 2
    finally:
        rx.close()


def test_byte_corrupted_before_it_is_advanced_fails(bt, oracle):
    chunk_len = 12 * 1024 + 192
    data = bytearray(chunk(oracle, chunk_len, 5))
    want = oracle.sha1(bytes(data))
    data[3000] ^= 0x40  # inside the third payload: advanced with it
    rx = bt.Receiver(chunk_len=chunk_len, nslots=1, stride=64)
    try:
        rx.receive(bytes(data), want, 9)
        assert rx.drain() == [(9, False, oracle.sha1(bytes(data)))]
    finally:
        rx.close()


def test_concurrent_slots_release_and_reuse(bt, oracle):
    """Four slots fed round-robin and committed out of order; slot 2 is
    released half-way and reused at once for another chunk, whose verdict it
    must give (its state restarted from the IV)."""
    chunk_len = 12 * 1024 + 192
    chunks = [chunk(oracle, chunk_len, 20 + k) for k in range(5)]
    want = [oracle.sha1(c) for c in chunks]
    rx = bt.Receiver(chunk_len=chunk_len, nslots=4, stride=1024)
    try:
        slots = [rx.slot() for _ in range(4)]
        assert len(set(slots)) == 4
        owner = [0, 1, 2, 3]  # chunk received in each slot
        pos = [0, 0, 0, 0]
        half = (chunk_len // 2 // rc.PIECE) * rc.PIECE
        while min(pos) < chunk_len:
            for k in range(4):
                if pos[k] >= chunk_len:
                    continue
                upto = min(pos[k] + rc.PIECE, chunk_len)
                rc.deliver(rx, slots[k], chunks[owner[k]], upto=upto, start=pos[k])
                pos[k] = upto
                if k == 2 and owner[2] == 2 and pos[2] >= half:  # aborted download
                    assert rx.stats()["advanced_bytes"] > 0
                    rx.release(slots[2])
                    again = rx.slot()
                    assert again == slots[2]
                    owner[2], pos[2] = 4, 0
        for k in (3, 0, 2, 1):
            rx.commit(slots[k], want[owner[k]], tag=owner[k])
        got = sorted(rx.drain())
        assert got == [(c, True, want[c]) for c in (0, 1, 3, 4)]
        s = rx.stats()
        assert s["released"] == 1 and s["committed"] == 4 and rx.pending() == 0
    finally:
        rx.close()


def test_commit_lengths(bt, oracle):
    chunk_len = 4160
    data = chunk(oracle, chunk_len, 31)
    rx = bt.Receiver(chunk_len=chunk_len, nslots=3, stride=64)
    try:
        # a short last chunk: len < chunk_len, tail of 20 bytes
        p = rx.slot()
        rc.deliver(rx, p, data, upto=3000)
        rx.commit(p, oracle.sha1(data[:3000]), 1, length=3000)
        # nothing advanced: the whole chain at commit
        q = rx.slot()
        ctypes.memmove(q, data, chunk_len)
        before = rx.stats()["advance_launches"]
        rx.commit(q, oracle.sha1(data), 2)
        assert rx.stats()["advance_launches"] == before
        # every byte advanced already (len a 64-byte multiple): the padding alone is left
        s = rx.slot()
        rc.deliver(rx, s, data)
        assert rx.stats()["advanced_bytes"] >= 2944 + chunk_len
        rx.commit(s, oracle.sha1(data), 3)
        assert sorted(rx.drain()) == [(1, True, oracle.sha1(data[:3000])), (2, True, oracle.sha1(data)),
                                      (3, True, oracle.sha1(data))]
    finally:
        rx.close()


def test_all_slots_outstanding_and_misuse(bt, oracle):
    rx = bt.Receiver(chunk_len=4160, nslots=2, stride=64)
    try:
        a, b = rx.slot(), rx.slot()
        with pytest.raises(bt.BtSha1Error, match="all 2 slots are outstanding"):
            rx.slot()
        rx.advance(a, 1000)
        with pytest.raises(bt.BtSha1Error, match="must not decrease"):
            rx.advance(a, 999)
        with pytest.raises(bt.BtSha1Error, match="exceed chunk_len"):
            rx.advance(a, 4161)
        with pytest.raises(bt.BtSha1Error, match="already hashed"):
            rx.commit(a, bytes(20), 0, length=900)  # 960 bytes are hashed
        with pytest.raises(bt.BtSha1Error, match="not an outstanding slot"):
            rx.advance(a + 64, 1000)
        rx.release(a)
        with pytest.raises(bt.BtSha1Error, match="not an outstanding slot"):
            rx.release(a)
        rx.release(b)
        assert rx.poll() == [] and rx.drain() == []
    finally:
        rx.close()


def test_reference_fixture_chunks_at_the_default_stride(bt, oracle):
    """Every chunk of tests/golden/C.tar.xz received as 1484-byte payloads at
    the default 64 KiB stride, against the digests the reference's make-chunks
    wrote (tests/golden/ref_C.chunks); one corrupted delivery must fail."""
    img = c_tar_bytes()
    ref = [bytes.fromhex(l.split()[1]) for l in open(os.path.join(GOLDEN, "ref_C.chunks")).read().splitlines()[2:]]
    n = len(ref)
    assert n == 4 and len(img) == n * bt.CHUNK
    rx = bt.Receiver(nslots=4)
    try:
        got = []
        for k in range(n):
            rx.receive(img[k * bt.CHUNK:(k + 1) * bt.CHUNK], ref[k], k)
            got += rx.poll()
        bad = bytearray(img[:bt.CHUNK])
        bad[400000] ^= 1
        got += rx.drain()
        rx.receive(bytes(bad), ref[0], 99)
        got += rx.drain()
        assert sorted(got) == [(k, True, ref[k]) for k in range(n)] + [(99, False, oracle.sha1(bytes(bad)))]
        launches, nadv, nbytes = rc.stride_rule(bt.CHUNK, 0)
        s = rx.stats()
        assert s["advance_launches"] == (n + 1) * nadv and s["advanced_bytes"] == (n + 1) * nbytes
        assert nbytes >= bt.CHUNK - 65536 - rc.PIECE
    finally:
        rx.close()
