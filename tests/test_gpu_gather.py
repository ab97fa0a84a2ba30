"""GPU: scatter-gather SHA-1 (bt_sha1_gather_dev / bt_sha1_gather_verify_dev,
k_sha1_gather / k_sha1_gather_verify) and the datagram-slot verifier.

1. One wave in which every lane straddles at another byte, beside the host
   walk's cases (gather_cases.straddle_batch), at n = 1, 63, 64, 65, 257, 320.
2. The same batch tiled past the threshold of the 256-thread form.
3. Whole 512 KiB chunks as 354 datagrams in shuffled arrival order.
4. The fused compare: every digest bit, odd addresses, no digest buffer.
5. One segment per message agrees with ragged_dev / ragged_verify_dev.
6. The gather verifier.
7. verify-stream -G (datagram slots) on the golden C.tar and on a file that
   ends in a short chunk.
"""
import ctypes
import hashlib
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import gather_cases as gc
import ragged_verify_cases as rv
import test_gpu_launch_forms as lf
import verdict_cases as vc
from conftest import GOLDEN, PKG, c_tar_bytes, load_btsha1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def bt(torch):
    m = load_btsha1()
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(torch, arr):
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()


class Tables:
    def __init__(self, torch, batch, first=None, count=None):
        self.blob = dev(torch, batch["blob"])
        self.segs = dev(torch, batch["segs"])
        self.first = dev(torch, batch["first"] if first is None else first)
        self.count = dev(torch, batch["count"] if count is None else count)

    def args(self):
        return self.blob.data_ptr(), self.segs.data_ptr(), self.first.data_ptr(), self.count.data_ptr()


@pytest.fixture(scope="module")
def straddle(torch):
    b = gc.straddle_batch()
    return b, Tables(torch, b)


# ---------------------------------------------------------------------------
# 1. One wave, every straddle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 320])
def test_gather_every_straddle_in_one_wave(bt, torch, straddle, n):
    b, t = straddle
    dig = lf.Guarded(torch, n, 20, 1)
    bt.gather_dev(*t.args(), n, dig.ptr)
    lf.settle(torch, ("gather_dev", n), [("digests", dig, b["want"][:20 * n])])


def test_gather_no_messages_touches_nothing(bt, torch, straddle):
    _, t = straddle
    dig, ok = lf.Guarded(torch, 4, 20), lf.Guarded(torch, 4, 1)
    bt.gather_dev(*t.args(), 0, dig.ptr)
    bt.gather_verify_dev(*t.args(), 0, t.blob.data_ptr(), ok.ptr, dig.ptr)
    lf.settle(torch, "n == 0", [("digests", dig, None), ("ok", ok, None)])


# ---------------------------------------------------------------------------
# 2. Both workgroup widths
# ---------------------------------------------------------------------------
def test_gather_256_thread_form(bt, torch, cus):
    b = gc.straddle_batch()
    n = cus * 256 + 1  # at least one wave per SIMD: btsha1_launch_gather's 256-thread workgroups
    reps = -(-n // b["n"])
    first, count = np.tile(b["first"], reps)[:n], np.tile(b["count"], reps)[:n]
    t = Tables(torch, b, first, count)
    dig = lf.Guarded(torch, n, 20, 1)
    bt.gather_dev(*t.args(), n, dig.ptr)
    lf.settle(torch, "256 threads", [("digests", dig, (b["want"] * reps)[:20 * n])])


def test_gather_verify_256_thread_form(bt, torch, cus):
    """k_sha1_gather_verify in 256-thread workgroups: verdicts and digests of
    lanes past 63 of a workgroup, the verdict batch planted on the last 168."""
    b = gc.straddle_batch()
    n = cus * 256 + 1
    reps = -(-n // b["n"])
    t = Tables(torch, b, np.tile(b["first"], reps)[:n], np.tile(b["count"], reps)[:n])
    want = (b["want"] * reps)[:20 * n]
    exp = dev(torch, vc.expectations(want))
    ok, dig = lf.Guarded(torch, n, 1, 1), lf.Guarded(torch, n, 20, 1)
    bt.gather_verify_dev(*t.args(), n, exp.data_ptr(), ok.ptr, dig.ptr)
    got = lf.settle(torch, "256 threads, verify", [("ok", ok, lf.WRITTEN), ("digests", dig, want)])
    assert not vc.problems(got["ok"]), vc.problems(got["ok"])


# ---------------------------------------------------------------------------
# 3. Datagram shape at full size
# ---------------------------------------------------------------------------
def test_gather_whole_chunks_from_datagrams(bt, torch, oracle):
    b = gc.datagram_batch(oracle)
    assert b["n"] == 64
    t = Tables(torch, b)
    dig, ok = lf.Guarded(torch, 64, 20, 1), lf.Guarded(torch, 64, 1, 1)
    bt.gather_dev(*t.args(), 64, dig.ptr)
    exp = dev(torch, np.frombuffer(b["want"], dtype=np.uint8))
    bt.gather_verify_dev(*t.args(), 64, exp.data_ptr(), ok.ptr)
    lf.settle(torch, "datagrams", [("digests", dig, b["want"]), ("ok", ok, bytes([1]) * 64)])


# ---------------------------------------------------------------------------
# 4. Fused compare
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_digests", [True, False])
def test_gather_verify_every_digest_bit(bt, torch, straddle, with_digests):
    b, t = straddle
    n = b["n"]
    for exact in (True, False):
        exp = lf.Guarded(torch, n, 20, 1)
        exp.buf[exp.lead:exp.lead + exp.used] = dev(torch, vc.expectations(b["want"], exact))
        ok, dig = lf.Guarded(torch, n, 1, 1), lf.Guarded(torch, n, 20, 3)
        bt.gather_verify_dev(*t.args(), n, exp.ptr, ok.ptr, dig.ptr if with_digests else None)
        got = lf.settle(torch, ("verify", exact, with_digests),
                        [("ok", ok, lf.WRITTEN), ("digests", dig, b["want"] if with_digests else None)])
        assert not vc.problems(got["ok"], exact), vc.problems(got["ok"], exact)


# ---------------------------------------------------------------------------
# 5. Agreement with the ragged kernels
# ---------------------------------------------------------------------------
def test_gather_of_single_segments_is_ragged(bt, torch, oracle):
    n = 300
    blob, offs, lens, want = rv.batch(oracle, n)
    d = lf.upload(torch, blob)
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    seg = np.zeros((n, 2), dtype=np.uint64)
    seg[:, 0], seg[:, 1] = offs, lens
    d_seg, d_first = dev(torch, seg), dev(torch, np.arange(n, dtype=np.uint64))
    d_count = dev(torch, np.ones(n, dtype=np.uint32))
    exp = dev(torch, vc.expectations(want))
    outs = [lf.Guarded(torch, n, e, 1) for e in (20, 20, 1, 1)]
    bt.ragged_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, outs[0].ptr)
    bt.gather_dev(d.data_ptr(), d_seg.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), n, outs[1].ptr)
    bt.ragged_verify_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, exp.data_ptr(), outs[2].ptr)
    bt.gather_verify_dev(d.data_ptr(), d_seg.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), n, exp.data_ptr(),
                         outs[3].ptr)
    got = lf.settle(torch, "agreement", [("ragged", outs[0], want), ("gather", outs[1], want),
                                         ("ragged ok", outs[2], lf.WRITTEN), ("gather ok", outs[3], lf.WRITTEN)])
    assert np.array_equal(got["ragged ok"], got["gather ok"]) and not vc.problems(got["gather ok"])


# ---------------------------------------------------------------------------
# 6. The gather verifier
# ---------------------------------------------------------------------------
SLOT = 5 * gc.DGRAM


def land(slot, payloads, order, dup=None):
    """Datagrams into the slot in `order` (sequence numbers; `dup`: one more
    copy of that one at the end); returns the segment list by sequence number."""
    where = {}
    for arrival, seq in enumerate(list(order) + ([dup] if dup is not None else [])):
        pkt = seq.to_bytes(4, "little") + bytes(12) + payloads[seq]
        ctypes.memmove(slot + arrival * gc.DGRAM, pkt, len(pkt))
        where.setdefault(seq, arrival * gc.DGRAM + gc.HEADER)
    return [(where[s], len(payloads[s])) for s in range(len(payloads))]


def test_gather_verifier(bt):
    rng = random.Random(0x6A7)
    v = bt.Verifier(chunk_len=SLOT, batch=8, nstreams=2, gather=True, max_segs=8)
    try:
        want, segments, payload = [], 0, 0
        for rnd in range(3):  # three batches through a ring of two
            slots = [v.slot() for _ in range(8)]
            assert [b - a for a, b in zip(slots, slots[1:])] == [(SLOT + 15) // 16 * 16] * 7
            plan = list(range(8))
            rng.shuffle(plan)  # settled in any order
            for k in plan:
                tag = 100 * rnd + k
                if k == 3:
                    v.release(slots[k])
                    continue
                if k == 5:  # a plain commit: the one-segment message (0, len)
                    data = rng.randbytes(777)
                    ctypes.memmove(slots[k], data, len(data))
                    v.commit(slots[k], hashlib.sha1(data).digest(), tag, len(data))
                    want.append((tag, True, hashlib.sha1(data).digest()))
                    segments, payload = segments + 1, payload + 777
                    continue
                pays = [rng.randbytes(gc.PAYLOAD) for _ in range(3)] + [rng.randbytes(gc.LAST_PAYLOAD)]
                segs = land(slots[k], pays, rng.sample(range(4), 4), dup=rng.randrange(4))
                if k == 6:  # an empty segment in the list
                    segs.insert(2, (SLOT, 0))
                if k == 1:  # refused, and the slot stays outstanding and committable
                    with pytest.raises(bt.BtSha1Error, match="segment 1 .* ends past the slot's 7500 bytes"):
                        v.commit_gather(slots[k], [segs[0], (SLOT - 10, 11)], bytes(20), tag)
                    with pytest.raises(bt.BtSha1Error, match="9 segments, gather verifier built for 8 per chunk"):
                        v.commit_gather(slots[k], [(0, 1)] * 9, bytes(20), tag)
                dg = hashlib.sha1(b"".join(pays)).digest()
                good = k != 2
                v.commit_gather(slots[k], segs, dg if good else dg[:7] + bytes([dg[7] ^ 0x40]) + dg[8:], tag)
                want.append((tag, good, dg))
                segments, payload = segments + len(segs), payload + sum(n for _, n in segs)
            assert v.stats()["batches"] == rnd + 1  # the eighth settled slot launched the batch
        got = v.drain()
        assert sorted(got) == sorted(want) and v.pending() == 0
        pitch = (SLOT + 15) // 16 * 16
        assert v.gather_stats() == {"gather_batches": 3, "gather_chunks": 21, "segments": segments,
                                    "payload_bytes": payload, "copied_bytes": 3 * 8 * pitch}
        assert v.stats() == {"batches": 3, "ragged_batches": 0, "chunks": 21, "short_chunks": 0, "released": 3}
        for bad_len in (0, SLOT + 1):
            with pytest.raises(bt.BtSha1Error, match=f"chunk of {bad_len} bytes, gather verifier's slots take 1 .. {SLOT}"):
                v.submit(b"x" * bad_len, bytes(20), 1)
        # a flushed batch of one, through submit
        v.submit(b"abc", hashlib.sha1(b"abc").digest(), 7)
        assert v.drain() == [(7, True, hashlib.sha1(b"abc").digest())]
        assert v.gather_stats()["copied_bytes"] == (3 * 8 + 1) * pitch
    finally:
        v.close()


@pytest.mark.parametrize("ragged", [False, True])
def test_other_verifiers_refuse_commit_gather_and_launch_as_before(bt, ragged):
    full = 65536
    v = bt.Verifier(chunk_len=full, batch=8, nstreams=2, ragged=ragged)
    try:
        s = v.slot()
        with pytest.raises(bt.BtSha1Error, match="commit_gather needs a verifier from bt_sha1_verifier_create_gather"):
            v.commit_gather(s, [(0, 16)], bytes(20), 1)
        data = bytes(range(256)) * (full // 256)
        ctypes.memmove(s, data, full)
        v.commit(s, hashlib.sha1(data).digest(), 5, full)  # the slot was left outstanding
        if ragged:
            v.submit(data[:100], hashlib.sha1(data[:100]).digest(), 6)
        got = v.drain()
        assert got[0] == (5, True, hashlib.sha1(data).digest()) and len(got) == 1 + ragged
        assert v.stats() == {"batches": 1, "ragged_batches": int(ragged), "chunks": 1 + ragged,
                             "short_chunks": int(ragged), "released": 0}
        assert v.gather_stats() == dict.fromkeys(("gather_batches", "gather_chunks", "segments", "payload_bytes",
                                                  "copied_bytes"), 0)
    finally:
        v.close()


# ---------------------------------------------------------------------------
# 7. verify-stream -G
# ---------------------------------------------------------------------------
EXE = os.path.join(PKG, "bin", "verify-stream")
OLD_KEYS = ["chunks", "ok", "failed", "seconds", "GiB_per_s", "batch", "streams", "poll_every", "verifiers", "devices",
            "receive_threads", "rounds", "warmup_rounds", "timed_chunks", "late_fills", "mode"]


def stream(args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    return r, json.loads(last), sorted(re.findall(r"^Hash: (\w{40})$", r.stdout, re.M))


@pytest.fixture(scope="module")
def stream_files(tmp_path_factory):
    """(file, chunks file, bytes) for the golden C.tar and for 3 x 512 KiB + 1000 bytes."""
    d = tmp_path_factory.mktemp("gather_stream")
    c = d / "C.tar"
    c.write_bytes(c_tar_bytes())
    data = random.Random(0x7A11).randbytes(3 * gc.CHUNK + 1000)
    t = d / "tail.bin"
    t.write_bytes(data)
    ck = d / "tail.chunks"
    ck.write_text("".join(f"{i} {hashlib.sha1(data[i * gc.CHUNK:(i + 1) * gc.CHUNK]).hexdigest()}\n" for i in range(4)))
    return {"C.tar": (str(c), os.path.join(GOLDEN, "C.tar.make-chunks.out"), c_tar_bytes()),
            "tail": (str(t), str(ck), data)}


@pytest.mark.parametrize("name", ["C.tar", "tail"])
@pytest.mark.parametrize("mode", [["-b", "2"], ["-b", "2", "-r", "3"], ["-b", "1", "-g", "2", "-t"]],
                         ids=["one round", "resident rounds", "g2t"])
def test_verify_stream_datagram_slots(stream_files, name, mode):
    path, ck, data = stream_files[name]
    lens = [len(data[i:i + gc.CHUNK]) for i in range(0, len(data), gc.CHUNK)]
    assert len(lens) == 4
    r, js, failed = stream(["-G", *mode, path, ck])
    rounds = 3 if "-r" in mode else 1
    timed = rounds - 1 if rounds > 1 else 1  # round 0 lands the datagrams, untimed when there are more
    assert r.returncode == 0 and not failed and "Verification failed" not in r.stdout
    assert (js["chunks"], js["ok"], js["failed"]) == (4 * rounds, 4 * rounds, 0)
    assert js["mode"] == "datagram slots" and js["timed_chunks"] == 4 * timed
    ndg = [-(-n // gc.PAYLOAD) for n in lens]
    assert js["segments"] == timed * sum(ndg)  # the duplicate of each chunk is not listed
    assert js["wire_bytes"] == timed * sum((k + 1) * gc.DGRAM for k in ndg)  # it is in the slot
    assert js["hashed_bytes"] == timed * len(data)
    assert list(js)[:len(OLD_KEYS)] == OLD_KEYS


@pytest.mark.parametrize("name", ["C.tar", "tail"])
def test_verify_stream_datagram_slots_fail_what_packetized_fails(stream_files, name):
    path, ck, data = stream_files[name]
    rp, jp, fp = stream(["-x", "-b", "2", path, ck])
    rg, jg, fg = stream(["-G", "-x", "-b", "2", path, ck])
    assert rp.returncode == rg.returncode == 0  # -x: failures are the point
    assert (jp["failed"], jg["failed"]) == (1, 1) and fp == fg and len(fp) == 1
    bad = bytearray(data[3 * gc.CHUNK:4 * gc.CHUNK])  # chunk k = 3 is the one with k % 7 == 3
    bad[3 % len(bad)] ^= 0x5A
    assert fg == [hashlib.sha1(bad).hexdigest()]


@pytest.mark.parametrize("mode", [[], ["-z", "-b", "2", "-r", "2"]], ids=["packetized", "zcopy"])
def test_verify_stream_other_modes_keep_their_summary(stream_files, mode):
    path, ck, _ = stream_files["tail"]
    r, js, failed = stream([*mode, path, ck])
    assert r.returncode == 0 and not failed
    assert list(js) == OLD_KEYS  # no segments, wire_bytes or hashed_bytes
    assert js["mode"] == ("zero-copy slots" if mode else "packetized memcpy (util.c:275)")
    assert re.search(r'"late_fills": \d+, "mode": "[^"]+"}$', r.stdout.strip())
    r2 = subprocess.run([EXE, "-z", "-G", path, ck], capture_output=True, text=True, timeout=60)
    assert r2.returncode == 255 and "take one" in r2.stderr
