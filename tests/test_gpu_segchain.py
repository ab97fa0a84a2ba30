"""GPU: the chain form of whole segment lists (k_sha1_gather_chain: one
two-wave workgroup per message that builds its position table window by
window in LDS), through bt_sha1_segchain_dev and, behind
bt_sha1_set_segchain_batch, through bt_sha1_gather_dev /
bt_sha1_gather_verify_dev and a gather verifier.  Everything against hashlib
or the oracle (segchain_cases).

1. Padding edges: every tail length around the 0x80 mark and the bit count,
   the two empty messages, shared and overlapping segments, one 512 KiB chunk
   as 354 datagrams; digests only, verdicts only, both; one planted bit.
2. Window edges: 1023 .. 3000 non-empty segments of 1 .. 3 bytes, with and
   without 1500 empty ones between them.
3. Piece edges: piece_bytes 64, 128, 4096 on 37 segments; 64 on 2500.
4. Routing by the knob, results identical with it off.
5. Device and pinned host memory, n = 65 with empties, guard bytes.
6. The gather verifier with the knob on.
7. verify-stream -G -c.
"""
import contextlib
import ctypes
import hashlib
import random

import numpy as np
import pytest

import gather_cases as gc
import segchain_cases as sc
import test_gpu_launch_forms as lf
from conftest import load_btsha1

pytestmark = pytest.mark.gpu
AUTO = 2**64 - 1


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


@contextlib.contextmanager
def knob(bt, value):
    prev = bt.set_segchain_batch(value)
    try:
        yield
    finally:
        bt.set_segchain_batch(prev)


def dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def pinned(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).pin_memory()


class Tables:
    def __init__(self, torch, batch, put=dev):
        self.keep = [put(torch, batch[k]) for k in ("blob", "segs", "first", "count")]

    def args(self):
        return tuple(t.data_ptr() for t in self.keep)


def plant(want, i, byte, bit):
    """Expected hashes with one bit of message i's wrong, and the verdicts that must follow."""
    exp = bytearray(want)
    exp[20 * i + byte] ^= 1 << bit
    return bytes(exp), bytes(0 if k == i else 1 for k in range(len(want) // 20))


def chain(bt, torch, t, n, want, label, outputs="both", planted=None, piece=0, shift=1):
    """One launch of the chain form over the first n messages: digests only,
    verdicts only (no digest buffer) or both, every output between guards at
    an odd address; with verdicts, one bit of message `planted[0]` is wrong."""
    dig, ok = lf.Guarded(torch, n, 20, shift), lf.Guarded(torch, n, 1, shift)
    exp = want_ok = None
    if outputs != "digests":
        i, byte, bit = planted
        bad, want_ok = plant(want[:20 * n], i, byte, bit)
        exp = lf.Guarded(torch, n, 20, 3)
        exp.buf[exp.lead:exp.lead + exp.used] = dev(torch, np.frombuffer(bad, dtype=np.uint8))
    bt.segchain_dev(*t.args(), n, exp.ptr if exp else None, ok.ptr if exp else None,
                    dig.ptr if outputs != "verdicts" else None, piece)
    lf.settle(torch, label, [("digests", dig, want[:20 * n] if outputs != "verdicts" else None),
                             ("ok", ok, want_ok)])


# ---------------------------------------------------------------------------
# 1. Padding edges
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def padding(torch, oracle):
    b = sc.padding_batch(oracle)
    return b, Tables(torch, b)


@pytest.mark.parametrize("outputs,planted", [("digests", None), ("verdicts", (0, 0, 7)), ("verdicts", (7, 19, 0)),
                                             ("both", (1, 11, 3)), ("both", (15, 4, 5))])
def test_padding_edges(bt, torch, padding, outputs, planted):
    """The planted bit sits in an empty message (0: nothing listed, 1: three
    empty segments), in a short one, or in the 354-datagram chunk (15)."""
    b, t = padding
    assert b["n"] == 16 and [sum(sc.lengths(b, i)) for i in range(2, 12)] == list(sc.PAD_TOTALS)
    chain(bt, torch, t, b["n"], b["want"], ("padding", outputs, planted), outputs, planted)


def test_no_messages_is_no_work(bt, torch, padding):
    _, t = padding
    dig, ok = lf.Guarded(torch, 4, 20), lf.Guarded(torch, 4, 1)
    bt.segchain_dev(*t.args(), 0, dig.ptr, ok.ptr, dig.ptr)
    lf.settle(torch, "n == 0", [("digests", dig, None), ("ok", ok, None)])


# ---------------------------------------------------------------------------
# 2. Window edges
# ---------------------------------------------------------------------------
def test_window_edges(bt, torch):
    b = sc.window_batch()
    plans = [sc.plan(sc.lengths(b, i)) for i in range(b["n"])]
    # one window up to 1024 non-empty segments, two for 1025; a slide keeps the tail of the block it cut, so
    # 2048 take three.  Empty segments take no room in a window, but one behind its last entry hides the list's end.
    assert [len(p) for p in plans[:3]] == [1, 1, 2] and all(len(p) >= 3 for p in plans[3:6])
    assert all(len(q) >= len(p) for p, q in zip(plans[:6], plans[6:12])) and len(plans[12]) == 1
    assert any(p[1][0] for p in plans[2:6])  # a window that starts inside a segment
    t = Tables(torch, b)
    chain(bt, torch, t, b["n"], b["want"], "windows", "both", (4, 2, 6))


# ---------------------------------------------------------------------------
# 3. Piece edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("piece,n", [(64, 2), (128, 1), (4096, 1)])
def test_piece_edges(bt, torch, piece, n):
    """piece_bytes 64: every block is a body call of its own, and on the
    2500-segment message windows and pieces interleave."""
    b = sc.piece_batch()
    p = sc.plan(sc.lengths(b, 0), piece)
    calls = -(-10240 // piece)  # advances of one piece each; the last piece, whole or not, finishes
    assert len(p) == calls and p[-1][1:] == (10240 - (calls - 1) * piece, 10240)
    assert [f for f, _, _ in p[:3]] != [0, 0, 0]  # pieces start inside segments
    if n == 2:
        q = sc.plan(sc.lengths(b, 1), 64)
        assert len(q) > 64 and len({f for f, _, _ in q}) > 1
    chain(bt, torch, Tables(torch, b), n, b["want"], ("piece", piece), "both", (n - 1, 9, 1), piece=piece)


# ---------------------------------------------------------------------------
# 4. Routing
# ---------------------------------------------------------------------------
def routed(bt, torch, t, n, want, label):
    bad, want_ok = plant(want[:20 * n], n - 1, 13, 2)
    exp = dev(torch, np.frombuffer(bad, dtype=np.uint8))
    d1, d2, ok = lf.Guarded(torch, n, 20, 1), lf.Guarded(torch, n, 20, 1), lf.Guarded(torch, n, 1, 1)
    bt.gather_dev(*t.args(), n, d1.ptr)
    bt.gather_verify_dev(*t.args(), n, exp.data_ptr(), ok.ptr, d2.ptr)
    return lf.settle(torch, label, [("gather_dev", d1, want[:20 * n]), ("gather_verify_dev", d2, want[:20 * n]),
                                    ("ok", ok, want_ok)])


def test_routing_by_the_knob(bt, torch, oracle):
    b = gc.datagram_batch(oracle)  # the first four: 512 KiB chunks as 354 datagrams
    t = Tables(torch, b)
    assert bt.set_segchain_batch(0) == 0  # off by default
    assert [bt.seglist_kernel_name(n) for n in (1, 3, 4)] == ["k_sha1_gather"] * 3
    off = {n: routed(bt, torch, t, n, b["want"], ("off", n)) for n in (1, 3, 4)}
    with knob(bt, 3):
        assert [bt.seglist_kernel_name(n) for n in (1, 3, 4)] == ["k_sha1_gather_chain"] * 2 + ["k_sha1_gather"]
        for n in (1, 3, 4):
            on = routed(bt, torch, t, n, b["want"], ("on", n))
            assert all(np.array_equal(on[k], off[n][k]) for k in on)
    assert bt.set_segchain_batch(0) == 0


# ---------------------------------------------------------------------------
# 5. Memory
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "pinned"])
def test_mixed_lengths_from_device_and_pinned_memory(bt, torch, where):
    b = sc.mixed_batch(65)
    assert sum(1 for i in range(65) if sum(sc.lengths(b, i)) == 0) == 22
    t = Tables(torch, b, dev if where == "device" else pinned)
    chain(bt, torch, t, 65, b["want"], ("mixed", where), "both", (64, 0, 0), shift=3)
    chain(bt, torch, t, 64, b["want"], ("mixed, n = 64", where), "digests")  # message 64's entries stay as they were


# ---------------------------------------------------------------------------
# 6. The gather verifier
# ---------------------------------------------------------------------------
def test_gather_verifier_with_the_knob_on(bt, oracle):
    rng = random.Random(0x5E6C7)
    slot_len = 355 * gc.DGRAM  # 354 datagrams and one duplicate
    with knob(bt, AUTO):
        assert bt.seglist_kernel_name(3) == "k_sha1_gather_chain"
        v = bt.Verifier(chunk_len=slot_len, batch=4, nstreams=2, gather=True, max_segs=400)
        try:
            want = []
            for k in range(3):
                data = bytes(oracle.fill_synthetic(gc.CHUNK, 300 + k, sc.SEED))
                pays = [data[i:i + gc.PAYLOAD] for i in range(0, len(data), gc.PAYLOAD)]
                order = rng.sample(range(len(pays)), len(pays))
                slot, where = v.slot(), {}
                for arrival, seq in enumerate(order + [order[k]]):  # one comes again; the copy is not listed
                    pkt = seq.to_bytes(4, "little") + bytes(12) + pays[seq]
                    ctypes.memmove(slot + arrival * gc.DGRAM, pkt, len(pkt))
                    where.setdefault(seq, arrival * gc.DGRAM + gc.HEADER)
                segs = [(where[s], len(pays[s])) for s in range(len(pays))]
                assert len(segs) == 354
                dg = oracle.sha1(data)
                assert dg == hashlib.sha1(data).digest()
                good = k != 1
                v.commit_gather(slot, segs, dg if good else dg[:5] + bytes([dg[5] ^ 0x10]) + dg[6:], 50 + k)
                want.append((50 + k, good, dg))
            got = v.drain()
            assert sorted(got) == want and v.pending() == 0
            pitch = (slot_len + 15) // 16 * 16
            assert v.gather_stats() == {"gather_batches": 1, "gather_chunks": 3, "segments": 3 * 354,
                                        "payload_bytes": 3 * gc.CHUNK, "copied_bytes": 3 * pitch}
            assert v.stats() == {"batches": 1, "ragged_batches": 0, "chunks": 3, "short_chunks": 0, "released": 0}
        finally:
            v.close()


# ---------------------------------------------------------------------------
# 7. verify-stream -G -c
# ---------------------------------------------------------------------------
def test_verify_stream_switch(tmp_path):
    """-G -c: the gather verifier's batches of two chunks go through the chain
    form; same verdicts and counts as -G alone, and the summary says so."""
    import json
    import os
    import subprocess
    from conftest import PKG
    exe = os.path.join(PKG, "bin", "verify-stream")
    data = random.Random(0x7A12).randbytes(3 * gc.CHUNK + 1000)
    img, ck = tmp_path / "tail.bin", tmp_path / "tail.chunks"
    img.write_bytes(data)
    ck.write_text("".join(f"{i} {hashlib.sha1(data[i * gc.CHUNK:(i + 1) * gc.CHUNK]).hexdigest()}\n" for i in range(4)))
    out = {}
    for name, args in (("lane", ["-G"]), ("chain", ["-G", "-c"]), ("chain, one bad", ["-G", "-c", "-x"])):
        r = subprocess.run([exe, *args, "-b", "2", str(img), str(ck)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    assert "segchain" not in out["lane"] and out["chain"]["segchain"] is True
    assert list(out["chain"])[:-1] == list(out["lane"])
    for k in ("chunks", "ok", "failed", "segments", "hashed_bytes", "wire_bytes", "mode"):
        assert out["chain"][k] == out["lane"][k], k
    assert (out["chain"]["ok"], out["chain"]["failed"]) == (4, 0)
    assert (out["chain, one bad"]["ok"], out["chain, one bad"]["failed"]) == (3, 1)
