#!/usr/bin/env python3
"""tools/latency_bench.py -- latency of the single-message and ragged paths.

The hot kernel is throughput-shaped (131072 chunks in flight).  The drop-in
callers that keep the reference's synchronous contract pay a chunk's serial
chain instead: util.c:311 calls shahash once per received chunk, and
make_chunks hashes its short last chunk alone (chunk.c:20-21).  This prints
one JSON line per measurement (median of --reps):

  shahash_512k      shahash() of one 512 KiB host buffer, call to return
  shahash_<n>B      shahash() of a short message: the fixed cost of a drop-in call
  ragged_1x512k     bt_sha1_ragged_dev over one device-resident 512 KiB message
  ragged_1x512k_u   the same message at an odd byte offset (unaligned loads)
  ragged_4096       4096 device-resident messages of 480-544 KiB at 16-byte
                    aligned offsets (GiB/s of message bytes)
  ragged_4096_u     the same lengths at arbitrary byte offsets
  update_1484       SHA1Update of one 512 KiB chunk fed as 1484-byte payloads
                    (save_data_packet's granule, util.c:275) + SHA1Final
  batch_<n>_<mode>  n device-resident 512 KiB chunks through the hot kernel
                    (fixed) or the two-wave latency kernel (lat), kernel time
  verifier_b1       bt_sha1_verifier with batch 1: submit -> verdict
  receiver_commit_<stride>   bt_sha1_receiver: one 512 KiB chunk delivered in
                    1484-byte payloads with advance after each, every earlier
                    launch finished before the commit (as at network speed):
                    commit -> verdict.  Strides: default (64 KiB), 4096 and
                    never (UINT32_MAX: the whole chain at commit)
  receiver_first_byte_<stride>  the same delivery fed back to back with no
                    waiting: first byte -> verdict (what the extra launches
                    cost when the data is already there)
  finish_gather_intake_512k, finish_intake_512k_same_session, ratio_gather_over_contiguous
                         one finishing entry over a 512 KiB chunk held as 354
                         datagrams (k_sha1_gather_resume_table, kick -> sync,
                         wall) against k_sha1_resume_table over the same bytes
                         contiguous, in this process; their ratio
  commit_gather_intake_default, commit_intake_default_same_session,
  verdict_gather_verifier_lone_chunk
                         commit -> verdict of a chunk delivered as datagrams at
                         network pace at the default stride, the assembled-slot
                         intake's, and the gather verifier's flush -> verdict
                         for a lone chunk (--only gather runs just these)
  resume_1x512k_<where>  one finishing launch of bt_sha1_resume_dev over a whole
                    512 KiB message from the IV, kernel time: the message in
                    device memory (dev) or read in place from pinned host
                    memory (pinned), beside shahash_512k (k_sha1_chain on
                    pinned host memory) in the same process
--only receiver runs just the receiver rows, verifier_b1 and the resume rows
(one process, so the rows compare on one box).
Digests are checked against the oracle (hashlib is not used).
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "bittorrent-with-congestion-control_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

CHUNK = 512 * 1024


def emit(name, samples_s, extra=None):
    med = statistics.median(samples_s)
    d = {"case": name, "median_ms": round(med * 1e3, 4), "min_ms": round(min(samples_s) * 1e3, 4),
         "reps": len(samples_s)}
    d.update(extra or {})
    print(json.dumps(d), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", choices=["all", "receiver", "gather"], default="all")
    args = ap.parse_args()
    import numpy as np
    import torch
    import btsha1 as bt
    import py_oracle as orc

    rng = np.random.default_rng(7)
    msg = bytes(orc.fill_synthetic(CHUNK, 0, orc.SEED_SYNTH))
    want = orc.sha1(msg)
    if args.only == "gather":
        assert torch.cuda.is_available()
        torch.zeros(1, device="cuda")  # torch's runtime first
        gather_rows(bt, torch, msg, want, max(args.reps, 50))
        return
    if args.only == "receiver":
        assert torch.cuda.is_available()
        torch.zeros(1, device="cuda")  # torch's runtime first
        receiver_rows(bt, torch, msg, want, max(args.reps, 50))
        verifier_row(bt, msg, want, max(args.reps, 50))
        resume_rows(bt, torch, msg, want, max(args.reps, 50))
        return

    # shahash: host buffer in, 20 bytes out, synchronous (chunk.c:33-49).
    assert bt.shahash(msg) == want
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        got = bt.shahash(msg)
        ts.append(time.perf_counter() - t0)
    assert got == want
    emit("shahash_512k", ts)
    # Fixed cost of one drop-in call: short messages (one launch of the chain
    # kernel on pinned host memory + the spin on its completion word).
    for ln in (0, 55, 1484, 16384):
        m = msg[:ln]
        assert bt.shahash(m) == orc.sha1(m)
        ts = []
        for _ in range(200):
            t0 = time.perf_counter()
            bt.shahash(m)
            ts.append(time.perf_counter() - t0)
        emit(f"shahash_{ln}B", ts)

    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    dev = torch.empty(CHUNK + 4096, dtype=torch.uint8, device="cuda")
    out = torch.zeros(20 * 4096, dtype=torch.uint8, device="cuda")

    def ragged(base, offs, lens):
        o = torch.tensor(offs, dtype=torch.int64, device="cuda")
        ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
        res = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            bt.ragged_dev(base, o.data_ptr(), ln.data_ptr(), len(offs), out.data_ptr(), s.cuda_stream)
            b.record(s)
            torch.cuda.synchronize()
            res.append(a.elapsed_time(b) * 1e-3)
        return res[1:]

    prev_chain = bt.set_chain_batch(0)
    for kname, thr in (("k_sha1_ragged", 0), ("k_sha1_chain", 1 << 62)):
        bt.set_chain_batch(thr)
        for name, off in (("ragged_1x512k", 0), ("ragged_1x512k_u", 3)):
            dev[off:off + CHUNK].copy_(torch.frombuffer(bytearray(msg), dtype=torch.uint8))
            ts = ragged(dev.data_ptr(), [off], [CHUNK])
            assert bytes(out[:20].cpu().numpy().tobytes()) == want, name
            emit(name + ("_chain" if thr else ""), ts, {"kernel": kname})
    bt.set_chain_batch(0)

    n = 4096
    lens = [int(x) for x in rng.integers(480 * 1024, 544 * 1024, n)]
    prev_lat = bt.set_latency_batch(2**64 - 1)
    for name, aligned, lat in (("ragged_4096", True, 0), ("ragged_4096_u", False, 0),
                               ("ragged_4096_latr", True, 2**64 - 1), ("ragged_4096_u_latr", False, 2**64 - 1)):
        bt.set_latency_batch(lat)
        offs, pos = [], 0
        for ln in lens:
            pos += int(rng.integers(0, 16)) if not aligned else 0
            offs.append(pos)
            pos += ln
            pos = (pos + 15) & ~15 if aligned else pos
        total = pos + 64
        big = torch.empty(total, dtype=torch.uint8, device="cuda")
        bt.fill_synthetic(big.data_ptr(), total, 12345, orc.SEED_SYNTH, s.cuda_stream)
        torch.cuda.synchronize()
        ts = ragged(big.data_ptr(), offs, lens)
        host = big.cpu().numpy()
        for i in list(range(0, n, 511)) + [n - 1]:
            assert bytes(out[20 * i:20 * i + 20].cpu().numpy().tobytes()) == \
                orc.sha1(host[offs[i]:offs[i] + lens[i]].tobytes()), (name, i)
        med = statistics.median(ts)
        emit(name, ts, {"kernel": "k_sha1_lat_ragged" if lat else "k_sha1_ragged", "messages": n,
                        "GiB_per_s": round(sum(lens) / med / 2**30, 2)})
        del big
    bt.set_latency_batch(prev_lat)

    # Streaming API at the peer's packet granule.
    ts = []
    for _ in range(max(1, args.reps // 3)):
        t0 = time.perf_counter()
        h = bt.Sha1()
        for o in range(0, CHUNK, 1484):
            h.update(msg[o:o + 1484])
        got = h.final()
        ts.append(time.perf_counter() - t0)
    assert got == want
    emit("update_1484", ts)

    # Device-resident batches of n 512 KiB chunks: the two-wave latency kernel
    # (k_sha1_lat) against the hot kernel (k_sha1_fixed), kernel time only.
    nmax = 65536
    big = torch.empty(nmax * CHUNK, dtype=torch.uint8, device="cuda")
    bt.fill_synthetic(big.data_ptr(), nmax * CHUNK, 0, orc.SEED_SYNTH, s.cuda_stream)
    dig = torch.zeros(20 * nmax, dtype=torch.uint8, device="cuda")
    golden = {}
    gpath = os.path.join(REPO, "tests", "golden", "synth4096.txt")
    for line in open(gpath):
        if not line.startswith("#"):
            i, h = line.split()
            golden[int(i)] = h
    prev = bt.set_latency_batch(0)
    prev_chain_fixed = bt.set_chain_batch(0)
    for n in (1, 64, 256, 512, 1024, 2048, 4096, 16384, 24576, 32768, 65536):
        for mode, thr, cthr in (("fixed", 0, 0), ("lat", 1 << 62, 0), ("chainfixed", 1 << 62, 1 << 62)):
            if mode == "chainfixed" and n > 4096:
                continue
            bt.set_latency_batch(thr)
            bt.set_chain_batch(cthr)
            res = []
            for _ in range(max(3, args.reps // 2) + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                bt.chunks_dev(big.data_ptr(), n, CHUNK, CHUNK, dig.data_ptr(), s.cuda_stream)
                b.record(s)
                torch.cuda.synchronize()
                res.append(a.elapsed_time(b) * 1e-3)
            raw = dig[:20 * min(n, 4096)].cpu().numpy().tobytes()
            assert all(raw[20 * i:20 * i + 20].hex() == golden[i] for i in range(min(n, 4096))), (mode, n)
            med = statistics.median(res[1:])
            emit(f"batch_{n}_{mode}", res[1:], {"chunks": n, "GiB_per_s": round(n * CHUNK / med / 2**30, 2)})
    bt.set_latency_batch(prev)
    bt.set_chain_batch(prev_chain_fixed)
    # The same chunks as ragged messages through the chain kernel (one
    # two-wave workgroup per chunk).
    bt.set_chain_batch(1 << 62)
    for n in (1, 64, 256):
        o = torch.arange(n, dtype=torch.int64, device="cuda") * CHUNK
        ln = torch.full((n,), CHUNK, dtype=torch.int32, device="cuda")
        res = []
        for _ in range(max(3, args.reps // 2) + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            bt.ragged_dev(big.data_ptr(), o.data_ptr(), ln.data_ptr(), n, dig.data_ptr(), s.cuda_stream)
            b.record(s)
            torch.cuda.synchronize()
            res.append(a.elapsed_time(b) * 1e-3)
        raw = dig[:20 * n].cpu().numpy().tobytes()
        assert all(raw[20 * i:20 * i + 20].hex() == golden[i] for i in range(n)), ("chain", n)
        med = statistics.median(res[1:])
        emit(f"batch_{n}_chain", res[1:], {"chunks": n, "GiB_per_s": round(n * CHUNK / med / 2**30, 2)})
    bt.set_chain_batch(prev_chain)
    del big

    verifier_row(bt, msg, want, args.reps)
    receiver_rows(bt, torch, msg, want, max(args.reps, 50))


def verifier_row(bt, msg, want, reps):
    v = bt.Verifier(batch=1, nstreams=2)
    ts = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        v.submit(msg, want, tag=i)
        r = v.drain()
        ts.append(time.perf_counter() - t0)
        assert r == [(i, True, want)], r
    v.close()
    emit("verifier_b1", ts[1:])


def resume_rows(bt, torch, msg, want, reps):
    host = torch.frombuffer(bytearray(msg), dtype=torch.uint8)
    o = torch.zeros(1, dtype=torch.int64, device="cuda")
    ln = torch.full((1,), CHUNK, dtype=torch.int32, device="cuda")
    tt = torch.full((1,), CHUNK, dtype=torch.int64, device="cuda")
    st = torch.zeros(5, dtype=torch.int32, device="cuda")
    dig = torch.zeros(20, dtype=torch.uint8, device="cuda")
    bt.states_init_dev(st.data_ptr(), 1)
    for where, buf in (("dev", host.cuda()), ("pinned", host.pin_memory())):
        ts = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            bt.resume_dev(buf.data_ptr(), o.data_ptr(), ln.data_ptr(), tt.data_ptr(), 1, st.data_ptr(), dig.data_ptr())
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        assert dig.cpu().numpy().tobytes() == want, where
        emit(f"resume_1x512k_{where}", ts[1:], {"kernel": "k_sha1_resume"})
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        got = bt.shahash(msg)
        ts.append(time.perf_counter() - t0)
    assert got == want
    emit("shahash_512k", ts[1:], {"kernel": "k_sha1_chain"})


DGRAM, HEADER, PAYLOAD = 1500, 16, 1484


def gather_rows(bt, torch, msg, want, reps):
    """The chain-form gather kernel against its contiguous twin, in one process."""
    import ctypes
    nd = -(-CHUNK // PAYLOAD)
    pkts = [bytes(HEADER) + msg[k * PAYLOAD:(k + 1) * PAYLOAD] for k in range(nd)]
    segs = [(k * DGRAM + HEADER, len(pkts[k]) - HEADER) for k in range(nd)]
    src = (ctypes.c_uint8 * CHUNK).from_buffer_copy(msg)

    def land(p, k):
        ctypes.memmove(p + k * DGRAM, pkts[k], len(pkts[k]))

    def verdict(obj, tag):
        while True:
            got = obj.poll()
            if got:
                assert got == [(tag, True, want)], got
                return

    # (a) one finishing entry over the whole chunk, kick -> sync
    med = {}
    for name in ("gather_intake", "intake"):
        gather = name == "gather_intake"
        obj = bt.Intake(chunk_len=nd * DGRAM if gather else CHUNK, nslots=1, stride=bt.NEVER, gather=gather,
                        max_segs=nd if gather else 0)
        ts = []
        for i in range(reps + 1):
            p = obj.slot()
            if gather:
                for k in range(nd):
                    land(p, k)
                obj.append(p, segs)
                obj.commit_gather(p, want, i)
            else:
                ctypes.memmove(p, ctypes.addressof(src), CHUNK)
                obj.commit(p, want, i)
            t0 = time.perf_counter()
            assert obj.kick() == 1
            obj.sync()
            ts.append(time.perf_counter() - t0)
            assert obj.drain() == [(i, True, want)]
        obj.close()
        med[name] = statistics.median(ts[1:])
        emit(f"finish_{name}_512k" + ("" if gather else "_same_session"), ts[1:],
             {"kernel": "k_sha1_gather_resume_table" if gather else "k_sha1_resume_table", "clock": "wall",
              "datagrams": nd if gather else 0})
    print(json.dumps({"case": "ratio_gather_over_contiguous",
                      "ratio": round(med["gather_intake"] / med["intake"], 3)}), flush=True)

    # (b) commit -> verdict at network pace, default stride
    for name in ("gather_intake", "intake"):
        gather = name == "gather_intake"
        obj = bt.Intake(chunk_len=nd * DGRAM if gather else CHUNK, nslots=2, gather=gather, max_segs=nd if gather else 0)
        ts = []
        for i in range(reps + 1):
            p = obj.slot()
            for k in range(nd):
                if gather:
                    land(p, k)
                    obj.append(p, [segs[k]])
                else:
                    o = k * PAYLOAD
                    n = min(PAYLOAD, CHUNK - o)
                    ctypes.memmove(p + o, ctypes.addressof(src) + o, n)
                    obj.advance(p, o + n)
                assert obj.poll() == []
                obj.sync()  # the network's pace: a stride's launch ends long before the next stride has arrived
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if gather:
                obj.commit_gather(p, want, i)
            else:
                obj.commit(p, want, i)
            verdict(obj, i)
            ts.append(time.perf_counter() - t0)
        s = obj.stats()
        obj.close()
        emit(f"commit_{name}_default" + ("" if gather else "_same_session"), ts[1:],
             {"launches_per_chunk": s["launches"] // (reps + 1),
              "advanced_bytes_per_chunk": s["advanced_bytes"] // (reps + 1)})
    v = bt.Verifier(chunk_len=nd * DGRAM, batch=1, nstreams=2, gather=True, max_segs=nd)
    ts = []
    for i in range(reps + 1):
        p = v.slot()
        for k in range(nd):
            land(p, k)
        t0 = time.perf_counter()
        v.commit_gather(p, segs, want, i)
        v.flush()
        got = v.drain()
        ts.append(time.perf_counter() - t0)
        assert got == [(i, True, want)], got
    v.close()
    emit("verdict_gather_verifier_lone_chunk", ts[1:], {"kernel": "k_sha1_gather_verify"})


def receiver_rows(bt, torch, msg, want, reps):
    """The progressive receiver on one 512 KiB chunk in 1484-byte payloads
    (util.c:275), advance after each.  commit -> verdict with every earlier
    launch finished first (a device synchronise stands for the network's
    pace), then first byte -> verdict with the payloads fed back to back."""
    import ctypes
    src = (ctypes.c_uint8 * CHUNK).from_buffer_copy(msg)
    addr = ctypes.addressof(src)
    piece = 1484

    def deliver(rx, p):
        for o in range(0, CHUNK, piece):
            n = min(piece, CHUNK - o)
            ctypes.memmove(p + o, addr + o, n)
            rx.advance(p, o + n)

    def verdict(rx, tag):
        while True:
            r = rx.poll()
            if r:
                assert r == [(tag, True, want)], r
                return

    for name, stride in (("default", 0), ("4096", 4096), ("never", bt.NEVER)):
        rx = bt.Receiver(nslots=2, stride=stride)
        commit_ts, first_ts = [], []
        for i in range(reps + 1):  # the first repetition warms the kernel and the streams up
            p = rx.slot()
            deliver(rx, p)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rx.commit(p, want, i)
            verdict(rx, i)
            commit_ts.append(time.perf_counter() - t0)
        base = rx.stats()
        for i in range(reps + 1):
            p = rx.slot()
            t0 = time.perf_counter()
            deliver(rx, p)
            rx.commit(p, want, i)
            verdict(rx, i)
            first_ts.append(time.perf_counter() - t0)
        # the host's share of first byte -> verdict: the same payload copies and advance calls, nothing committed
        host_ts = []
        for i in range(5):
            p = rx.slot()
            t0 = time.perf_counter()
            deliver(rx, p)
            host_ts.append(time.perf_counter() - t0)
            rx.release(p)
        per_chunk = {"launches_per_chunk": base["launches"] // (reps + 1),
                     "advanced_bytes_per_chunk": base["advanced_bytes"] // (reps + 1)}
        rx.close()
        emit(f"receiver_commit_{name}", commit_ts[1:], per_chunk)
        emit(f"receiver_first_byte_{name}", first_ts[1:],
             dict(per_chunk, host_feed_ms=round(statistics.median(host_ts) * 1e3, 4)))


if __name__ == "__main__":
    main()
