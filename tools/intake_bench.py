#!/usr/bin/env python3
"""tools/intake_bench.py -- what bt_sha1_intake buys over bt_sha1_receiver.

One process, so the rows compare on one box.  One JSON line per row:

  feed_only_<n>      the feed loop alone: 512 KiB chunks over n slots, fed
                     round-robin in 64 KiB pieces with advance after each, at
                     stride NEVER and never committed (nothing is hashed): the
                     rate the Python loop itself can deliver
  sustained_receiver_64, sustained_intake_<n>
                     the same feed with hashing on (default stride), every
                     chunk committed when complete, one poll per turn: first
                     byte -> last verdict over --gib GiB, median / min / max of
                     --runs runs, GiB/s
  commit_receiver_default, commit_intake_default
                     one chunk at network pace in 1484-byte payloads (the
                     intake with one poll per payload), every earlier launch
                     finished before the commit: commit -> verdict.  The intake
                     row waits for each launch before the next payload, as a
                     network's pace would; commit_intake_unpaced_default feeds
                     the payloads back to back instead (the lone slot's first
                     launch then outlasts the whole feed, every later stride is
                     deferred, and the commit finds most of the chunk unhashed)
  finish_intake_512k, finish_receiver_512k, resume_1x512k_*, shahash_512k
                     one whole 512 KiB chain from the IV in one launch: the
                     table kernel's single finishing entry (kick -> sync, wall),
                     the receiver's single launch at stride NEVER (commit ->
                     drain, wall), k_sha1_resume (events) and shahash (wall)
--gather: the same rows with DATAGRAM slots (bt.Intake(gather=True)): every
64 KiB piece is landed as its 1500-byte datagrams (16-byte header, 1484-byte
payload) and appended; sustained_gather_intake_<n>, then latency_bench's
gather rows (one finishing entry over 354 datagrams against the contiguous
table kernel, commit -> verdict at the default stride).
Digests are checked against the oracle (hashlib is not used).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "bittorrent-with-congestion-control_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, HERE)

CHUNK = 512 * 1024
PIECE = 64 * 1024


def feed(obj, nslots, nchunks, addr, want, commit=True, copy=True):
    """Round-robin feed of nchunks chunks over nslots slots; returns seconds
    from the first byte to the last verdict (commit) or to the last byte.
    copy=False: obj.advance lands the bytes itself (DatagramFeed)."""
    todo, free, got = nchunks, nslots, 0
    active = []  # [slot, bytes delivered]
    tag = 0
    t0 = time.perf_counter()
    while got < nchunks:
        while todo and free:
            active.append([obj.slot(), 0])
            todo -= 1
            free -= 1
        still = []
        for a in active:
            p, o = a
            if copy:
                ctypes.memmove(p + o, addr + o, PIECE)
            a[1] = o + PIECE
            obj.advance(p, a[1])
            if a[1] < CHUNK:
                still.append(a)
            elif commit:
                obj.commit(p, want, tag)
                tag += 1
            else:
                obj.release(p)
                free += 1
                got += 1
        active = still
        if commit:
            for v in obj.poll():
                assert v[1] and v[2] == want, v
                got += 1
                free += 1
    return time.perf_counter() - t0


def spread(name, rates, extra=None):
    d = {"case": name, "GiB_per_s": round(statistics.median(rates), 3), "min": round(min(rates), 3),
         "max": round(max(rates), 3), "runs": len(rates)}
    d.update(extra or {})
    print(json.dumps(d), flush=True)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0, help="GiB per sustained run")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50, help="repetitions of the latency rows")
    ap.add_argument("--only", choices=["all", "latency"], default="all")
    ap.add_argument("--gather", action="store_true", help="datagram slots: the gather intake's rows")
    ap.add_argument("--receiver-gib", type=float, default=None,
                    help="GiB per receiver run (default: --gib); its rate does not depend on the length")
    args = ap.parse_args()
    import torch
    import btsha1 as bt
    import latency_bench as lb
    import py_oracle as orc

    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")  # torch's runtime first
    msg = bytes(orc.fill_synthetic(CHUNK, 0, orc.SEED_SYNTH))
    want = orc.sha1(msg)
    src = (ctypes.c_uint8 * CHUNK).from_buffer_copy(msg)
    addr = ctypes.addressof(src)
    nchunks = int(args.gib * 2**30) // CHUNK
    gib = nchunks * CHUNK / 2**30

    if args.gather:
        if args.only == "all":
            sustained_gather(bt, args, msg, want, nchunks, gib)
        lb.gather_rows(bt, torch, msg, want, args.reps)
        return
    if args.only == "all":
        sustained(bt, args, addr, want, nchunks, gib)
    latency(bt, lb, torch, args, addr, msg, want)


def sustained(bt, args, addr, want, nchunks, gib):
    for n in (64, 512):
        ix = bt.Intake(nslots=n, stride=bt.NEVER)
        rates = [gib / feed(ix, n, nchunks, addr, want, commit=False) for _ in range(3)]
        assert ix.stats()["launches"] == 0
        ix.close()
        spread(f"feed_only_{n}", rates, {"hashing": "off"})

    rows = {}
    rn = int((args.receiver_gib or args.gib) * 2**30) // CHUNK
    rx = bt.Receiver(nslots=64)
    feed(rx, 64, 128, addr, want)  # warm-up
    rows["receiver"] = spread("sustained_receiver_64",
                              [rn * CHUNK / 2**30 / feed(rx, 64, rn, addr, want) for _ in range(args.runs)],
                              {"GiB_per_run": rn * CHUNK / 2**30})
    rx.close()
    for n in (64, 256, 512):
        ix = bt.Intake(nslots=n)
        feed(ix, n, 2 * n, addr, want)  # warm-up
        before = ix.stats()
        rates = [gib / feed(ix, n, nchunks, addr, want) for _ in range(args.runs)]
        s = ix.stats()
        ix.close()
        rows[n] = spread(f"sustained_intake_{n}", rates,
                         {"GiB_per_run": gib, "max_entries": s["max_entries"],
                          "entries_per_launch": round((s["entries"] - before["entries"]) /
                                                      max(1, s["launches"] - before["launches"]), 1),
                          "deferred": s["deferred"] - before["deferred"]})
    r, i64 = rows["receiver"], rows[64]
    print(json.dumps({"case": "ratio_intake_64_over_receiver_64",
                      "ratio": round(i64["GiB_per_s"] / r["GiB_per_s"], 2),
                      "spreads_GiB_per_s": [round(r["max"] - r["min"], 3), round(i64["max"] - i64["min"], 3)],
                      "beats_by_more_than_both_spreads":
                          i64["GiB_per_s"] - r["GiB_per_s"] > (r["max"] - r["min"]) + (i64["max"] - i64["min"]),
                      "ratio_512_over_64": round(rows[512]["GiB_per_s"] / i64["GiB_per_s"], 2)}), flush=True)


class DatagramFeed:
    """feed()'s view of a gather intake: a 64 KiB piece is landed as the
    datagrams whose payloads end inside it, each appended as it lands."""
    DGRAM, HEADER, PAYLOAD = 1500, 16, 1484

    def __init__(self, ix, msg):
        self.ix = ix
        self.nd = -(-CHUNK // self.PAYLOAD)
        self.pkts = [bytes(self.HEADER) + msg[k * self.PAYLOAD:(k + 1) * self.PAYLOAD] for k in range(self.nd)]
        self.sent = {}

    def slot(self):
        p = self.ix.slot()
        self.sent[p] = 0
        return p

    def advance(self, p, filled):
        k = self.sent[p]
        while k < self.nd and (min((k + 1) * self.PAYLOAD, CHUNK) <= filled):
            ctypes.memmove(p + k * self.DGRAM, self.pkts[k], len(self.pkts[k]))
            self.ix.append(p, [(k * self.DGRAM + self.HEADER, len(self.pkts[k]) - self.HEADER)])
            k += 1
        self.sent[p] = k

    def commit(self, p, want, tag):
        self.ix.commit_gather(p, want, tag)

    def release(self, p):
        self.ix.release(p)

    def poll(self):
        return self.ix.poll()


def sustained_gather(bt, args, msg, want, nchunks, gib):
    nd = -(-CHUNK // DatagramFeed.PAYLOAD)
    for n in (64, 512):
        ix = bt.Intake(chunk_len=nd * DatagramFeed.DGRAM, nslots=n, gather=True, max_segs=nd)
        fd = DatagramFeed(ix, msg)
        feed(fd, n, 2 * n, 0, want, copy=False)  # warm-up
        before = ix.stats()
        rates = [gib / feed(fd, n, nchunks, 0, want, copy=False) for _ in range(args.runs)]
        s = ix.stats()
        ix.close()
        spread(f"sustained_gather_intake_{n}", rates,
               {"GiB_per_run": gib, "max_entries": s["max_entries"],
                "entries_per_launch": round((s["entries"] - before["entries"]) /
                                            max(1, s["launches"] - before["launches"]), 1),
                "deferred": s["deferred"] - before["deferred"]})


def latency(bt, lb, torch, args, addr, msg, want):
    # commit -> verdict at network pace
    def verdict(obj, tag):
        while True:
            got = obj.poll()
            if got:
                assert got == [(tag, True, want)], got
                return

    for name, make, paced in (("receiver", bt.Receiver, False), ("intake", bt.Intake, True),
                              ("intake_unpaced", bt.Intake, False)):
        obj = make(nslots=2)
        ts = []
        for i in range(args.reps + 1):
            p = obj.slot()
            for o in range(0, CHUNK, 1484):
                n = min(1484, CHUNK - o)
                ctypes.memmove(p + o, addr + o, n)
                obj.advance(p, o + n)
                if make is bt.Intake:
                    assert obj.poll() == []
                    if paced:  # the network's pace: a stride's launch ends long before the next stride has arrived
                        obj.sync()
            if make is bt.Intake:
                obj.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            obj.commit(p, want, i)
            verdict(obj, i)
            ts.append(time.perf_counter() - t0)
        s = obj.stats()
        obj.close()
        lb.emit(f"commit_{name}_default", ts[1:], {"launches_per_chunk": s["launches"] // (args.reps + 1),
                                                   "advanced_bytes_per_chunk": s["advanced_bytes"] // (args.reps + 1)})

    # one whole chain in one launch
    for name, obj in (("intake", bt.Intake(nslots=1, stride=bt.NEVER)), ("receiver", bt.Receiver(nslots=1, stride=bt.NEVER))):
        ts = []
        for i in range(args.reps + 1):
            p = obj.slot()
            ctypes.memmove(p, addr, CHUNK)
            if name == "intake":
                obj.commit(p, want, i)
                t0 = time.perf_counter()
                assert obj.kick() == 1
                obj.sync()
                ts.append(time.perf_counter() - t0)
                assert obj.drain() == [(i, True, want)]
            else:
                t0 = time.perf_counter()
                obj.commit(p, want, i)
                got = obj.drain()
                ts.append(time.perf_counter() - t0)
                assert got == [(i, True, want)]
        obj.close()
        lb.emit(f"finish_{name}_512k", ts[1:],
                {"kernel": "k_sha1_resume_table" if name == "intake" else "k_sha1_resume", "clock": "wall"})
    lb.resume_rows(bt, torch, msg, want, args.reps)


if __name__ == "__main__":
    main()
