#!/usr/bin/env python3
"""tools/gather_bench.py -- what hashing a chunk where its datagrams landed costs.

Device-resident: bt_sha1_gather_dev over n chunks of 512 KiB, each cut as 354
DATA datagrams of 1500 bytes (16-byte header, 1484 bytes of payload, the last
436), beside bt_sha1_ragged_dev over the same payload bytes laid out
contiguously, at the same n.  HIP events around each launch, 2 warm-ups, the
median of 5, and the ratio of the two.  The digests of both must be equal.
Prints one JSON line per n (64, 4096, 32768 by default), with the time per
64-byte block of one message (the serial chain every lane runs).  At the
largest n that leaves bt_sha1_ragged_dev on its loader / round-wave form, the
lane kernel k_sha1_ragged -- the kernel the gather kernel is modelled on -- is
timed too, with the latency batch set to 0 for those launches.

Host paths: verify-stream on ONE image (8 GiB by default) in a tmpfs file, in
one session, one receive thread: -G (datagram slots: table build + H2D of the
datagrams + gather hash + verdict), -z (payloads landed contiguously) and
packetized (util.c:275's 1484-byte memcpys); -G and -z time 4 rounds over the
resident slots after the landing round, packetized 2 rounds after 1 untimed.
Rates are over hashed (payload) bytes.
--lat: beside each n, bt_sha1_gather_dev with the segment-list latency knob on
(bt_sha1_set_seglist_latency_batch(auto): k_sha1_gather_lat), the launches
interleaved with the knob-off ones in the same session, digests equal.
--chain: a leg of its own, nothing else runs.  For n = 1, 4, 64 and 2, 3, 4, 8
x CUs chunks (or the N given) as 354 datagrams in a shuffled arrival order:
bt_sha1_gather_verify_dev with both segment-list knobs off (what is launched by
default), with the latency knob on, and with bt_sha1_set_segchain_batch(n)
(k_sha1_gather_chain, also past the 2 x CUs its auto setting stops at), beside
bt_sha1_ragged_verify_dev over the same bytes laid out contiguously; the four
alternate inside each of 7 repetitions, verdicts checked every time.
--pkts: a leg of its own, nothing else runs.  For n = 64, 4096, 32768 (or the
N given) chunks as 354 datagrams in a shuffled arrival order:
bt_sha1_pkts_verify_dev (k_sha1_pkts: one uint32 per datagram, no segment
list) beside bt_sha1_gather_verify_dev with both segment-list knobs off
(k_sha1_gather_verify, what the same slots launch without it) and
bt_sha1_ragged_verify_dev over the same bytes contiguous with the latency and
chain batches at 0 (the lane kernel k_sha1_ragged_verify); the three alternate
inside each of 7 repetitions, verdicts checked every time.
usage: gather_bench.py [--host-gib G] [--no-device] [--lat] [--chain] [--pkts] [N ...]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "bittorrent-with-congestion-control_amd"))

CHUNK, DGRAM, HEADER, PAYLOAD, LAST = 512 * 1024, 1500, 16, 1484, 436
NDG = 354
SLOT = NDG * DGRAM


def host_paths(torch, bt, gib):
    n = int(gib * 2**30) // CHUNK
    dev = torch.empty(n * CHUNK, dtype=torch.uint8, device="cuda")
    bt.fill_synthetic(dev.data_ptr(), n * CHUNK, 0, 0x0B175EED)
    dig = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
    bt.chunks_dev(dev.data_ptr(), n, CHUNK, CHUNK, dig.data_ptr())
    torch.cuda.synchronize()
    want = dig.cpu().numpy().tobytes()
    shm = "/dev/shm"
    if not os.path.isdir(shm) or shutil.disk_usage(shm).free < 2 * n * CHUNK:
        shm = tempfile.gettempdir()
    vs = os.path.join(HERE, "bittorrent-with-congestion-control_amd", "bin", "verify-stream")
    with tempfile.TemporaryDirectory(dir=shm) as d:
        img, lst = os.path.join(d, "img"), os.path.join(d, "img.chunks")
        dev.cpu().numpy().tofile(img)
        del dev
        torch.cuda.empty_cache()
        with open(lst, "w") as f:
            for i in range(n):
                f.write(f"{i} {want[20 * i:20 * i + 20].hex()}\n")
        ring = ["-b", str(n // 2), "-s", "2"]  # resident modes: every chunk keeps a slot
        rates = {}
        for name, args in (("datagram_slots", ["-G", *ring, "-r", "5"]), ("zero_copy", ["-z", *ring, "-r", "5"]),
                           ("packetized", ["-b", "1024", "-s", "2", "-r", "3", "-w", "1"])):
            r = subprocess.run([vs, *args, img, lst], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, (name, r.stdout[-1000:], r.stderr[-1000:])
            js = json.loads(r.stdout.strip().splitlines()[-1])
            assert js["failed"] == 0 and js["ok"] == js["chunks"], (name, js)
            rates[name] = js["GiB_per_s"]
            print(json.dumps({"host_path": name, "image_GiB": n * CHUNK / 2**30, **js}), flush=True)
        print(json.dumps({"host_paths": rates,
                          "datagram_over_zero_copy": round(rates["datagram_slots"] / rates["zero_copy"], 4),
                          "expected_1484_over_1500": round(PAYLOAD / DGRAM, 4),
                          "datagram_over_packetized": round(rates["datagram_slots"] / rates["packetized"], 3)}),
              flush=True)


def chain_leg(torch, bt, sizes, reps=7):
    """One JSON line per n: the same n chunks as 354 datagrams in a shuffled
    arrival order, verified (bt_sha1_gather_verify_dev) with the segment-list
    knobs off (k_sha1_gather_verify, what is launched by default), with the
    latency knob on (k_sha1_gather_lat) and with the chain knob on
    (k_sha1_gather_chain), beside the same bytes contiguous through
    bt_sha1_ragged_verify_dev.  The four launches alternate inside every
    repetition; 2 warm-ups, HIP events, the median of `reps`."""
    auto, cus = 2**64 - 1, torch.cuda.get_device_properties(0).multi_processor_count
    for n in sizes or [1, 4, 64, 2 * cus, 3 * cus, 4 * cus, 8 * cus]:
        rng = np.random.default_rng(0x5E6C + n)
        wire = torch.empty(n * SLOT + 16, dtype=torch.uint8, device="cuda")
        bt.fill_synthetic(wire.data_ptr(), (n * SLOT) & ~15, 0, 0x6A7E)
        where = np.stack([rng.permutation(NDG) for _ in range(n)]).astype(np.uint64)  # where[i, seq]: arrival place
        seg = np.zeros((n, NDG, 2), dtype=np.uint64)
        seg[:, :, 0] = np.arange(n, dtype=np.uint64)[:, None] * SLOT + where * DGRAM + HEADER
        seg[:, :, 1] = PAYLOAD
        seg[:, NDG - 1, 1] = LAST
        idx = torch.from_numpy(where.astype(np.int64)).cuda()
        dg = wire[:n * SLOT].view(n, NDG, DGRAM)
        by_seq = torch.gather(dg, 1, idx[:, :, None].expand(n, NDG, DGRAM))
        flat = torch.empty(n * CHUNK, dtype=torch.uint8, device="cuda")
        fv = flat.view(n, CHUNK)
        fv[:, :(NDG - 1) * PAYLOAD] = by_seq[:, :NDG - 1, HEADER:].reshape(n, -1)
        fv[:, (NDG - 1) * PAYLOAD:] = by_seq[:, NDG - 1, HEADER:HEADER + LAST]
        del by_seq, idx
        d_seg = torch.from_numpy(seg.view(np.uint8).reshape(-1)).cuda()
        d_first = torch.arange(n, dtype=torch.int64, device="cuda") * NDG
        d_count = torch.full((n,), NDG, dtype=torch.int32, device="cuda")
        d_off = torch.arange(n, dtype=torch.int64, device="cuda") * CHUNK
        d_len = torch.full((n,), CHUNK, dtype=torch.int32, device="cuda")
        exp = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
        bt.ragged_dev(flat.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, exp.data_ptr())
        torch.cuda.synchronize()
        exp[20 * (n - 1) + 7] ^= 4  # one chunk fails: a verdict of all ones proves nothing
        want = torch.ones(n, dtype=torch.uint8, device="cuda")
        want[n - 1] = 0
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")

        def seglist(chain, lat):
            def run():
                c, l = bt.set_segchain_batch(chain), bt.set_seglist_latency_batch(lat)
                try:
                    bt.gather_verify_dev(wire.data_ptr(), d_seg.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), n,
                                         exp.data_ptr(), ok.data_ptr())
                    return bt.seglist_kernel_name(n)
                finally:
                    bt.set_segchain_batch(c)
                    bt.set_seglist_latency_batch(l)
            return run

        def contiguous():
            bt.ragged_verify_dev(flat.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, exp.data_ptr(), ok.data_ptr())
            return "bt_sha1_ragged_verify_dev"

        legs = {"off": seglist(0, 0), "lat": seglist(0, auto), "chain": seglist(n, 0), "contiguous": contiguous}
        names, times = {}, {k: [] for k in legs}
        for rep in range(2 + reps):
            for k, fn in legs.items():
                ok.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                names[k] = fn()
                b.record()
                b.synchronize()
                assert torch.equal(ok, want), (n, k)
                if rep >= 2:
                    times[k].append(a.elapsed_time(b))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({"leg": "chain", "n": n, "cus": cus, "kernels": names,
                          "off_median_ms": round(med["off"], 4), "lat_median_ms": round(med["lat"], 4),
                          "chain_median_ms": round(med["chain"], 4), "contiguous_median_ms": round(med["contiguous"], 4),
                          "chain_over_off": round(med["chain"] / med["off"], 3),
                          "chain_over_lat": round(med["chain"] / med["lat"], 3),
                          "chain_over_contiguous": round(med["chain"] / med["contiguous"], 3),
                          "chain_us_per_block": round(med["chain"] * 1e3 / (CHUNK // 64 + 1), 4),
                          "ms": {k: [round(x, 4) for x in v] for k, v in times.items()},
                          "auto_would_route": n <= 2 * cus, "source_id": bt.source_id()}), flush=True)
        del wire, flat, dg, fv, d_seg


def pkts_leg(torch, bt, sizes, reps=7):
    """One JSON line per n; 2 warm-ups, HIP events, the median of `reps`."""
    for n in sizes or [64, 4096, 32768]:
        rng = np.random.default_rng(0x9C75 + n)
        wire = torch.empty(n * SLOT + 16, dtype=torch.uint8, device="cuda")
        bt.fill_synthetic(wire.data_ptr(), (n * SLOT) & ~15, 0, 0x6A7E)
        where = np.stack([rng.permutation(NDG) for _ in range(n)]).astype(np.uint64)  # where[i, seq]: arrival place
        seg = np.zeros((n, NDG, 2), dtype=np.uint64)
        seg[:, :, 0] = np.arange(n, dtype=np.uint64)[:, None] * SLOT + where * DGRAM + HEADER
        seg[:, :, 1] = PAYLOAD
        seg[:, NDG - 1, 1] = LAST
        idx = torch.from_numpy(where.astype(np.int64)).cuda()
        flat = torch.empty(n * CHUNK, dtype=torch.uint8, device="cuda")
        fv = flat.view(n, CHUNK)
        step = max(1, min(n, 2048))  # the reordered copy, a few chunks at a time
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            dg = wire[lo * SLOT:hi * SLOT].view(hi - lo, NDG, DGRAM)
            by_seq = torch.gather(dg, 1, idx[lo:hi, :, None].expand(hi - lo, NDG, DGRAM))
            fv[lo:hi, :(NDG - 1) * PAYLOAD] = by_seq[:, :NDG - 1, HEADER:].reshape(hi - lo, -1)
            fv[lo:hi, (NDG - 1) * PAYLOAD:] = by_seq[:, NDG - 1, HEADER:HEADER + LAST]
            del by_seq, dg
        del idx
        d_seg = torch.from_numpy(seg.view(np.uint8).reshape(-1)).cuda()
        d_first = torch.arange(n, dtype=torch.int64, device="cuda") * NDG
        d_count = torch.full((n,), NDG, dtype=torch.int32, device="cuda")
        d_order = torch.from_numpy(where.astype(np.uint32).view(np.int32).reshape(-1)).cuda()
        d_slot = torch.arange(n, dtype=torch.int64, device="cuda") * SLOT
        d_off = torch.arange(n, dtype=torch.int64, device="cuda") * CHUNK
        d_len = torch.full((n,), CHUNK, dtype=torch.int32, device="cuda")
        geom = bt.PktGeom(DGRAM, HEADER, PAYLOAD, NDG)
        exp = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
        bt.ragged_dev(flat.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, exp.data_ptr())
        torch.cuda.synchronize()
        exp[20 * (n - 1) + 7] ^= 4  # one chunk fails: a verdict of all ones proves nothing
        want = torch.ones(n, dtype=torch.uint8, device="cuda")
        want[n - 1] = 0
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")

        def pkts():
            bt.pkts_verify_dev(wire.data_ptr(), geom, d_slot.data_ptr(), d_len.data_ptr(), d_order.data_ptr(),
                               d_first.data_ptr(), n, exp.data_ptr(), ok.data_ptr())
            return "k_sha1_pkts"

        def gather():
            c, l = bt.set_segchain_batch(0), bt.set_seglist_latency_batch(0)
            try:
                bt.gather_verify_dev(wire.data_ptr(), d_seg.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), n,
                                     exp.data_ptr(), ok.data_ptr())
                return bt.seglist_kernel_name(n) + "_verify"
            finally:
                bt.set_segchain_batch(c)
                bt.set_seglist_latency_batch(l)

        def lanes():
            c, l = bt.set_chain_batch(0), bt.set_latency_batch(0)
            try:
                bt.ragged_verify_dev(flat.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, exp.data_ptr(),
                                     ok.data_ptr())
                return "k_sha1_ragged_verify"
            finally:
                bt.set_chain_batch(c)
                bt.set_latency_batch(l)

        legs = {"pkts": pkts, "gather": gather, "ragged": lanes}
        names, times = {}, {k: [] for k in legs}
        for rep in range(2 + reps):
            for k, fn in legs.items():
                ok.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                names[k] = fn()
                b.record()
                b.synchronize()
                assert torch.equal(ok, want), (n, k)
                if rep >= 2:
                    times[k].append(a.elapsed_time(b))
        med = {k: statistics.median(v) for k, v in times.items()}
        blocks = CHUNK // 64 + 1
        print(json.dumps({"leg": "pkts", "n": n, "kernels": names,
                          **{f"{k}_median_ms": round(v, 4) for k, v in med.items()},
                          **{f"{k}_us_per_block": round(v * 1e3 / blocks, 4) for k, v in med.items()},
                          "pkts_over_gather": round(med["pkts"] / med["gather"], 3),
                          "pkts_over_ragged": round(med["pkts"] / med["ragged"], 3),
                          "gather_over_ragged": round(med["gather"] / med["ragged"], 3),
                          "pkts_GiB_s": round(n * CHUNK / 2**30 / (med["pkts"] / 1e3), 2),
                          "ms": {k: [round(x, 4) for x in v] for k, v in times.items()},
                          "source_id": bt.source_id()}), flush=True)
        del wire, flat, fv, d_seg, d_order


def main():
    import torch
    import btsha1 as bt
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int)
    ap.add_argument("--host-gib", type=float, default=8.0)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--lat", action="store_true")
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("--pkts", action="store_true")
    a = ap.parse_args()
    sizes = a.sizes or [64, 4096, 32768]
    assert (NDG - 1) * PAYLOAD + LAST == CHUNK
    if a.chain:  # a leg of its own: the knobs off and on over the same batches, nothing else
        chain_leg(torch, bt, a.sizes)
        return
    if a.pkts:  # likewise
        pkts_leg(torch, bt, a.sizes)
        return
    if a.host_gib > 0:
        host_paths(torch, bt, a.host_gib)
    for n in [] if a.no_device else sizes:
        wire = torch.empty(n * SLOT + 16, dtype=torch.uint8, device="cuda")
        bt.fill_synthetic(wire.data_ptr(), (n * SLOT) & ~15, 0, 0x6A7E)
        dg = wire[:n * SLOT].view(n, NDG, DGRAM)
        flat = torch.empty(n * CHUNK, dtype=torch.uint8, device="cuda")
        fv = flat.view(n, CHUNK)
        fv[:, :(NDG - 1) * PAYLOAD] = dg[:, :NDG - 1, HEADER:].reshape(n, -1)
        fv[:, (NDG - 1) * PAYLOAD:] = dg[:, NDG - 1, HEADER:HEADER + LAST]
        seg = np.zeros((n, NDG, 2), dtype=np.uint64)
        seg[:, :, 0] = (np.arange(n, dtype=np.uint64)[:, None] * SLOT + np.arange(NDG, dtype=np.uint64)[None, :] * DGRAM
                        + HEADER)
        seg[:, :, 1] = PAYLOAD
        seg[:, NDG - 1, 1] = LAST
        d_seg = torch.from_numpy(seg.view(np.uint8).reshape(-1)).cuda()
        d_first = torch.arange(n, dtype=torch.int64, device="cuda") * NDG
        d_count = torch.full((n,), NDG, dtype=torch.int32, device="cuda")
        d_off = torch.arange(n, dtype=torch.int64, device="cuda") * CHUNK
        d_len = torch.full((n,), CHUNK, dtype=torch.int32, device="cuda")
        gd = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
        rd = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")

        def gather():
            bt.gather_dev(wire.data_ptr(), d_seg.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), n, gd.data_ptr())

        def ragged():
            bt.ragged_dev(flat.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, rd.data_ptr())

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        for _ in range(2):
            gather()
            ragged()
        torch.cuda.synchronize()
        assert torch.equal(gd, rd), n
        tg, tr = [], []
        for _ in range(5):
            tg.append(timed(gather))
            tr.append(timed(ragged))
        mg, mr = statistics.median(tg), statistics.median(tr)
        lanes = None
        if n > 2 * torch.cuda.get_device_properties(0).multi_processor_count:
            before = bt.set_latency_batch(0)  # ragged_dev then launches k_sha1_ragged
            try:
                for _ in range(2):
                    ragged()
                torch.cuda.synchronize()
                assert torch.equal(gd, rd), n
                lanes = statistics.median(timed(ragged) for _ in range(5))
            finally:
                bt.set_latency_batch(before)
        lat = {}
        if a.lat:
            def gather_lat():
                before = bt.set_seglist_latency_batch(2**64 - 1)
                try:
                    gather()
                finally:
                    bt.set_seglist_latency_batch(before)

            gd.zero_()
            for _ in range(2):
                gather_lat()
            torch.cuda.synchronize()
            assert torch.equal(gd, rd), n
            to, tl = [], []
            for _ in range(5):
                to.append(timed(gather))
                tl.append(timed(gather_lat))
            before = bt.set_seglist_latency_batch(2**64 - 1)
            name = bt.seglist_kernel_name(n)
            bt.set_seglist_latency_batch(before)
            mo, ml = statistics.median(to), statistics.median(tl)
            lat = {"knob_on_kernel": name, "knob_off_median_ms": round(mo, 4), "knob_on_median_ms": round(ml, 4),
                   "knob_on_over_off": round(ml / mo, 3), "knob_on_over_ragged": round(ml / mr, 3),
                   "knob_on_us_per_block": round(ml * 1e3 / (CHUNK // 64 + 1), 4),
                   "knob_off_ms": [round(x, 4) for x in to], "knob_on_ms": [round(x, 4) for x in tl]}
        blocks = CHUNK // 64 + 1
        print(json.dumps({"n": n, "payload_bytes": n * CHUNK, "wire_bytes": n * SLOT,
                          "gather_dev_median_ms": round(mg, 4), "ragged_dev_median_ms": round(mr, 4),
                          "gather_over_ragged": round(mg / mr, 3),
                          "k_sha1_ragged_median_ms": lanes and round(lanes, 4),
                          "gather_over_k_sha1_ragged": lanes and round(mg / lanes, 3),
                          "gather_GiB_s": round(n * CHUNK / 2**30 / (mg / 1e3), 2),
                          "ragged_GiB_s": round(n * CHUNK / 2**30 / (mr / 1e3), 2),
                          "gather_us_per_block": round(mg * 1e3 / blocks, 4),
                          "ragged_us_per_block": round(mr * 1e3 / blocks, 4),
                          "gather_dev_ms": [round(x, 4) for x in tg], "ragged_dev_ms": [round(x, 4) for x in tr],
                          **lat, "source_id": bt.source_id()}), flush=True)
        del wire, flat, dg, fv, d_seg


if __name__ == "__main__":
    main()
