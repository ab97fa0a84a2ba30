"""Shared by tests/test_gpu_gather_resume.py, tests/test_gpu_gather_intake.py
and the barrier-accounting child of tests/test_gpu_gather_resume_barriers.py:
launches of the chain-form gather kernels (bt_sha1_gather_resume_dev, the
gather intake), each compared with the oracle, and what the kernels' barrier
invariant predicts for them (resume_cases.barrier_want: the formula is
k_sha1_resume's).

Every run_* function takes report(name, launches, problems) as resume_cases'
do: `launches` is the list of (len, total) pairs of every entry of every launch
the case made, `problems` a list of strings (empty when all results are exact).
"""
import ctypes
import random

import numpy as np

import gather_cases as gc
from resume_cases import FINISH_R, IV, NEVER, SENT

SEAM_K = (1, 63, 64, 65, 129, 130)      # resume at from = 64 k: around the 64-block loader batches
SEAM_BLOCKS = 130
CYCLE = (1484, 15, 0, 17, 1, 436)       # segment lengths of the seam messages, cycling


def carve(total, cycle=CYCLE):
    """Segment lengths that cycle through `cycle` and sum to `total`."""
    lens, k = [], 0
    while total:
        lens.append(min(cycle[k % len(cycle)], total))
        total -= lens[-1]
        k += 1
    return lens


def positions(seg_list, first, count):
    """d_seg_pos for gather_cases' tables: parallel to the segment rows, the
    message position of each segment's first byte."""
    pos = np.zeros(max(len(seg_list), 1), dtype=np.uint64)
    for f, c in zip(first, count):
        at = 0
        for k in range(int(f), int(f) + int(c)):
            pos[k] = at
            at += seg_list[k][1]
    return pos


class Tables:
    """One byte image and its segment rows on the device; launch() is one
    bt_sha1_gather_resume_dev call over entries that each name a row range."""

    def __init__(self, torch, blob, seg_rows, pos):
        self.torch = torch
        self.blob = torch.from_numpy(np.array(blob, dtype=np.uint8)).cuda()
        self.segs = torch.from_numpy(np.ascontiguousarray(seg_rows).view(np.int64)).cuda()
        self.pos = torch.from_numpy(np.ascontiguousarray(pos).view(np.int64)).cuda()

    def launch(self, bt, first, count, frm, lens, totals, states, expected=None, digests=True):
        """states: list of 5-word lists, one per entry.  Returns (states after,
        digests, oks, canaries untouched)."""
        torch = self.torch
        n = len(first)
        dev = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
        f, c = dev([int(x) for x in first], torch.int64), dev([int(x) for x in count], torch.int32)
        fr, ln, tt = dev(frm, torch.int64), dev(lens, torch.int32), dev(totals, torch.int64)
        st = torch.from_numpy(np.array([w for s in states for w in s], dtype=np.uint32).view(np.int32)).cuda()
        dig = torch.full((20 * n + 1,), SENT, dtype=torch.uint8, device="cuda")
        ok = torch.full((n + 1,), SENT, dtype=torch.uint8, device="cuda")
        exp = None
        if expected is not None:
            exp = torch.frombuffer(bytearray(b"".join(expected)), dtype=torch.uint8).cuda()
        bt.gather_resume_dev(self.blob.data_ptr(), self.segs.data_ptr(), self.pos.data_ptr(), f.data_ptr(),
                             c.data_ptr(), fr.data_ptr(), ln.data_ptr(), tt.data_ptr(), n, st.data_ptr(),
                             dig.data_ptr() if digests else None, exp.data_ptr() if exp is not None else None,
                             ok.data_ptr() if exp is not None else None)
        torch.cuda.synchronize()
        a = st.cpu().numpy().view(np.uint32)
        raw = dig.cpu().numpy().tobytes()
        oks = [int(x) for x in ok.cpu()]
        return ([[int(x) for x in a[5 * i:5 * i + 5]] for i in range(n)], [raw[20 * i:20 * i + 20] for i in range(n)],
                oks[:-1], raw[20 * n] == SENT and oks[-1] == SENT)


def from_batch(torch, batch):
    return Tables(torch, batch["blob"], batch["segs"], positions(batch["seg_list"], batch["first"], batch["count"]))


_cache = {}


def seam_batch(orc):
    """Five messages of 64 x 130 + r bytes, r in FINISH_R, carved by
    gather_cases.Builder into segments whose lengths cycle through CYCLE."""
    if "seam" not in _cache:
        b = gc.Builder(gc.SEED + 7)
        msgs = []
        for i, r in enumerate(FINISH_R):
            data = bytes(orc.fill_synthetic(64 * SEAM_BLOCKS + r, 300 + i, gc.SEED))
            segs = []
            at = 0
            for n in carve(len(data)):
                off, _ = b.place(n)
                b.blob[off:off + n] = data[at:at + n]
                segs.append((off, n))
                at += n
            b.message(segs)
            msgs.append(data)
        out = b.done()
        out["msgs"] = msgs
        assert out["want"] == b"".join(orc.sha1(m) for m in msgs)
        _cache["seam"] = out
    return _cache["seam"]


def run_seams(bt, torch, orc, report, mixed=False):
    """Every (k, r): advance [0, 64 k) from the IV, then finish from 64 k, each
    step ONE launch of 30 workgroups (r = 0 after k = 130 is len == 0: the
    padding alone).  mixed: the second launch finishes every other entry and
    advances the rest to block 130, a third finishes those."""
    batch = seam_batch(orc)
    t = from_batch(torch, batch)
    pairs = [(k, i) for k in SEAM_K for i in range(len(FINISH_R))]
    n = len(pairs)
    first = [batch["first"][i] for _, i in pairs]
    count = [batch["count"][i] for _, i in pairs]
    msgs = [batch["msgs"][i] for _, i in pairs]
    want = [batch["want"][20 * i:20 * i + 20] for _, i in pairs]
    hashed = [64 * k for k, _ in pairs]
    launches = list(zip(hashed, [0] * n))
    states, dig, _, clean = t.launch(bt, first, count, [0] * n, hashed, [0] * n, [IV] * n)
    bad = [f"k={pairs[e][0]} r={FINISH_R[pairs[e][1]]}: state after the advance" for e in range(n)
           if states[e] != orc.compress_blocks(IV, msgs[e][:hashed[e]])]
    if not clean or any(d != bytes([SENT]) * 20 for d in dig):
        bad.append("an advance wrote a digest")
    report("seams: advance to 64 k, 30 entries", launches, bad)
    bad = []
    if mixed:
        adv = [e for e in range(n) if e % 2 and hashed[e] < 64 * SEAM_BLOCKS]
        lens = [64 * SEAM_BLOCKS - hashed[e] if e in adv else len(msgs[e]) - hashed[e] for e in range(n)]
        totals = [0 if e in adv else len(msgs[e]) for e in range(n)]
        launches = list(zip(lens, totals))
        after, dig, _, clean = t.launch(bt, first, count, hashed, lens, totals, states)
        for e in range(n):
            if e in adv:
                if after[e] != orc.compress_blocks(IV, msgs[e][:64 * SEAM_BLOCKS]) or dig[e] != bytes([SENT]) * 20:
                    bad.append(f"entry {e}: advance inside a mixed launch")
            elif dig[e] != want[e] or after[e] != states[e]:
                bad.append(f"entry {e}: finish inside a mixed launch")
        report("seams: mixed advance / finish launch", launches, bad + ([] if clean else ["canary overwritten"]))
        first, count, msgs, want = ([x[e] for e in adv] for x in (first, count, msgs, want))
        states = [after[e] for e in adv]
        pairs = [pairs[e] for e in adv]
        hashed = [64 * SEAM_BLOCKS] * len(adv)
        n, bad = len(adv), []
    lens = [len(m) - h for m, h in zip(msgs, hashed)]
    totals = [len(m) for m in msgs]
    after, dig, _, clean = t.launch(bt, first, count, hashed, lens, totals, states)
    bad += [f"k={pairs[e][0]} r={FINISH_R[pairs[e][1]]}: {dig[e].hex()} want {want[e].hex()}" for e in range(n)
            if dig[e] != want[e]]
    if after != states:
        bad.append("a finish wrote a state back")
    report("seams: finish from 64 k", list(zip(lens, totals)), bad + ([] if clean else ["canary overwritten"]))


# ---- the gather intake ------------------------------------------------------
GAP = 16


def land(slot, data, lens, filler=0xEE, at=0):
    """`data` cut into segments of these lengths, each written into the slot
    (an integer address) behind a gap of filler, offsets at every residue mod
    16.  Returns the (off, len) list and the first free offset."""
    segs, o = [], 0
    for k, n in enumerate(lens):
        gap = GAP + (k % 16)
        ctypes.memset(slot + at, filler, gap)
        at += gap
        ctypes.memmove(slot + at, data[o:o + n], n)
        segs.append((at, n))
        at += n
        o += n
    return segs, at


def slot_bytes(total):
    """A slot length that holds `total` bytes carved by CYCLE and landed by land()."""
    return total + (GAP + 16) * (len(carve(total)) + 8)


def run_intake_seams(bt, orc, report):
    """The table form over the seam shapes: six slots, slot j's chunk is 64 x
    130 + r_j bytes and its first append ends 5 bytes past block k_j.  Stride
    64.  Kick 1 advances every slot to 64 k; then half the slots are committed
    and the others get the rest of their segments: kick 2 is a mixed table;
    kick 3 finishes the others."""
    shapes = [(k, FINISH_R[j % len(FINISH_R)]) for j, k in enumerate(SEAM_K)]
    chunks = [bytes(orc.fill_synthetic(64 * SEAM_BLOCKS + r, 400 + j, gc.SEED)) for j, (_, r) in enumerate(shapes)]
    want = [orc.sha1(c) for c in chunks]
    slot_len = slot_bytes(len(chunks[0]) + 64)
    rx = bt.Intake(chunk_len=slot_len, nslots=len(shapes), stride=64, gather=True, max_segs=64)
    try:
        slots, rest = [], []
        for (k, r), data in zip(shapes, chunks):
            p = rx.slot()
            cut = min(64 * k + 5, len(data))
            head, at = land(p, data[:cut], carve(cut))
            tail, _ = land(p, data[cut:], carve(len(data) - cut), at=at)
            rx.append(p, head)
            slots.append(p)
            rest.append(tail)
        s0 = rx.stats()
        n1 = rx.kick()
        rx.sync()
        s1 = rx.stats()
        launches = [(64 * k, 0) for k, _ in shapes]
        bad = []
        if n1 != len(shapes) or s1["launches"] - s0["launches"] != 1 or s1["entries"] - s0["entries"] != len(shapes):
            bad.append(f"kick 1: {n1} entries")
        if s1["advanced_bytes"] - s0["advanced_bytes"] != sum(l for l, _ in launches):
            bad.append("kick 1: advanced_bytes")
        report("intake seams: advance to 64 k", launches, bad)
        launches, bad = [], []
        for j, (k, r) in enumerate(shapes):
            if rest[j]:
                rx.append(slots[j], rest[j])
            total = len(chunks[j])
            if j % 2 == 0:
                rx.commit_gather(slots[j], want[j], j)
                launches.append((total - 64 * k, total))
            elif (total & ~63) > 64 * k:
                launches.append(((total & ~63) - 64 * k, 0))
        n2 = rx.kick()
        rx.sync()
        if n2 != len(launches):
            bad.append(f"kick 2: {n2} entries, want {len(launches)}")
        report("intake seams: mixed table", launches, bad)
        launches = []
        for j, (k, r) in enumerate(shapes):
            if j % 2:
                rx.commit_gather(slots[j], want[j], j)
                launches.append((len(chunks[j]) & 63, len(chunks[j])))
        n3 = rx.kick()
        rx.sync()
        got = sorted(rx.drain())
        bad = [] if n3 == len(launches) else [f"kick 3: {n3} entries"]
        if got != [(j, True, want[j]) for j in range(len(shapes))]:
            bad.append("verdicts: %r" % [(t, ok, d.hex()) for t, ok, d in got])
        report("intake seams: the remaining finishes", launches, bad)
    finally:
        rx.close()
