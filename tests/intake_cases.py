"""Shared by tests/test_gpu_intake.py and the barrier-accounting child of
tests/test_gpu_intake_barriers.py: runs of bt_sha1_intake whose launches are
known entry by entry, each compared with the oracle.

Every run_* function takes report(name, launches, problems) as the cases of
resume_cases.py do: `launches` is the list of (len, total) pairs of every table
entry of every k_sha1_resume_table launch the case made (total == 0: an
advance), `problems` a list of strings (empty when all results are exact).
Every count is taken after sync(), never from a race.
"""
import ctypes

import resume_cases as rc

FINISH_R = (0, 1, 55, 56, 63)
FINISH_WHOLE = (0, 1, 63, 64, 65, 129)  # around the 64-block loader batches
SHAPES = [(r, w) for w in FINISH_WHOLE for r in FINISH_R if (r, w) != (0, 0)]  # a chunk has at least one byte
SHAPE_CHUNK = 64 * 129 + 63


def chunk(orc, n, seed):
    return bytes(orc.fill_synthetic(n, seed, 0x1A7))


def put(slot, data, start=0, upto=None):
    """Bytes [start, upto) of `data` into the slot (no advance)."""
    part = data[start:len(data) if upto is None else upto]
    ctypes.memmove(slot + start, part, len(part))


def delta(ix, before):
    now = ix.stats()
    return {k: now[k] - before[k] for k in now}


def run_padding_shapes(bt, orc, report, stride):
    """One slot per (r, whole blocks) shape, all finished by ONE launch.  At
    stride NEVER nothing is hashed before the commit; at stride 64 every whole
    block is advanced first (one launch for all slots that have one), so the
    finishing entries carry the r tail bytes and the padding alone -- for
    r == 0 the padding alone, len 0.  The expected hash of shape 7 is wrong."""
    n = len(SHAPES)
    data = [chunk(orc, 64 * w + r, 200 + i) for i, (r, w) in enumerate(SHAPES)]
    want = [orc.sha1(d) for d in data]
    planted = 7
    ix = bt.Intake(chunk_len=SHAPE_CHUNK, nslots=n, stride=stride)
    try:
        slots = [ix.slot() for _ in range(n)]
        for p, d in zip(slots, data):
            put(p, d)
            ix.advance(p, len(d))
        before = ix.stats()
        got = ix.kick()
        ix.sync()
        d1 = delta(ix, before)
        if stride == rc.NEVER:
            adv = []
            bad = [] if got == 0 and d1["launches"] == 0 and d1["entries"] == 0 else [f"a kick before commit: {d1}"]
        else:
            adv = [(64 * w, 0) for r, w in SHAPES if w]
            bad = [] if (got == len(adv) and d1["launches"] == 1 and d1["entries"] == len(adv)
                         and d1["advanced_bytes"] == sum(l for l, _ in adv)) else [f"advance kick: {got} {d1}"]
            report(f"padding shapes, stride {stride}: the advances", adv, bad)
            bad = []
        for i, (p, d) in enumerate(zip(slots, data)):
            ix.commit(p, bytes(20) if i == planted else want[i], i, length=len(d))
        before = ix.stats()
        got = ix.kick()
        ix.sync()
        d2 = delta(ix, before)
        hashed = (lambda w: 0) if stride == rc.NEVER else (lambda w: 64 * w)
        fin = [(len(d) - hashed(w), len(d)) for d, (r, w) in zip(data, SHAPES)]
        if not (got == n and d2["launches"] == 1 and d2["entries"] == n and d2["deferred"] == 0
                and d2["advanced_bytes"] == 0):
            bad.append(f"finishing kick: {got} {d2}")
        if stride != rc.NEVER and not any(l == 0 for l, _ in fin):
            bad.append("no slot with the padding alone left")
        res = sorted(ix.drain())
        if res != [(i, i != planted, want[i]) for i in range(n)]:
            bad += [f"shape {SHAPES[i]}: {res[i] if i < len(res) else None}" for i in range(n)
                    if i >= len(res) or res[i] != (i, i != planted, want[i])]
        if delta(ix, before)["launches"] != 1:
            bad.append("drain launched again")
        report(f"padding shapes, stride {stride}: the finishes", fin, bad)
    finally:
        ix.close()


MIXED_CHUNK = 12 * 1024 + 192
MIXED_PART = 8000  # what the slots that are only advanced have received at the first kick


def run_mixed(bt, orc, report):
    """Eight slots in one table: the even ones complete and committed (never
    advanced before: one finishing entry over everything), the odd ones at
    8000 bytes (an advancing entry over 7936).  A later kick finishes the odd ones."""
    n = 8
    data = [chunk(orc, MIXED_CHUNK, 300 + i) for i in range(n)]
    want = [orc.sha1(d) for d in data]
    ix = bt.Intake(chunk_len=MIXED_CHUNK, nslots=n, stride=4096)
    try:
        slots = [ix.slot() for _ in range(n)]
        for i, (p, d) in enumerate(zip(slots, data)):
            if i % 2 == 0:
                put(p, d)
                ix.commit(p, want[i], i)
            else:
                put(p, d, 0, MIXED_PART)
                ix.advance(p, MIXED_PART)
        before = ix.stats()
        got = ix.kick()
        ix.sync()
        d1 = delta(ix, before)
        whole = MIXED_PART & ~63
        first = [(MIXED_CHUNK, MIXED_CHUNK) if i % 2 == 0 else (whole, 0) for i in range(n)]
        bad = [] if (got == n and d1["launches"] == 1 and d1["entries"] == n and d1["deferred"] == 0
                     and d1["advanced_bytes"] == (n // 2) * whole) else [f"mixed kick: {got} {d1}"]
        res = sorted(ix.poll())  # harvests the even ones; nothing is due, so its kick launches nothing
        if res != [(i, True, want[i]) for i in range(0, n, 2)]:
            bad.append(f"verdicts of the committed half: {res}")
        if delta(ix, before)["launches"] != 1:
            bad.append("poll launched with nothing due")
        report("mixed table: 4 finishes and 4 advances", first, bad)
        for i in range(1, n, 2):
            put(slots[i], data[i], MIXED_PART)
            ix.advance(slots[i], MIXED_CHUNK)  # due again: the finish below takes the span with it
            ix.commit(slots[i], want[i], i)
        before = ix.stats()
        got = ix.kick()
        ix.sync()
        d2 = delta(ix, before)
        bad = [] if (got == n // 2 and d2["launches"] == 1 and d2["entries"] == n // 2
                     and d2["advanced_bytes"] == 0) else [f"second kick: {got} {d2}"]
        res = sorted(ix.drain())
        if res != [(i, True, want[i]) for i in range(1, n, 2)]:
            bad.append(f"verdicts of the other half: {res}")
        report("mixed table: the later kick finishes the rest", [(MIXED_CHUNK - whole, MIXED_CHUNK)] * (n // 2), bad)
    finally:
        ix.close()
