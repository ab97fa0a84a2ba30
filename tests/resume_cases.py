"""Shared by tests/test_gpu_resume.py, tests/test_gpu_receiver.py and the
barrier-accounting child of tests/test_gpu_resume_barriers.py: the launch
shapes of the resumable chain kernel (bt_sha1_resume_dev), each compared with
the oracle, and what the kernel's barrier invariant predicts for them.

Every run_* function takes report(name, launches, problems): `launches` is the
list of (lens, totals) pairs of every message of every k_sha1_resume launch the
case made, `problems` a list of strings (empty when all results are exact).
"""
import ctypes

import numpy as np

IV = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]  # sha.c:149-163
SENT = 0xA5
PIECE = 1484  # save_data_packet's payload, util.c:275
NEVER = 0xFFFFFFFF


def nbatch(length, total):
    """64-block loader batches of one message of a launch (sha1_kernels.hip,
    k_sha1_resume): nb = lens >> 6 for an advance, plus the one or two padding
    blocks of sha.c:536-543 for a finish."""
    nb = length >> 6
    if total:
        nb += 2 if (length & 63) >= 56 else 1
    return (nb + 63) // 64


def barrier_want(launches):
    """(waves checked, barriers executed) of the barrier-accounting build: two
    waves per message, nbatch + 1 barriers per wave."""
    return 2 * len(launches), sum(2 * (nbatch(l, t) + 1) for l, t in launches)


def stride_rule(chunk_len, stride, piece=PIECE, length=None):
    """What bt_sha1_receiver does for a chunk delivered in `piece`-byte
    payloads with advance after each: ([(lens, totals)] of its launches,
    advance launches, bytes advanced before commit)."""
    length = chunk_len if length is None else length
    stride = stride or 65536
    hashed, launches = 0, []
    for o in range(0, length, piece):
        filled = min(o + piece, length)
        whole = filled & ~63
        if whole > hashed and whole - hashed >= stride:
            launches.append((whole - hashed, 0))
            hashed = whole
    nadv = len(launches)
    launches.append((length - hashed, length))
    return launches, nadv, hashed


class Batch:
    """n messages laid out in one device (or pinned host) buffer."""

    def __init__(self, torch, msgs, pads=None, pinned=False, fill=0):
        self.torch = torch
        self.msgs = [bytes(m) for m in msgs]
        pads = pads or [0] * len(msgs)
        self.offs, pos = [], 0
        for m, pad in zip(self.msgs, pads):
            pos += pad
            self.offs.append(pos)
            pos += len(m)
        self.host = np.full(pos + 64, fill, dtype=np.uint8)
        for m, o in zip(self.msgs, self.offs):
            self.host[o:o + len(m)] = np.frombuffer(m, dtype=np.uint8)
        t = torch.from_numpy(self.host.copy())
        self.buf = t.pin_memory() if pinned else t.cuda()
        n = len(msgs)
        st = torch.zeros(5 * n, dtype=torch.int32)
        self.states = st.pin_memory() if pinned else st.cuda()
        self.dig = torch.full((20 * n + 1,), SENT, dtype=torch.uint8, device="cuda")
        self.ok = torch.full((n + 1,), SENT, dtype=torch.uint8, device="cuda")

    def write(self, i, start, data):
        """Bytes [start, start + len(data)) of message i (relative to its offset)."""
        t = self.torch.frombuffer(bytearray(data), dtype=self.torch.uint8)
        o = self.offs[i] + start
        self.buf[o:o + len(data)] = t if self.buf.device.type == "cpu" else t.cuda()

    def set_states(self, states):
        flat = np.array([w for s in states for w in s], dtype=np.uint32).view(np.int32)
        t = self.torch.from_numpy(flat)
        self.states.copy_(t)

    def get_states(self):
        self.torch.cuda.synchronize()
        a = self.states.cpu().numpy().view(np.uint32)
        return [[int(x) for x in a[5 * i:5 * i + 5]] for i in range(len(self.msgs))]

    def launch(self, bt, starts, lens, totals, expected=None, digests=True):
        """One bt_sha1_resume_dev launch: message i's bytes [starts[i], starts[i] + lens[i])."""
        torch = self.torch
        n = len(self.msgs)
        o = torch.tensor([a + b for a, b in zip(self.offs, starts)], dtype=torch.int64, device="cuda")
        ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
        tt = torch.tensor(totals, dtype=torch.int64, device="cuda")
        exp = None
        if expected is not None:
            exp = torch.frombuffer(bytearray(b"".join(expected)), dtype=torch.uint8).cuda()
        bt.resume_dev(self.buf.data_ptr(), o.data_ptr(), ln.data_ptr(), tt.data_ptr(), n, self.states.data_ptr(),
                      self.dig.data_ptr() if digests else None, exp.data_ptr() if exp is not None else None,
                      self.ok.data_ptr() if exp is not None else None)
        torch.cuda.synchronize()
        return list(zip(lens, totals))

    def digests(self):
        raw = self.dig.cpu().numpy().tobytes()
        return [raw[20 * i:20 * i + 20] for i in range(len(self.msgs))], raw[20 * len(self.msgs)]

    def oks(self):
        a = [int(x) for x in self.ok.cpu()]
        return a[:-1], a[-1]


def synth(orc, n, seed):
    return bytes(orc.fill_synthetic(n, seed, 0x2E5))


ADVANCE_BLOCKS = (0, 1, 63, 64, 65, 128, 129)  # around the 64-block loader batches
ADVANCE_CHAINS = ((1, 64), (65, 63, 129), (64, 0, 1))


def run_advances(bt, torch, orc, report):
    """One advance of 0 .. 129 blocks from the IV (lens with and without a
    stray tail, which an advance must ignore), then two and three chained."""
    for k, nblk in enumerate(ADVANCE_BLOCKS):
        length = 64 * nblk + (17 if k % 2 else 0)
        msg = synth(orc, length, 10 + k)
        b = Batch(torch, [msg], pads=[k % 5])
        bt.states_init_dev(b.states.data_ptr(), 1)
        launches = b.launch(bt, [0], [length], [0])
        want = orc.compress_blocks(IV, msg[:64 * nblk])
        got = b.get_states()[0]
        bad = [] if got == want else [f"state {got} want {want}"]
        if b.digests() != ([bytes([SENT]) * 20], SENT):
            bad.append("an advance wrote a digest")
        report(f"advance {nblk} blocks, lens {length}", launches, bad)
    for k, chain in enumerate(ADVANCE_CHAINS):
        msg = synth(orc, 64 * sum(chain), 30 + k)
        b = Batch(torch, [msg], pads=[3])
        bt.states_init_dev(b.states.data_ptr(), 1)
        pos, want = 0, IV
        for nblk in chain:
            launches = b.launch(bt, [pos], [64 * nblk], [0])
            want = orc.compress_blocks(want, msg[pos:pos + 64 * nblk])
            pos += 64 * nblk
            got = b.get_states()[0]
            report(f"chain {chain}: after {pos // 64} blocks", launches,
                   [] if got == want else [f"state {got} want {want}"])


FINISH_R = (0, 1, 55, 56, 63)
FINISH_WHOLE = (0, 1, 64)
PREFIX = 192


def run_finishes(bt, torch, orc, report, compare_chunks_dev=True):
    """Finishes with every tail r and 0 / 1 / 64 whole blocks left: after a
    192-byte prefix advanced by an earlier launch (lens == 0 among them: the
    padding alone), and as messages never advanced (state = IV, total = len),
    which must also equal bt_sha1_chunks_dev's digest."""
    shapes = [(r, w) for r in FINISH_R for w in FINISH_WHOLE]
    msgs = [synth(orc, PREFIX + 64 * w + r, 50 + i) for i, (r, w) in enumerate(shapes)]
    want = [orc.sha1(m) for m in msgs]
    n = len(msgs)
    b = Batch(torch, msgs, pads=[(7 * i) % 16 for i in range(n)])
    bt.states_init_dev(b.states.data_ptr(), n)
    launches = b.launch(bt, [0] * n, [PREFIX] * n, [0] * n)
    mid = b.get_states()
    bad = [f"message {i}: state after the prefix" for i, m in enumerate(msgs)
           if mid[i] != orc.compress_blocks(IV, m[:PREFIX])]
    report("prefix advance of 15 messages", launches, bad)
    launches = b.launch(bt, [PREFIX] * n, [len(m) - PREFIX for m in msgs], [len(m) for m in msgs])
    got, canary = b.digests()
    bad = [f"r={shapes[i][0]} whole={shapes[i][1]}: {got[i].hex()} want {want[i].hex()}" for i in range(n)
           if got[i] != want[i]]
    if canary != SENT:
        bad.append("digest canary overwritten")
    if b.get_states() != mid:
        bad.append("a finish wrote a state back")
    report("finish after a prefix, 15 tails", launches, bad)

    fresh = [m[PREFIX:] for m in msgs if len(m) > PREFIX]  # total = len: the empty message cannot be a finish
    want = [orc.sha1(m) for m in fresh]
    n = len(fresh)
    b = Batch(torch, fresh, pads=[(5 * i) % 16 for i in range(n)])
    bt.states_init_dev(b.states.data_ptr(), n)
    launches = b.launch(bt, [0] * n, [len(m) for m in fresh], [len(m) for m in fresh])
    got, _ = b.digests()
    bad = [f"never advanced, len {len(fresh[i])}: {got[i].hex()} want {want[i].hex()}" for i in range(n)
           if got[i] != want[i]]
    if compare_chunks_dev:
        for i, m in enumerate(fresh):
            d = torch.zeros(len(m) + 64, dtype=torch.uint8, device="cuda")
            d[:len(m)] = torch.frombuffer(bytearray(m), dtype=torch.uint8).cuda()
            out = torch.zeros(20, dtype=torch.uint8, device="cuda")
            bt.chunks_dev(d.data_ptr(), 1, len(m), (len(m) + 15) // 16 * 16, out.data_ptr())
            torch.cuda.synchronize()
            if out.cpu().numpy().tobytes() != got[i]:
                bad.append(f"len {len(m)}: differs from bt_sha1_chunks_dev")
    report("finish of messages never advanced", launches, bad)


def run_mixed(bt, torch, orc, report):
    """7 messages in one launch, advances and finishes interleaved at random
    byte alignments, planted mismatches in every third finishing message."""
    import random
    rng = random.Random(77)
    kinds = "FAFFAFF"
    prefix = [64 * rng.randrange(0, 5) for _ in kinds]  # hashed before this launch (state uploaded from the oracle)
    lens = [64 * rng.randrange(0, 70) + rng.randrange(0, 64) for _ in kinds]
    lens[3] = 64 * 64 + 60  # a finish that fills a whole loader batch and needs two padding blocks
    msgs = [synth(orc, p + l, 80 + i) for i, (p, l) in enumerate(zip(prefix, lens))]
    n = len(msgs)
    b = Batch(torch, msgs, pads=[rng.randrange(0, 16) for _ in msgs])
    before = [orc.compress_blocks(IV, m[:p]) for m, p in zip(msgs, prefix)]
    b.set_states(before)
    fin = [i for i, k in enumerate(kinds) if k == "F"]
    planted = set(fin[::3])
    want_dig = [orc.sha1(m) for m in msgs]
    expected = [bytes(20) if i in planted else (want_dig[i] if kinds[i] == "F" else bytes([0x5A]) * 20)
                for i in range(n)]
    totals = [len(m) if k == "F" else 0 for m, k in zip(msgs, kinds)]
    launches = b.launch(bt, prefix, lens, totals, expected=expected)
    got, canary = b.digests()
    oks, ok_canary = b.oks()
    states = b.get_states()
    bad = []
    for i, k in enumerate(kinds):
        if k == "F":
            if got[i] != want_dig[i]:
                bad.append(f"message {i}: digest")
            if oks[i] != (0 if i in planted else 1):
                bad.append(f"message {i}: ok = {oks[i]}")
            if states[i] != before[i]:
                bad.append(f"message {i}: a finish wrote its state")
        else:
            if states[i] != orc.compress_blocks(before[i], msgs[i][prefix[i]:prefix[i] + (lens[i] & ~63)]):
                bad.append(f"message {i}: state")
            if got[i] != bytes([SENT]) * 20 or oks[i] != SENT:
                bad.append(f"message {i}: an advance wrote a digest or a verdict")
    if canary != SENT or ok_canary != SENT:
        bad.append("canary overwritten")
    report("mixed launch of 7", launches, bad)


def run_read_bound(bt, torch, orc, report):
    """The bytes right after offsets[i] + lens[i] hold 0xFF during a launch and
    the real data only before the next one: a launch that used a byte past its
    range would hash the 0xFF."""
    msgs = [synth(orc, 192 + 130 + 75, 120), synth(orc, 192 + 130 + 124, 121)]  # last launches: 77 and 126 bytes, tails r = 13 and r = 62
    want = [orc.sha1(m) for m in msgs]
    b = Batch(torch, [bytes([0xFF]) * len(m) for m in msgs], pads=[1, 6], fill=0xFF)
    bt.states_init_dev(b.states.data_ptr(), 2)
    launches, pos = [], [0, 0]
    for step, ln in enumerate(((192, 192), (130, 130), (75, 124))):
        for i in range(2):
            hashed = pos[i] & ~63  # earlier launches consumed whole blocks only
            b.write(i, hashed, msgs[i][hashed:pos[i] + ln[i]])
        torch.cuda.synchronize()
        last = step == 2
        starts = [p & ~63 for p in pos]
        lens = [pos[i] + ln[i] - starts[i] for i in range(2)]
        launches += b.launch(bt, starts, lens, [len(m) if last else 0 for m in msgs])
        pos = [pos[i] + ln[i] for i in range(2)]
    got, _ = b.digests()
    report("read bound: 0xFF past every launch's range", launches,
           [f"message {i}: {got[i].hex()} want {want[i].hex()}" for i in range(2) if got[i] != want[i]])


def run_pinned(bt, torch, orc, report):
    """d_base and d_states in pinned host memory: same results."""
    msgs = [synth(orc, 64 * 70 + 9, 140), synth(orc, 64 * 3 + 57, 141)]
    b = Batch(torch, msgs, pads=[2, 5], pinned=True)
    b.set_states([IV, IV])
    launches = b.launch(bt, [0, 0], [64 * 66, 64 * 2], [0, 0])
    bad = []
    if b.get_states() != [orc.compress_blocks(IV, msgs[0][:64 * 66]), orc.compress_blocks(IV, msgs[1][:128])]:
        bad.append("states in pinned memory")
    launches += b.launch(bt, [64 * 66, 128], [len(msgs[0]) - 64 * 66, len(msgs[1]) - 128], [len(m) for m in msgs])
    got, _ = b.digests()
    bad += [f"message {i}: digest" for i in range(2) if got[i] != orc.sha1(msgs[i])]
    report("pinned host base and states", launches, bad)


DEVICE_CASES = (run_advances, run_finishes, run_mixed, run_read_bound, run_pinned)


def deliver(rx, slot, data, upto=None, start=0, piece=PIECE):
    """Append data[start:upto] to the slot in `piece`-byte payloads (util.c:275), advance after each."""
    upto = len(data) if upto is None else upto
    for o in range(start, upto, piece):
        part = data[o:min(o + piece, upto)]
        ctypes.memmove(slot + o, part, len(part))
        rx.advance(slot, o + len(part))
