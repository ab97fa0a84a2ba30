"""GPU: bit lengths past 2^32 and offsets past 4 GiB.

Lengths.  The padding's 64-bit bit count (sha.c:536-543) is written in six
places; the largest message of the suite is about 64 MiB, so its high word was
0 in every test and `(uint32_t)(bits >> 32)` could be replaced by 0 anywhere.
A message of 512 MiB and more never has to exist: chaining states and totals
are inputs of bt_sha1_resume_dev, of bt_sha1_column_dev and of the streaming
context, so a launch can finish a message whose first P bytes were "hashed
before".  Expected values are verdict_cases.wide_digest, which
tests/test_padding_reference.py checks against hashlib and against sha.c.
Covered here:
  chain_block (both branches)      resume_dev, 64 finishing entries, one launch
  k_sha1_lat's padding, kLatLast   column_dev LAST, 2 and 3 slots, +- fused compare
  SHA1Final in bt_dropin.cpp       the streaming context continued from a set
                                   totalLength, beside the reference's own
Still open -- each needs a real message of >= 512 MiB, one serial chain of
8.4 M blocks, 6 s or more per launch before the oracle hashes it:
  finish() in sha1_device.h (k_sha1_fixed, k_sha1_ragged), k_sha1_lat_ragged's
  `bits`, k_sha1_chain's own `len * 8ull`, and the table kernel's `total`
  (its chain_block call is the one resume_dev covers).

Offsets.  offsets[] is 64-bit in k_sha1_chain, k_sha1_lat_ragged,
k_sha1_ragged and k_sha1_resume, and the strided ragged form computes
i * pitch in 64 bits, but no ragged, chain or resume test placed a message at
or past 2^32.  One buffer of 4 GiB + 2 MiB, allocated and written only where
messages lie: the bytes an offset truncated to 32 bits would reach hold 0x5A
or other data, so truncation gives another digest.
"""
import contextlib
import ctypes
import os
import random

import numpy as np
import pytest

import test_gpu_launch_forms as lf
import verdict_cases as vc
from conftest import REPO, load_btsha1

pytestmark = pytest.mark.gpu

Guarded, settle, WRITTEN = lf.Guarded, lf.settle, lf.WRITTEN


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


def upload_words(torch, g, words):
    """uint32 words into the body of a Guarded output."""
    raw = np.asarray(words, dtype=np.uint32).reshape(-1).tobytes()
    assert len(raw) == g.used
    g.buf[g.lead:g.lead + g.used] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    return raw


# ---------------------------------------------------------------------------
# B. Bit lengths past 2^32
# ---------------------------------------------------------------------------
def test_wide_lengths_resume_kernel(bt, torch, oracle):
    """All 64 (P, tail) pairs of verdict_cases.GRID as finishing entries of one
    k_sha1_resume launch, totals[i] = P + len: digests exact; then with the
    fused compare, every fifth expectation off in bit 37."""
    cases = vc.grid_cases(oracle)
    n = len(cases)
    assert n == 64
    want_dig = b"".join(vc.wide_digest(oracle, st, p, tail) for p, tail, st in cases)
    blob, offs = bytearray(), []
    for i, (_, tail, _) in enumerate(cases):
        blob += bytes([0xEE]) * (1 + (7 * i) % 15)
        offs.append(len(blob))
        blob += tail
    blob += bytes(64)
    d = lf.upload(torch, blob)
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_len = torch.tensor([len(t) for _, t, _ in cases], dtype=torch.int32, device="cuda")
    # 2^61 - 128 + 129 bytes fit int64; the kernel reads the same 64 bits as uint64
    d_tot = torch.tensor([p + len(t) for p, t, _ in cases], dtype=torch.int64, device="cuda")
    exp, want_ok = vc.flip_every_fifth(want_dig)
    d_exp = torch.from_numpy(exp.reshape(-1)).cuda()
    for verify in (False, True):
        st = Guarded(torch, 5 * n, 4)
        st_bytes = upload_words(torch, st, [s for _, _, s in cases])
        dig, ok = Guarded(torch, n, 20, 1), Guarded(torch, n, 1, 3)
        bt.resume_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_tot.data_ptr(), n, st.ptr, dig.ptr,
                      d_exp.data_ptr() if verify else None, ok.ptr if verify else None)
        got = settle(torch, ("wide resume", verify), [("digests", dig, WRITTEN), ("states", st, st_bytes),
                                                     ("ok", ok, WRITTEN if verify else None)])
        wrong = [(f"P={cases[i][0]:#x}", f"tail {len(cases[i][1])}") for i in range(n)
                 if got["digests"][20 * i:20 * i + 20].tobytes() != want_dig[20 * i:20 * i + 20]]
        assert not wrong, (f"{len(wrong)} of {n} digests differ", wrong)
        if verify:
            off = [i for i in range(n) if got["ok"][i] != want_ok[i]]
            assert not off, ("verdicts differ at entries", off, [int(got["ok"][i]) for i in off])


_columns = {}


def column_reference(orc, cus, width):
    """(columns as an (nmax, width) array, states as (nmax, 5), {msg_len:
    digests back to back}) for nmax = 64 * CUs + 1 chunks, computed once per
    width; a launch of fewer chunks takes the prefix."""
    if width not in _columns:
        nmax = 64 * cus + 1
        rng = np.random.default_rng(0xC01 + width)
        cols = np.frombuffer(bytes(orc.fill_synthetic(nmax * width, width, 0xC01)), dtype=np.uint8).reshape(nmax, width)
        states = rng.integers(0, 2**32, size=(nmax, 5), dtype=np.uint64).astype(np.uint32)
        assert not (states == np.array(vc.IV, dtype=np.uint32)).all(axis=1).any()
        digs = {}
        for msg_len in vc.COLUMN_MSG_LENS:
            digs[msg_len] = b"".join(vc.wide_digest(orc, [int(x) for x in states[i]], msg_len - width, cols[i].tobytes())
                                     for i in range(nmax))
        _columns[width] = (cols, states, digs)
    return _columns[width]


@pytest.mark.parametrize("slots", [2, 3])
@pytest.mark.parametrize("width", vc.COLUMN_WIDTHS)
def test_wide_lengths_column_last(bt, torch, oracle, cus, width, slots):
    """k_sha1_lat<.., kLatLast>: the last `width` bytes of n messages of
    msg_len bytes each, chaining states in the column-major layout (word k of
    chunk i at state[k*n + i]); the only way to the latency kernel's padding
    with a high word.  Plain and with the fused compare, per msg_len."""
    n = 65 if slots == 2 else 64 * cus + 1
    assert (3 if (n + 63) // 64 > cus else 2) == slots, (n, cus, slots)
    cols, states, digs = column_reference(oracle, cus, width)
    d_col = torch.from_numpy(cols[:n].reshape(-1).copy()).cuda()
    assert d_col.data_ptr() % 16 == 0
    for msg_len in vc.COLUMN_MSG_LENS:
        want_dig = digs[msg_len][:20 * n]
        exp, want_ok = vc.flip_every_fifth(want_dig)
        d_exp = torch.from_numpy(exp.reshape(-1)).cuda()
        for verify in (False, True):
            st = Guarded(torch, 5 * n, 4)
            st_bytes = upload_words(torch, st, states[:n].T.copy())  # (5, n): column-major
            dig, ok = Guarded(torch, n, 20), Guarded(torch, n, 1, 3)
            assert st.ptr % 4 == 0 and dig.ptr % 4 == 0
            bt.column_dev(d_col.data_ptr(), n, width, width, bt.COLUMN_LAST, st.ptr, msg_len, dig.ptr,
                          d_exp.data_ptr() if verify else None, ok.ptr if verify else None)
            run = ("wide column", width, slots, f"msg_len={msg_len:#x}", verify)
            got = settle(torch, run, [("digests", dig, WRITTEN), ("states", st, st_bytes),
                                      ("ok", ok, WRITTEN if verify else None)])
            bad = vc.digest_problems(got["digests"], want_dig)
            if verify:
                off = [int(i) for i in np.nonzero(got["ok"] != want_ok)[0]]
                if off:
                    bad.append(f"{len(off)} verdicts differ, chunks {off[:20]}")
            assert not bad, (run, bad)


def test_wide_lengths_streaming_context(bt, oracle):
    """The drop-in's SHA1Context continued from totalLength = 8 * P and a
    random state, beside the REFERENCE's own context (sha.c in
    oracle/_ref/libref_sha1.so) set the same way: updates of 63 bytes, 1 byte
    (the count is now exactly 2^32 or 2^35 bits) and 65 bytes, the contexts
    compared after each; then SHA1Final's digest and totalLength."""
    ref_path = os.path.join(REPO, "oracle", "_ref", "libref_sha1.so")
    assert os.path.exists(ref_path), "oracle/_ref/libref_sha1.so missing: built by oracle/Makefile"
    ref = ctypes.CDLL(ref_path)
    ctx_t = bt.SHA1Context
    ref.SHA1Init.argtypes = [ctypes.POINTER(ctx_t)]
    ref.SHA1Update.argtypes = [ctypes.POINTER(ctx_t), ctypes.c_void_p, ctypes.c_uint32]
    ref.SHA1Final.argtypes = [ctypes.POINTER(ctx_t), ctypes.c_void_p]
    rng = random.Random(0x57E)
    for p in vc.STREAM_PREFIXES:
        state = vc.seeded_state(rng)
        msg = bytes(oracle.fill_synthetic(129, p % 1000, 0x57E))
        rc, s = ctx_t(), bt.Sha1()
        ref.SHA1Init(ctypes.byref(rc))
        for c in (rc, s.ctx):
            c.totalLength = 8 * p
            for k in range(5):
                c.hash[k] = state[k]
        at = 0
        for step, ln in enumerate((63, 1, 65)):
            piece = msg[at:at + ln]
            ref.SHA1Update(ctypes.byref(rc), (ctypes.c_uint8 * ln).from_buffer_copy(piece), ln)
            s.update(piece)
            at += ln
            nbuf = rc.bufferLength
            assert rc.totalLength == 8 * (p + at) and nbuf == at % 64, (p, step)
            assert (s.ctx.totalLength, list(s.ctx.hash), s.ctx.bufferLength) == \
                (rc.totalLength, list(rc.hash), nbuf), (p, step)
            assert bytes(s.ctx.buffer[:nbuf]) == bytes(rc.buffer[:nbuf]), (p, step)
            if step == 1:
                assert rc.totalLength in (2**32, 2**35) and rc.totalLength & 0xFFFFFFFF == 0
        out = (ctypes.c_uint8 * 20)()
        ref.SHA1Final(ctypes.byref(rc), out)
        got = s.final()
        assert got == bytes(out) == vc.wide_digest(oracle, state, p, msg), (p, got.hex(), bytes(out).hex())
        assert s.ctx.totalLength == rc.totalLength, p


# ---------------------------------------------------------------------------
# C. Offsets past 4 GiB
# ---------------------------------------------------------------------------
G4 = 2**32
BUF_BYTES = G4 + 2**21
LOW_FILL, HIGH_FILL = 0x5A, 0xC3  # bytes [0, 2^21) and [2^32 - 2^20, end) wherever no data was written
# (offset, length): at 3, straddling 2^32, ending at 2^32, starting at it, one past it and 64 KiB + 1 past it
MESSAGES = [(3, 4097), (3, 63), (G4 - 200, 1000), (G4 - 200, 4097), (G4 - 64, 64), (G4 - 64, 129),
            (G4, 1), (G4, 120), (G4 + 1, 55), (G4 + 1, 1000), (G4 + 65537, 56), (G4 + 65537, 119)]
# written data: (start, bytes); everything a message or a strided chunk covers
DATA_SPANS = [(0, 8192), (2**31, 4096), (G4 - 4096, 12288), (G4 + 65536, 4096)]
STRIDE_N, STRIDE_LEN = 3, 1000
# 2^31 + 24 is no multiple of 16; 2^31 + 16 is, but 64 * pitch + 4096 > 2^32: neither is the hot kernel's layout
STRIDE_PITCHES = (2**31 + 24, 2**31 + 16)
MODES = ["default", "latr", "lanes"]


class Wide:
    """The 4 GiB + 2 MiB device buffer and a host copy of what was written to it."""

    def __init__(self, torch, orc):
        self.buf = torch.empty(BUF_BYTES, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[:2**21] = LOW_FILL
        self.buf[G4 - 2**20:] = HIGH_FILL
        self.spans = []
        for k, (start, size) in enumerate(DATA_SPANS):
            data = bytes(orc.fill_synthetic(size, 77 + k, 0xFA57))
            self.buf[start:start + size] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            self.spans.append((start, data))
        torch.cuda.synchronize()

    def read(self, off, length):
        for start, data in self.spans:
            if start <= off and off + length <= start + len(data):
                return data[off - start:off - start + length]
        raise AssertionError(f"[{off:#x}, +{length}) is not inside one written span")


@pytest.fixture(scope="module")
def wide(torch, oracle):
    w = Wide(torch, oracle)
    # what a truncated offset would read differs from what lies at the offset
    for off, ln in MESSAGES:
        if off >= G4:
            low = w.read(off - G4, ln) if off - G4 + ln <= 8192 else bytes([LOW_FILL]) * ln
            assert low != w.read(off, ln)
    yield w
    del w.buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def message_digests(wide, oracle):
    assert all(off + ln <= BUF_BYTES for off, ln in MESSAGES)
    return b"".join(oracle.sha1(wide.read(off, ln)) for off, ln in MESSAGES)


@contextlib.contextmanager
def ragged_form(bt, mode, n):
    """The ragged launcher's three kernels, each asserted before it is used
    (it shares the fixed-layout thresholds, which kernel_name reports):
    default knobs with n within the chain batch -> k_sha1_chain by offsets;
    "latr" -> k_sha1_lat_ragged; "lanes" -> k_sha1_ragged."""
    if mode == "default":
        assert bt.kernel_name(n) == "k_sha1_chain", (n, bt.kernel_name(n))
        yield
    else:
        with lf.ragged_mode(bt, mode):
            assert bt.kernel_name(n) == ("k_sha1_lat" if mode == "latr" else "k_sha1_fixed"), (mode, bt.kernel_name(n))
            yield


def named_problems(got, want, names):
    g = np.frombuffer(bytes(got), dtype=np.uint8).reshape(-1, 20)
    w = np.frombuffer(bytes(want), dtype=np.uint8).reshape(-1, 20)
    return [f"{names[i]}: {g[i].tobytes().hex()} want {w[i].tobytes().hex()}" for i in range(len(names))
            if not np.array_equal(g[i], w[i])]


MESSAGE_NAMES = [f"offset 2^32{off - G4:+d} len {ln}" if off > 2**31 else f"offset {off} len {ln}" for off, ln in MESSAGES]


@pytest.mark.parametrize("mode", MODES)
def test_wide_offsets_ragged(bt, torch, wide, message_digests, mode):
    """ragged_dev over messages at and past 2^32, through each of its kernels."""
    n = len(MESSAGES)
    d_off = torch.tensor([o for o, _ in MESSAGES], dtype=torch.int64, device="cuda")
    d_len = torch.tensor([ln for _, ln in MESSAGES], dtype=torch.int32, device="cuda")
    dig = Guarded(torch, n, 20, 1)
    with ragged_form(bt, mode, n):
        bt.ragged_dev(wide.buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, dig.ptr)
        got = settle(torch, ("wide ragged", mode), [("digests", dig, WRITTEN)])
    bad = named_problems(got["digests"], message_digests, MESSAGE_NAMES)
    assert not bad, (mode, bad)


def test_wide_offsets_resume(bt, torch, oracle, wide, message_digests):
    """k_sha1_resume at the same offsets: one launch advances every message
    over its whole blocks (states checked against the oracle), the next
    finishes each from offset + whole blocks."""
    n = len(MESSAGES)
    whole = [ln & ~63 for _, ln in MESSAGES]
    d_len = torch.tensor([ln for _, ln in MESSAGES], dtype=torch.int32, device="cuda")
    st = Guarded(torch, 5 * n, 4)
    dig = Guarded(torch, n, 20, 1)
    bt.states_init_dev(st.ptr, n)
    d_off = torch.tensor([o for o, _ in MESSAGES], dtype=torch.int64, device="cuda")
    d_zero = torch.zeros(n, dtype=torch.int64, device="cuda")
    bt.resume_dev(wide.buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_zero.data_ptr(), n, st.ptr, dig.ptr)
    mid = np.array([oracle.compress_blocks(vc.IV, wide.read(o, w)) for (o, _), w in zip(MESSAGES, whole)],
                   dtype=np.uint32)
    got = settle(torch, "wide resume: advance", [("states", st, WRITTEN), ("digests", dig, None)])
    states = got["states"].view(np.uint32).reshape(n, 5)
    bad = [MESSAGE_NAMES[i] for i in range(n) if not np.array_equal(states[i], mid[i])]
    assert not bad, ("states after the advance", bad)
    d_off2 = torch.tensor([o + w for (o, _), w in zip(MESSAGES, whole)], dtype=torch.int64, device="cuda")
    d_len2 = torch.tensor([ln - w for (_, ln), w in zip(MESSAGES, whole)], dtype=torch.int32, device="cuda")
    d_tot = torch.tensor([ln for _, ln in MESSAGES], dtype=torch.int64, device="cuda")
    bt.resume_dev(wide.buf.data_ptr(), d_off2.data_ptr(), d_len2.data_ptr(), d_tot.data_ptr(), n, st.ptr, dig.ptr)
    got = settle(torch, "wide resume: finish", [("states", st, mid.tobytes()), ("digests", dig, WRITTEN)])
    bad = named_problems(got["digests"], message_digests, MESSAGE_NAMES)
    assert not bad, bad


@pytest.mark.parametrize("pitch", STRIDE_PITCHES, ids=["pitch2^31+24", "pitch2^31+16"])
@pytest.mark.parametrize("mode", MODES)
def test_wide_offsets_strided(bt, torch, oracle, wide, mode, pitch):
    """chunks_dev with a pitch the hot kernel's layout refuses: chunk i at
    i * pitch, computed in 64 bits by each ragged kernel; chunk 2 starts past 2^32."""
    assert pitch % 16 != 0 or 64 * pitch + 4096 > G4  # bt_runtime.cpp fast_layout: not the fixed-layout kernels
    assert (STRIDE_N - 1) * pitch > G4 and (STRIDE_N - 1) * pitch + STRIDE_LEN <= BUF_BYTES
    want = b"".join(oracle.sha1(wide.read(i * pitch, STRIDE_LEN)) for i in range(STRIDE_N))
    assert wide.read((STRIDE_N - 1) * pitch, STRIDE_LEN) != wide.read((STRIDE_N - 1) * pitch - G4, STRIDE_LEN)
    dig = Guarded(torch, STRIDE_N, 20, 1)
    with ragged_form(bt, mode, STRIDE_N):
        bt.chunks_dev(wide.buf.data_ptr(), STRIDE_N, STRIDE_LEN, pitch, dig.ptr)
        got = settle(torch, ("wide strided", mode, pitch), [("digests", dig, WRITTEN)])
    bad = named_problems(got["digests"], want, [f"chunk {i} at {i * pitch:#x}" for i in range(STRIDE_N)])
    assert not bad, (mode, pitch, bad)
