"""GPU: the fixed-layout kernels at the largest pitch their contract admits.

k_sha1_fixed, k_sha1_lat and its column forms address a wave's 64 chunks as a
64-bit base `base + chunk0 * (uint64_t)pitch` plus 32-bit buffer offsets
`voff = lane * pitch` and `nrec = (nvalid - 1) * pitch + ...` (cast to int for
the descriptor).  The host admits 64 * pitch + 4096 <= 2^32 (fast_layout,
bt_runtime.cpp), the column launcher 64 * pitch < 2^32, but the largest pitch
of any other test of ordinary size is 512 KiB + 256: voff of lane 63 and nrec
stay 100 times below 2^32, every wave's base below it, and a 32-bit
`chunk0 * pitch` would show only in the 64 GiB run of the hot kernel.

Here P = 2^26 - 64, the largest pitch fast_layout takes (64 * P + 4096 = 2^32
exactly), and n = 130 chunks in one device buffer of 130 * 2^26 bytes that is
written only where chunks lie:
  voff of lane 63      63 * P = 2^32 - 2^26 - 4032
  nrec of a full wave  63 * P + len, past 2^31: negative as the int it is cast to
  wave bases           chunk0 = 64 and 128 start at 2^32 - 4096 and 2^33 - 8192
  idx * 20             digests and verdicts of chunks 64 .. 129, behind canaries
  the last wave        2 chunks (nvalid - 1 = 1)
Chunk i holds rows i of one synthetic stream, so a chunk read from another
chunk's address shows; and wherever i * pitch mod 2^32 is not i * pitch (or
the wave's chunk0 * pitch mod 2^32 plus the lane's offset is not), a fixed
filler lies at that truncated address (laid before the chunks, which may
overlap it), so a base or an offset cut to 32 bits reads defined bytes that
are asserted to differ from the chunk.  Expected values are oracle.sha1 and
oracle.compress_blocks of the host copy.

The neighbour P + 16 is refused by fast_layout: chunks_dev must hash it
through the ragged kernels (i * pitch in 64 bits), verify_dev must refuse it.
The columns run at their launcher's own largest pitch, 2^26 - 16.

Not reachable at this pitch: the hot kernel's 256-thread form (it needs
256 * CUs chunks: 4 TiB of address space), the 3-slot latency form (more than
CUs workgroups: 1 TiB) and the image-tail form (pitch == chunk_len: a real
64 MiB serial chain per lane).  Their launch forms are covered at small
pitches by test_gpu_launch_forms.py.
"""
import numpy as np
import pytest

import test_gpu_launch_forms as lf
import test_gpu_parity as par
import test_gpu_wide_lengths as wl
import verdict_cases as vc
from conftest import load_btsha1

pytestmark = pytest.mark.gpu

Guarded, settle, WRITTEN = lf.Guarded, lf.settle, lf.WRITTEN
kernel_mode, LAT, CHAIN = par.kernel_mode, par.LAT, par.CHAIN
named_problems = wl.named_problems

G4 = 2**32
N = 130
SLOT = 2**26
BUF_BYTES = N * SLOT
P = SLOT - 64            # fast_layout's largest pitch
P_REFUSED = P + 16       # the next multiple of 16: 64 * pitch + 4096 = 2^32 + 1024
P_COLUMN = SLOT - 16     # btsha1_launch_column's largest pitch: 64 * pitch = 2^32 - 1024
LENS = (56, 448, 4096 + 17)  # two padding blocks and no main loop; epilogue only; main loop, epilogue and a tail
ROW = 4128               # bytes laid per chunk: the longest length rounded up to 16
FILLER = 0x5A
PLANTED = (0, 63, 64, 127, 128, 129)  # first and last chunk of each full wave, both chunks of the last
MODES = [3, LAT, CHAIN]
MODE_IDS = ["hot64", "lat2", "chain"]
COLUMNS = [(0, 128), (128, 64), (192, 192)]  # FIRST, MIDDLE, LAST: (offset, width); msg_len 384
MSG_LEN = 384


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


class Pitched:
    """The 130 * 2^26-byte device buffer and the host copy of its 130 rows.
    lay(pitch) puts row i at i * pitch and the filler at every truncated
    address, and checks on the CPU what a truncated read would see."""

    def __init__(self, torch, orc):
        self.torch = torch
        self.buf = torch.empty(BUF_BYTES, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        stream = bytes(orc.fill_synthetic(N * ROW, 0x9A7C, 0x9A7C))  # one stream of distinct words: every row distinct
        self.rows = np.frombuffer(stream, dtype=np.uint8).reshape(N, ROW)
        assert len({self.rows[i, :56].tobytes() for i in range(N)}) == N
        self.d_rows = torch.from_numpy(self.rows.copy()).cuda()
        self.pitch = None
        self.digests = {ln: b"".join(orc.sha1(self.rows[i, :ln].tobytes()) for i in range(N)) for ln in LENS}

    def lay(self, pitch):
        if self.pitch == pitch:
            return
        torch = self.torch
        assert pitch % 16 == 0 and ROW <= pitch and (N - 1) * pitch + ROW <= BUF_BYTES
        # (chunk, address) where a 32-bit i * pitch, or a 32-bit chunk0 * pitch under a 64-bit lane offset, lands
        low = []
        for i in range(N):
            c0 = i & ~63
            low += [(i, a) for a in sorted({i * pitch % G4, c0 * pitch % G4 + (i - c0) * pitch}) if a != i * pitch]
        assert {i for i, _ in low} == set(range(65, N)) and all(a + ROW <= BUF_BYTES for _, a in low)
        for _, a in low:
            self.buf[a:a + ROW] = FILLER
        view = self.buf.as_strided((N, ROW), (pitch, 1))
        view.copy_(self.d_rows)
        torch.cuda.synchronize()
        assert np.array_equal(view.cpu().numpy(), self.rows), "the rows did not reach i * pitch"
        assert np.array_equal(self.buf[(N - 1) * pitch:(N - 1) * pitch + ROW].cpu().numpy(), self.rows[N - 1])
        # what lies at a truncated address: filler, overlaid by the rows that were written after it
        for i, a in low:
            seen = np.full(ROW, FILLER, dtype=np.uint8)
            for j in range(N):
                lo, hi = max(a, j * pitch), min(a + ROW, j * pitch + ROW)
                if lo < hi:
                    assert j != i
                    seen[lo - a:hi - a] = self.rows[j, lo - j * pitch:hi - j * pitch]
            got = self.buf[a:a + ROW].cpu().numpy()
            assert np.array_equal(got, seen), ("truncated address of chunk", i)
            for ln in LENS + (64,):
                assert not np.array_equal(seen[:ln], self.rows[i, :ln]), (i, ln)
        self.pitch = pitch


@pytest.fixture(scope="module")
def pitched(torch, oracle):
    p = Pitched(torch, oracle)
    yield p
    del p.buf
    torch.cuda.empty_cache()


CHUNK_NAMES = [f"chunk {i}" for i in range(N)]


def assert_form(bt, cus, mode):
    """130 chunks: the hot kernel in 64-thread workgroups, k_sha1_lat with 2 slots, or k_sha1_chain."""
    if mode == LAT:
        lf.assert_lat(bt, cus, N, False, 2)
    elif mode == CHAIN:
        assert bt.kernel_name(N) == "k_sha1_chain", bt.kernel_name(N)
    else:
        assert bt.kernel_name(N) == "k_sha1_fixed" and N < 256 * cus, (bt.kernel_name(N), cus)


def test_the_shapes_sit_on_the_limits():
    assert P % 16 == 0 and 64 * P + 4096 == G4              # fast_layout takes P and nothing larger
    assert P_REFUSED % 16 == 0 and 64 * P_REFUSED + 4096 > G4
    assert P_COLUMN % 16 == 0 and 64 * P_COLUMN < G4 <= 64 * (P_COLUMN + 16)
    assert 63 * P + max(LENS) > 2**31                        # nrec of a full wave is negative as an int
    assert (64 * P, 128 * P) == (G4 - 4096, 2 * G4 - 8192)   # the bases of the waves at chunk0 = 64 and 128
    assert N % 64 == 2
    assert (N - 1) * P_REFUSED + max(LENS) <= BUF_BYTES      # chunk 129 at P + 16 still fits the buffer
    assert (N - 1) * P_COLUMN + MSG_LEN <= BUF_BYTES


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_max_pitch_plain_digests(bt, torch, cus, pitched, mode):
    pitched.lay(P)
    with kernel_mode(bt, mode):
        assert_form(bt, cus, mode)
        for ln in LENS:
            dig = Guarded(torch, N, 20)
            assert dig.ptr % 4 == 0
            bt.chunks_dev(pitched.buf.data_ptr(), N, ln, P, dig.ptr)
            got = settle(torch, ("max pitch plain", mode, ln), [("digests", dig, WRITTEN)])
            bad = named_problems(got["digests"], pitched.digests[ln], CHUNK_NAMES)
            assert not bad, (mode, ln, len(bad), bad[:8])


def planted_expectations(digests):
    """Expectations with one bit off at the PLANTED indices (another bit at each), and the verdicts."""
    exp = np.frombuffer(digests, dtype=np.uint8).reshape(N, 20).copy()
    for k, i in enumerate(PLANTED):
        bit = (31 * k + 7) % 160
        exp[i, bit // 8] ^= 1 << (bit % 8)
    ok = np.ones(N, dtype=np.uint8)
    ok[list(PLANTED)] = 0
    return exp, ok


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_max_pitch_fused_compare(bt, torch, cus, pitched, mode):
    pitched.lay(P)
    with kernel_mode(bt, mode):
        assert_form(bt, cus, mode)
        for ln in LENS:
            want_dig = pitched.digests[ln]
            for exact in (False, True):
                exp, want_ok = planted_expectations(want_dig)
                if exact:
                    exp, want_ok = np.frombuffer(want_dig, dtype=np.uint8), np.ones(N, dtype=np.uint8)
                d_exp = torch.zeros(20 * N + 1, dtype=torch.uint8, device="cuda")
                d_exp[1:] = torch.from_numpy(exp.reshape(-1).copy()).cuda()
                ok, dig = Guarded(torch, N, 1, 3), Guarded(torch, N, 20)
                assert (d_exp.data_ptr() + 1) % 2 == 1 and ok.ptr % 2 == 1 and dig.ptr % 4 == 0
                bt.verify_dev(pitched.buf.data_ptr(), N, ln, P, d_exp.data_ptr() + 1, ok.ptr, dig.ptr)
                run = ("max pitch verify", mode, ln, "exact" if exact else "planted")
                got = settle(torch, run, [("ok", ok, WRITTEN), ("digests", dig, WRITTEN)])
                bad = named_problems(got["digests"], want_dig, CHUNK_NAMES)[:8]
                off = [int(i) for i in np.nonzero(got["ok"] != want_ok)[0]]
                if off:
                    bad.append(f"{len(off)} verdicts differ, chunks {off[:20]}: ok = {[int(got['ok'][i]) for i in off[:20]]}")
                assert not bad, (run, bad)


@pytest.mark.parametrize("mode", wl.MODES)
def test_neighbour_pitch_takes_the_ragged_kernels(bt, torch, pitched, mode):
    """P + 16: fast_layout refuses it, so chunks_dev hashes chunk i at
    i * pitch, in 64 bits, through k_sha1_chain, k_sha1_lat_ragged or k_sha1_ragged."""
    pitched.lay(P_REFUSED)
    with wl.ragged_form(bt, mode, N):
        for ln in LENS:
            dig = Guarded(torch, N, 20)
            bt.chunks_dev(pitched.buf.data_ptr(), N, ln, P_REFUSED, dig.ptr)
            got = settle(torch, ("neighbour pitch", mode, ln), [("digests", dig, WRITTEN)])
            bad = named_problems(got["digests"], pitched.digests[ln], CHUNK_NAMES)
            assert not bad, (mode, ln, len(bad), bad[:8])


def test_neighbour_pitch_is_refused_by_verify(bt, torch, pitched):
    pitched.lay(P_REFUSED)
    ln = LENS[1]
    d_exp = torch.from_numpy(np.frombuffer(pitched.digests[ln], dtype=np.uint8).copy()).cuda()
    ok, dig = Guarded(torch, N, 1), Guarded(torch, N, 20)
    with pytest.raises(bt.BtSha1Error, match=r"verify needs a 16-byte aligned layout with 64\*pitch \+ 4096 <= 4 GiB"):
        bt.verify_dev(pitched.buf.data_ptr(), N, ln, P_REFUSED, d_exp.data_ptr(), ok.ptr, dig.ptr)
    settle(torch, "neighbour pitch verify", [("ok", ok, None), ("digests", dig, None)])


def test_max_pitch_columns(bt, torch, oracle, cus, pitched):
    """column_dev at 2^26 - 16 with 130 rows, hashed where they lie: FIRST of
    128 bytes, MIDDLE of 64, LAST of 192 (msg_len 384) without and with the
    fused compare; the chaining states after each column, the digests and
    verdicts after the last."""
    pitched.lay(P_COLUMN)
    assert (N + 63) // 64 <= cus  # 2 slots
    base = pitched.buf.data_ptr()
    msgs = [pitched.rows[i, :MSG_LEN].tobytes() for i in range(N)]
    want_dig = b"".join(oracle.sha1(m) for m in msgs)
    st = Guarded(torch, 5 * N, 4)
    assert st.ptr % 4 == 0
    for part, (off, width) in zip((bt.COLUMN_FIRST, bt.COLUMN_MIDDLE), COLUMNS[:2]):
        bt.column_dev(base + off, N, P_COLUMN, width, part, st.ptr)
        got = settle(torch, ("max pitch column", part), [("states", st, WRITTEN)])
        states = got["states"].copy().view(np.uint32).reshape(5, N)  # column-major: word k of chunk i at [k, i]
        want = np.array([oracle.compress_blocks(vc.IV, m[:off + width]) for m in msgs], dtype=np.uint32).T
        wrong = [int(i) for i in np.nonzero((states != want).any(axis=0))[0]]
        assert not wrong, (("FIRST", "MIDDLE")[part], f"{len(wrong)} of {N} states differ, chunks {wrong[:20]}")
    st_bytes = got["states"].tobytes()
    off, width = COLUMNS[2]
    assert off + width == MSG_LEN
    exp, want_ok = planted_expectations(want_dig)
    d_exp = torch.from_numpy(exp.reshape(-1).copy()).cuda()
    for verify in (False, True):
        dig, ok = Guarded(torch, N, 20), Guarded(torch, N, 1, 3)
        assert dig.ptr % 4 == 0
        bt.column_dev(base + off, N, P_COLUMN, width, bt.COLUMN_LAST, st.ptr, MSG_LEN, dig.ptr,
                      d_exp.data_ptr() if verify else None, ok.ptr if verify else None)
        run = ("max pitch column LAST", "verify" if verify else "plain")
        got = settle(torch, run, [("digests", dig, WRITTEN), ("states", st, st_bytes),
                                  ("ok", ok, WRITTEN if verify else None)])
        bad = named_problems(got["digests"], want_dig, CHUNK_NAMES)[:8]
        if verify:
            diff = [int(i) for i in np.nonzero(got["ok"] != want_ok)[0]]
            if diff:
                bad.append(f"{len(diff)} verdicts differ, chunks {diff[:20]}")
        assert not bad, (run, bad)
