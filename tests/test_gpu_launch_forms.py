"""GPU: the launch forms that only large batches reach, at small shapes.

The kernels of sha1_kernels.hip change form with the batch size and the
device's CU count (`cus`): k_sha1_fixed and k_sha1_ragged run 64-thread
workgroups below 256 * cus chunks and 256-thread ones from there on
(chain_workgroup); k_sha1_lat and k_sha1_lat_ragged run with 2 LDS slots up to
`cus` workgroups and with 3 past that (launch_lat, btsha1_launch_ragged).  The
thresholds count chunks, not bytes, so chunks of 0 to about 1 KiB reach every
form with images of at most 64 MiB:

  1. k_sha1_fixed in 256-thread workgroups -- the shipping hot path: plain
     digests, the fused compare (with and without a digest buffer, `expected`
     and `ok` at odd addresses), the tail wave as wave 0, 1, 2 or 3 of a
     four-wave block, and the stamped build of the clock probe;
  2. k_sha1_ragged in 256-thread workgroups, by offsets and strided;
  3. the 3-slot k_sha1_lat (plain, fused compare, tail chunk -- also where the
     tail's own workgroup is what takes the grid past `cus`) and
     k_sha1_lat_ragged at both slot counts with workgroups whose messages all
     fit one or two blocks.

Every expected digest comes from the oracle.  Every output of every device
launch (digests, ok, clock stamps) lies inside a larger buffer filled with a
sentinel byte, 64 entries of guard on either side: "lanes past the end re-hash
the wave's last chunk, no store", the tail digest's index and the
`digests == nullptr` branches are checked by what must stay unwritten, which a
buffer of exactly 20 * n bytes cannot show.  Each test first asserts the form
it means to hit, so a device whose CU count would send the shape elsewhere
fails loudly instead of testing the 64-thread or 2-slot form again.
"""
import contextlib
import random

import numpy as np
import pytest

import column_cases as cc
from conftest import load_btsha1

pytestmark = pytest.mark.gpu

GUARD, SENT = cc.GUARD, cc.SENT
LAT = "lat"
WRITTEN = object()  # settle(): an output whose values the test checks itself; only its guards are checked
SEED = 0xF0A3


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


@contextlib.contextmanager
def kernel_mode(bt, mode):
    """Pin the fixed-layout launches to the latency kernel (LAT) or to the hot
    kernel (3 = its ring depth; latency and chain kernels off), as
    test_gpu_parity.kernel_mode does.  Restores the defaults."""
    prev = bt.set_latency_batch(1 << 62 if mode == LAT else 0)
    prev_chain = bt.set_chain_batch(0)
    if mode != LAT:
        bt.set_variant(mode, 1, 0)
    try:
        yield
    finally:
        bt.set_variant(3, 1, 0)
        bt.set_latency_batch(prev)
        bt.set_chain_batch(prev_chain)


@contextlib.contextmanager
def ragged_mode(bt, mode):
    """Pin ragged batches to the ragged latency kernel ("latr") or to the
    one-message-per-lane ragged kernel ("lanes"), as test_gpu_parity.ragged_mode does."""
    prev = bt.set_chain_batch(0)
    prev_lat = bt.set_latency_batch(0 if mode == "lanes" else 1 << 62)
    try:
        yield
    finally:
        bt.set_chain_batch(prev)
        bt.set_latency_batch(prev_lat)


# ---------------------------------------------------------------------------
# Canaries
# ---------------------------------------------------------------------------
class Guarded:
    """One output of a launch: `count` entries of `entry` bytes inside a device
    buffer filled with SENT, GUARD entries before and after it (`shift` more
    bytes in front, for outputs that take any alignment).  A launch that is
    deliberately not given the buffer still gets one, checked whole."""

    def __init__(self, torch, count, entry, shift=0):
        self.entry, self.lead, self.used = entry, GUARD * entry + shift, count * entry
        self.buf = torch.full((self.lead + self.used + GUARD * entry,), SENT, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + self.lead


def settle(torch, label, outputs):
    """After a launch: outputs = [(name, Guarded, want)] with want = the exact
    bytes, WRITTEN (guards only) or None (the buffer was not passed: all of it
    still SENT).  One copy to the host per output; asserts that nothing
    differs and returns {name: the output's bytes as a numpy array}."""
    torch.cuda.synchronize()
    problems, bodies = [], {}
    for name, g, want in outputs:
        raw = g.buf.cpu().numpy()
        body = bodies[name] = raw[g.lead:g.lead + g.used]
        if not (raw[:g.lead] == SENT).all():
            problems.append(f"{name}: written before the output")
        if not (raw[g.lead + g.used:] == SENT).all():
            problems.append(f"{name}: written past the output")
        if want is None:
            if not (body == SENT).all():
                problems.append(f"{name}: written though the launch was not given it")
        elif want is not WRITTEN:
            w = np.frombuffer(want, dtype=np.uint8)
            assert w.size == g.used, (label, name, w.size, g.used)
            if not np.array_equal(body, w):
                wrong = np.nonzero((body.reshape(-1, g.entry) != w.reshape(-1, g.entry)).any(axis=1))[0]
                problems.append(f"{name}: {len(wrong)} of {g.used // g.entry} entries differ, first {wrong[0]}")
    assert not problems, (label, problems)
    return bodies


# ---------------------------------------------------------------------------
# Images and references
# ---------------------------------------------------------------------------
_refs = {}


def image(orc, length, pitch, n):
    """(n chunks of `length` bytes at `pitch` as a bytearray, their digests back
    to back).  The digests are computed once per shape, for the largest n a
    test uses; smaller batches take the prefix."""
    img = orc.fill_synthetic(n * pitch, 977 * length + pitch, SEED)  # one stream of distinct words
    key = (length, pitch, n)
    if key not in _refs:
        _refs[key] = b"".join(orc.hash_chunks(img, length, pitch, nthreads=8))
        assert len(_refs[key]) == 20 * n
    return img, _refs[key]


def upload(torch, data):
    """`data` (a non-empty bytearray) in device memory, 16-byte aligned as the fixed-layout kernels need."""
    d = torch.frombuffer(data, dtype=torch.uint8).cuda()
    assert d.data_ptr() % 16 == 0
    return d


def plain(bt, torch, d, n, length, pitch, ref, label, shift=0):
    dig = Guarded(torch, n, 20, shift)
    assert dig.ptr % 4 == shift  # a misaligned digest buffer sends a fixed layout to the ragged kernel
    bt.chunks_dev(d.data_ptr(), n, length, pitch, dig.ptr)
    settle(torch, label, [("digests", dig, ref[:20 * n])])


def fused_compare(bt, torch, d, n, length, pitch, ref, with_digests, odd, label):
    """bt_sha1_verify_dev with every 7th expectation wrong (as column_cases
    does); odd: `expected` one byte and `ok` three bytes off their tensors'
    alignment (expected is read bytewise, ok is a byte array)."""
    exp = np.frombuffer(ref[:20 * n], dtype=np.uint8).copy()
    exp.reshape(n, 20)[::7, 0] ^= 1
    want_ok = (np.arange(n) % 7 != 0).astype(np.uint8)
    d_exp = torch.zeros(20 * n + 1, dtype=torch.uint8, device="cuda")
    d_exp[int(odd):int(odd) + 20 * n] = torch.from_numpy(exp).cuda()
    ok = Guarded(torch, n, 1, 3 if odd else 0)
    dig = Guarded(torch, n, 20)
    assert (d_exp.data_ptr() + int(odd)) % 2 == int(odd) and dig.ptr % 4 == 0
    bt.verify_dev(d.data_ptr(), n, length, pitch, d_exp.data_ptr() + int(odd), ok.ptr, dig.ptr if with_digests else None)
    settle(torch, label, [("ok", ok, want_ok.tobytes()), ("digests", dig, ref[:20 * n] if with_digests else None)])


def host_image(bt, orc, nfull, chunk_len, rem, label):
    """bt.chunks_host's call (bt_sha1_chunks_host: the staged pipeline, one
    launch_image per batch) on nfull chunks + rem bytes, the digests landing
    inside a host canary; compared with the oracle.  The run must have been a
    single batch with no column split, so that the one launch had nfull whole
    chunks and the tail chunk."""
    import ctypes
    img = orc.fill_synthetic(nfull * chunk_len + rem, 31 * nfull + rem, SEED)
    nch = nfull + 1
    out = np.full(20 * (nch + 2 * GUARD), SENT, dtype=np.uint8)
    src = (ctypes.c_uint8 * len(img)).from_buffer(img)
    got = bt.lib.bt_sha1_chunks_host(src, len(img), chunk_len, out.ctypes.data + 20 * GUARD)
    assert got == nch, (label, got, bt.last_error())
    s = bt.pipeline_stats()
    assert (s["batches"], s["chunks"], s["column_chunks"], s["feed"]) == (1, nch, 0, "staged"), (label, s)
    want = np.frombuffer(b"".join(orc.hash_chunks(img, chunk_len, nthreads=8)), dtype=np.uint8)
    body = out[20 * GUARD:20 * (GUARD + nch)].reshape(nch, 20)
    wrong = np.nonzero((body != want.reshape(nch, 20)).any(axis=1))[0]
    assert not len(wrong), (label, f"{len(wrong)} of {nch} digests differ, first {wrong[0]}")
    assert (out[:20 * GUARD] == SENT).all() and (out[20 * (GUARD + nch):] == SENT).all(), (label, "guards")


# ---------------------------------------------------------------------------
# 1. k_sha1_fixed in 256-thread workgroups
# ---------------------------------------------------------------------------
# NBUF = 3 ring slots of one 128-byte line: nmain = 3 * floor(len / 384) slots.
FIXED_SHAPES = [
    (0, 16), (55, 64), (56, 64),  # no main loop, no whole block; one and two padding blocks
    (64, 64), (383, 384),         # no main loop, 1 and 5 epilogue blocks (383: + 63 bytes, two padding blocks)
    (384, 384),                   # exactly one ring turn and nothing after
    (384, 640),                   # the same behind a pitch of len + 256
    (760, 768),                   # one turn + the largest epilogue: 5 blocks + 56 bytes
    (887, 896),                   # two turns + one block + 55 bytes
]
# chunks past 256 * cus: a partly filled last wave as wave 0, 1, 2 or 3 of the last block, and whole
# waves of it that return early
FIXED_KS = (0, 1, 63, 64, 65, 191, 192, 193, 255)


def assert_fixed_256(bt, cus, n):
    assert bt.kernel_name(n) == "k_sha1_fixed" and n >= 256 * cus, (bt.kernel_name(n), n, cus)


@pytest.mark.parametrize("length,pitch", FIXED_SHAPES, ids=[f"len{a}-pitch{b}" for a, b in FIXED_SHAPES])
def test_launch_forms_fixed_256_plain(bt, torch, oracle, cus, length, pitch):
    """chunks_dev at n = 256 * cus + k for every k of FIXED_KS: the whole
    cross product (a launch of these shapes is a few hundred microseconds),
    one image per shape."""
    img, ref = image(oracle, length, pitch, 256 * cus + max(FIXED_KS))
    d = upload(torch, img)
    with kernel_mode(bt, 3):
        for k in FIXED_KS:
            n = 256 * cus + k
            assert_fixed_256(bt, cus, n)
            plain(bt, torch, d, n, length, pitch, ref, ("fixed plain", length, pitch, k))


@pytest.mark.parametrize("length,pitch", [(56, 64), (760, 768)], ids=["len56", "len760"])
def test_launch_forms_fixed_256_fused_compare(bt, torch, oracle, cus, length, pitch):
    """verify_dev in the 256-thread form: exact verdicts, exact digests when
    asked for, nothing written to a digest buffer that was not passed, guards
    untouched; at k = 65 and 255 with `expected` and `ok` at odd addresses."""
    img, ref = image(oracle, length, pitch, 256 * cus + max(FIXED_KS))
    d = upload(torch, img)
    with kernel_mode(bt, 3):
        for k in (0, 65, 255):
            n = 256 * cus + k
            assert_fixed_256(bt, cus, n)
            for with_digests in (True, False):
                fused_compare(bt, torch, d, n, length, pitch, ref, with_digests, k != 0,
                              ("fixed verify", length, k, with_digests))


# nfull = 256 * cus + k: the tail wave is wave 0 of a fresh block (0, 1, 193 -- after a partly filled
# wave 3 -- and 255), wave 1 (64), wave 2 (65, 128) or wave 3 (192) beside waves of whole chunks
TAIL_KS = (0, 1, 64, 65, 128, 192, 193, 255)


@pytest.mark.parametrize("chunk_len", [64, 448])
def test_launch_forms_fixed_256_tail_wave(bt, oracle, cus, chunk_len):
    rems = (1, 55, 56, 63, chunk_len - 1)
    with kernel_mode(bt, 3):
        for i, k in enumerate(TAIL_KS):
            nfull = 256 * cus + k
            assert_fixed_256(bt, cus, nfull)
            # every k with two rems at 64-byte chunks (4 MiB images), one at 448 (29 MiB); every rem at both
            for rem in sorted({rems[i % 5], rems[(i + 3) % 5]} if chunk_len == 64 else {rems[i % 5]}):
                host_image(bt, oracle, nfull, chunk_len, rem, ("fixed tail", chunk_len, k, rem))


def test_launch_forms_fixed_256_clock_probe(bt, torch, oracle, cus):
    """The stamped build in 256-thread workgroups: digests exact, one stamp
    quadruple per wave that owns a chunk -- 4 * ceil(n / 64) words, none from
    the waves of the last block that return early -- and t1 > t0 in both clocks."""
    length, pitch, n = 760, 768, 256 * cus + 65
    img, ref = image(oracle, length, pitch, 256 * cus + max(FIXED_KS))
    d = upload(torch, img)
    waves = (n + 63) // 64
    with kernel_mode(bt, 3):
        assert_fixed_256(bt, cus, n)
        dig, st = Guarded(torch, n, 20), Guarded(torch, 4 * waves, 8)
        assert st.ptr % 8 == 0
        bt.clock_probe(d.data_ptr(), n, length, pitch, dig.ptr, st.ptr)
        got = settle(torch, "clock probe", [("digests", dig, ref[:20 * n]), ("stamps", st, WRITTEN)])
    s = got["stamps"].view(np.uint64).reshape(waves, 4)
    assert (s != np.uint64(int.from_bytes(bytes([SENT]) * 8, "little"))).all(), "a wave left its stamps unwritten"
    assert (s[:, 2] > s[:, 0]).all() and (s[:, 3] > s[:, 1]).all()


# ---------------------------------------------------------------------------
# 2. k_sha1_ragged in 256-thread workgroups
# ---------------------------------------------------------------------------
def pack(orc, rng, lens, seed):
    """One synthetic stream with message i at offs[i], 0 to 15 bytes of slack in front of each."""
    offs, pos = [], 0
    for ln in lens:
        pos += rng.randrange(0, 16)
        offs.append(pos)
        pos += ln
    assert {o % 16 for o in offs} == set(range(16))
    return orc.fill_synthetic(pos + 64, len(lens), seed), offs


def ragged(bt, torch, orc, lens, rng, label):
    """One ragged_dev batch: odd message offsets, the digests at an odd
    address, each message's digest from the oracle."""
    n = len(lens)
    blob, offs = pack(orc, rng, lens, SEED + n)
    d = upload(torch, blob)
    ot = torch.tensor(offs, dtype=torch.int64, device="cuda")
    lt = torch.tensor(lens, dtype=torch.int32, device="cuda")
    dig = Guarded(torch, n, 20, shift=1)
    assert dig.ptr % 2 == 1
    bt.ragged_dev(d.data_ptr(), ot.data_ptr(), lt.data_ptr(), n, dig.ptr)
    want = b"".join(orc.sha1(blob[o:o + ln]) for o, ln in zip(offs, lens))
    settle(torch, label, [("digests", dig, want)])


def test_launch_forms_ragged_256(bt, torch, oracle, cus):
    """ragged_dev past 256 * cus messages: lengths over absorb_ring's 0, 1, 2,
    3 and 4+ block cases and both of its leftover branches, every padding
    residue, every alignment."""
    n = 256 * cus + 65
    rng = random.Random(n)
    edges = [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 191, 192, 193, 200]
    lens = [rng.choice(edges + [rng.randrange(0, 400)]) for _ in range(n)]
    assert set(edges) <= set(lens) and max(lens) >= 320
    with ragged_mode(bt, "lanes"):
        # the ragged launcher shares the fixed-layout thresholds: neither the chain nor the latency kernel
        assert_fixed_256(bt, cus, n)
        ragged(bt, torch, oracle, lens, rng, "ragged 256")


def test_launch_forms_ragged_256_strided(bt, torch, oracle, cus):
    """chunks_dev with a pitch that is no multiple of 16 reaches the same
    kernel with offsets == nullptr: message i at i * pitch."""
    length, pitch, n = 200, 203, 256 * cus + 65
    img, ref = image(oracle, length, pitch, n)
    d = upload(torch, img)
    with ragged_mode(bt, "lanes"):
        assert_fixed_256(bt, cus, n)
        plain(bt, torch, d, n, length, pitch, ref, "ragged strided", shift=1)


# ---------------------------------------------------------------------------
# 3. Three-slot latency kernels in the product library
# ---------------------------------------------------------------------------
def assert_lat(bt, cus, n, tail, slots):
    """launch_lat: ceil(n / 64) workgroups + one for a tail chunk; 3 slots past `cus` of them."""
    grid = (n + 63) // 64 + (1 if tail else 0)
    assert bt.kernel_name(n + (1 if tail else 0)) == "k_sha1_lat", (bt.kernel_name(n), n)
    assert (3 if grid > cus else 2) == slots, (n, grid, cus, slots)


LAT_SHAPES = [
    (0, 16), (55, 64), (56, 64),  # nb_total = 1, 1, 2: R's loop takes its fallbacks on the first trip
    (64, 64), (119, 128), (120, 128),
    (64 * 5 + 63, 384),           # S's 4-deep ring wraps with nblocks % 4 == 1, then two padding blocks
    (64 * 8, 512),
]
LAT_NS = (1, 64, 100)  # chunks past 64 * cus


@pytest.mark.parametrize("length,pitch", LAT_SHAPES, ids=[f"len{a}" for a, _ in LAT_SHAPES])
def test_launch_forms_lat_3slot_plain(bt, torch, oracle, cus, length, pitch):
    img, ref = image(oracle, length, pitch, 64 * cus + max(LAT_NS))
    d = upload(torch, img)
    with kernel_mode(bt, LAT):
        for k in LAT_NS:
            n = 64 * cus + k
            assert (n + 63) // 64 > cus
            assert_lat(bt, cus, n, False, 3)
            plain(bt, torch, d, n, length, pitch, ref, ("lat plain", length, k))


@pytest.mark.parametrize("length,pitch", [(0, 16), (56, 64), (64 * 5 + 48, 64 * 5 + 48)], ids=["len0", "len56", "len368"])
def test_launch_forms_lat_3slot_fused_compare(bt, torch, oracle, cus, length, pitch):
    img, ref = image(oracle, length, pitch, 64 * cus + max(LAT_NS))
    d = upload(torch, img)
    with kernel_mode(bt, LAT):
        for k in (1, 100):
            n = 64 * cus + k
            assert_lat(bt, cus, n, False, 3)
            for with_digests in (True, False):
                fused_compare(bt, torch, d, n, length, pitch, ref, with_digests, k == 100,
                              ("lat verify", length, k, with_digests))


@pytest.mark.parametrize("chunk_len", [64, 448])
def test_launch_forms_lat_tail_chunk(bt, oracle, cus, chunk_len):
    """The tail chunk's workgroup in k_sha1_lat: nfull = 64 * cus, where that
    workgroup itself takes the grid from cus to cus + 1 and the launch from 2
    to 3 slots; one chunk more; and the 2-slot neighbour 64 * cus - 64."""
    with kernel_mode(bt, LAT):
        for nfull, slots in ((64 * cus, 3), (64 * cus + 1, 3), (64 * cus - 64, 2)):
            assert_lat(bt, cus, nfull, True, slots)
            for rem in (1, 55, 56, 63):
                host_image(bt, oracle, nfull, chunk_len, rem, ("lat tail", chunk_len, nfull, rem))


def recipe_lengths(rng, n):
    """Lengths for k_sha1_lat_ragged, one recipe per workgroup of 64 messages,
    cycled: 0 all < 56 bytes (nbmax == 1); 1 all < 120 with at least one >= 56
    (nbmax == 2); 2 all empty but a long lane 0; 3 all short but a long lane
    63; 4 mixed 0..1500.  The last, partly filled workgroup takes recipe 0
    (its lanes past n re-hash the last message)."""
    lens, kinds = [], set()
    for g in range((n + 63) // 64):
        m = min(64, n - 64 * g)
        kind = 0 if m < 64 else g % 5
        kinds.add(kind)
        if kind == 0:
            part = [rng.randrange(0, 56) for _ in range(m)]
        elif kind == 1:
            part = [rng.randrange(0, 120) for _ in range(m)]
            part[rng.randrange(m)] = rng.randrange(56, 120)
        elif kind == 2:
            part = [700] + [0] * (m - 1)
        elif kind == 3:
            part = [rng.randrange(0, 56) for _ in range(m - 1)] + [700]
        else:
            part = [rng.randrange(0, 1501) for _ in range(m)]
        lens += part
    assert kinds == set(range(5)) and n % 64 and max(lens[-(n % 64):]) < 56
    return lens


@pytest.mark.parametrize("slots", [3, 2])
def test_launch_forms_lat_ragged_short_workgroups(bt, torch, oracle, cus, slots):
    n = 64 * cus + 100 if slots == 3 else 600
    rng = random.Random(n)
    lens = recipe_lengths(rng, n)
    with ragged_mode(bt, "latr"):
        # btsha1_launch_ragged: the latency kernel's threshold, 3 slots past `cus` workgroups
        assert_lat(bt, cus, n, False, slots)
        ragged(bt, torch, oracle, lens, rng, ("lat ragged", slots))
