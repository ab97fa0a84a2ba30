"""GPU: every bit of every fused compare.

The library's product is a verdict -- "this chunk's SHA-1 equals the expected
one" -- and sha1_kernels.hip decides it at four sites: store_digest<true>
(five word compares; k_sha1_fixed and k_sha1_lat in all forms) and the 20-byte
loops of k_sha1_chain<false, true>, k_sha1_resume<true> and
k_sha1_resume_table<true>.  Every other test plants its mismatch in bit 0 of
byte 0 or expects all zeros, which a compare of 16 bytes, a dropped mask or a
wrong shift would pass.  Here each path runs the verdict batch of
verdict_cases.py: 168 messages, expectation i < 160 differing from the true
digest in bit i alone, the last 8 exact -- so every one of the 160 bit
positions must by itself turn a verdict to 0 -- and then the same messages
with 168 exact expectations, which must all give 1 (a compare that always
fails, a stale ok).  Where a path returns digests they must be the true ones
in both runs, never the expectations.  A failure names the digest bits whose
flip was accepted.

Paths: 1 k_sha1_chain (verify_dev, default knobs), 2 k_sha1_lat with 2 and 3
LDS slots, 3 k_sha1_fixed in 64- and 256-thread workgroups, 4 k_sha1_resume
over 168 finishing entries (resume_dev), 5 its single-message form
(btsha1.Receiver), 6 k_sha1_resume_table with the host's copy of the
expectation into the control block (btsha1.Intake), 7 the staging of
`expected` through the verifier's batches (btsha1.Verifier).  Each asserts the
form it means to hit first.  Outputs of the device-pointer paths lie inside
sentinel-guarded buffers (test_gpu_launch_forms.Guarded / settle).

Left out: the column LAST compare.  It is store_digest<true>, the code paths 2
and 3 run, and test_gpu_columns.py pins its planted pattern.
"""
import ctypes

import numpy as np
import pytest

import test_gpu_launch_forms as lf
import verdict_cases as vc
from conftest import load_btsha1

pytestmark = pytest.mark.gpu

Guarded, settle, WRITTEN, LAT = lf.Guarded, lf.settle, lf.WRITTEN, lf.LAT
SHAPES = [(56, 64), (760, 768)]  # two padding blocks and no whole one; a ring turn, 5 epilogue blocks and 56 bytes
SHAPE_IDS = ["len56", "len760"]


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


# ---------------------------------------------------------------------------
# Paths 1 to 3: bt_sha1_verify_dev
# ---------------------------------------------------------------------------
def verify_runs(bt, torch, d, n, length, pitch, ref, label):
    """The verdict batch on the last 168 of n chunks: planted with and without
    a digest buffer, then exact.  `expected` and `ok` at odd addresses."""
    want_dig = ref[:20 * n]
    for exact, with_digests in ((False, True), (False, False), (True, True)):
        exp = vc.expectations(want_dig, exact)
        d_exp = torch.zeros(20 * n + 1, dtype=torch.uint8, device="cuda")
        d_exp[1:] = torch.from_numpy(exp.reshape(-1)).cuda()
        ok, dig = Guarded(torch, n, 1, 3), Guarded(torch, n, 20)
        assert (d_exp.data_ptr() + 1) % 2 == 1 and ok.ptr % 2 == 1 and dig.ptr % 4 == 0
        bt.verify_dev(d.data_ptr(), n, length, pitch, d_exp.data_ptr() + 1, ok.ptr, dig.ptr if with_digests else None)
        run = (label, "exact" if exact else "planted", "digests" if with_digests else "no digest buffer")
        got = settle(torch, run, [("ok", ok, WRITTEN), ("digests", dig, want_dig if with_digests else None)])
        bad = vc.problems(got["ok"], exact)
        assert not bad, (run, bad)


@pytest.mark.parametrize("length,pitch", SHAPES, ids=SHAPE_IDS)
def test_verdict_bits_chain_kernel(bt, torch, oracle, length, pitch):
    """Path 1: verify_dev with default knobs sends 168 chunks to k_sha1_chain<false, true>."""
    n = vc.N
    assert bt.kernel_name(n) == "k_sha1_chain", bt.kernel_name(n)
    img, ref = lf.image(oracle, length, pitch, n)
    verify_runs(bt, torch, lf.upload(torch, img), n, length, pitch, ref, ("chain", length))


@pytest.mark.parametrize("length,pitch", SHAPES, ids=SHAPE_IDS)
def test_verdict_bits_latency_kernel(bt, torch, oracle, cus, length, pitch):
    """Path 2: store_digest<true> behind k_sha1_lat with 2 slots (n = 168) and
    with 3 (64 * CUs + 168, the batch on the last three workgroups, the last
    one holding 40 chunks)."""
    nmax = 64 * cus + vc.N
    img, ref = lf.image(oracle, length, pitch, nmax)
    d = lf.upload(torch, img)
    with lf.kernel_mode(bt, LAT):
        for n, slots in ((vc.N, 2), (nmax, 3)):
            lf.assert_lat(bt, cus, n, False, slots)
            verify_runs(bt, torch, d, n, length, pitch, ref, ("lat", length, slots))


@pytest.mark.parametrize("length,pitch", SHAPES, ids=SHAPE_IDS)
def test_verdict_bits_hot_kernel(bt, torch, oracle, cus, length, pitch):
    """Path 3: store_digest<true> behind k_sha1_fixed in 64-thread workgroups
    (n = 168) and in 256-thread ones (256 * CUs + 168)."""
    nmax = 256 * cus + vc.N
    img, ref = lf.image(oracle, length, pitch, 256 * cus + max(lf.FIXED_KS))  # the launch-form tests' image
    d = lf.upload(torch, img)
    with lf.kernel_mode(bt, 3):
        assert bt.kernel_name(vc.N) == "k_sha1_fixed" and vc.N < 256 * cus, (bt.kernel_name(vc.N), cus)
        verify_runs(bt, torch, d, vc.N, length, pitch, ref, ("fixed 64", length))
        lf.assert_fixed_256(bt, cus, nmax)
        verify_runs(bt, torch, d, nmax, length, pitch, ref, ("fixed 256", length))


# ---------------------------------------------------------------------------
# Path 4: bt_sha1_resume_dev
# ---------------------------------------------------------------------------
RESUME_TAILS = (1, 55, 56, 63, 64, 119, 120, 129)
RESUME_PREFIX = 64


def test_verdict_bits_resume_kernel(bt, torch, oracle):
    """Path 4: 168 finishing entries of k_sha1_resume<true> in one launch.
    Each message is a 64-byte prefix, present only as the chaining state the
    oracle computes for it (never the IV), and a tail of 1 .. 129 bytes at an
    unaligned offset; `expected`, `ok` and the digests at odd addresses."""
    n = vc.N
    lens = [RESUME_TAILS[i % len(RESUME_TAILS)] for i in range(n)]
    msgs = [bytes(oracle.fill_synthetic(RESUME_PREFIX + ln, i, 0x7E5)) for i, ln in enumerate(lens)]
    want_dig = b"".join(oracle.sha1(m) for m in msgs)
    states = [oracle.compress_blocks(vc.IV, m[:RESUME_PREFIX]) for m in msgs]
    assert all(tuple(s) != vc.IV for s in states)
    blob, offs, pos = bytearray(), [], 0
    for i, m in enumerate(msgs):
        pad = 1 + (5 * i) % 15
        blob += bytes([0xEE]) * pad + m[RESUME_PREFIX:]
        offs.append(pos + pad)
        pos += pad + lens[i]
    blob += bytes(64)
    assert {o % 16 for o in offs} == set(range(16))
    d = lf.upload(torch, blob)
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    d_tot = torch.tensor([RESUME_PREFIX + ln for ln in lens], dtype=torch.int64, device="cuda")
    st_bytes = np.array(states, dtype=np.uint32).reshape(-1).tobytes()
    for exact in (False, True):
        exp = vc.expectations(want_dig, exact)
        d_exp = torch.zeros(20 * n + 1, dtype=torch.uint8, device="cuda")
        d_exp[1:] = torch.from_numpy(exp.reshape(-1)).cuda()
        st = Guarded(torch, 5 * n, 4)
        st.buf[st.lead:st.lead + st.used] = torch.frombuffer(bytearray(st_bytes), dtype=torch.uint8).cuda()
        ok, dig = Guarded(torch, n, 1, 3), Guarded(torch, n, 20, 1)
        assert (d_exp.data_ptr() + 1) % 2 == 1 and ok.ptr % 2 == 1 and dig.ptr % 2 == 1 and st.ptr % 4 == 0
        bt.resume_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_tot.data_ptr(), n, st.ptr, dig.ptr,
                      d_exp.data_ptr() + 1, ok.ptr)
        run = ("resume", "exact" if exact else "planted")
        # a finish does not write its state back
        got = settle(torch, run, [("ok", ok, WRITTEN), ("digests", dig, want_dig), ("states", st, st_bytes)])
        bad = vc.problems(got["ok"], exact)
        assert not bad, (run, bad)


# ---------------------------------------------------------------------------
# Paths 5 to 7: the host objects
# ---------------------------------------------------------------------------
OBJ_CHUNK = 4096
_chunks = {}


def object_chunks(orc):
    """(168 chunks of 4096 bytes, their digests back to back), computed once."""
    if not _chunks:
        img = orc.fill_synthetic(vc.N * OBJ_CHUNK, 4096, 0xB175)
        _chunks["c"] = [bytes(img[i * OBJ_CHUNK:(i + 1) * OBJ_CHUNK]) for i in range(vc.N)]
        _chunks["d"] = b"".join(orc.hash_chunks(img, OBJ_CHUNK, nthreads=8))
    return _chunks["c"], _chunks["d"]


def check_verdicts(results, want_dig, exact, run):
    """results: [(tag, ok, digest)] in any order, tag = message index."""
    assert sorted(t for t, _, _ in results) == list(range(vc.N)), (run, "tags", sorted(t for t, _, _ in results))
    by_tag = {t: (ok, dg) for t, ok, dg in results}
    bad = vc.problems([by_tag[i][0] for i in range(vc.N)], exact)
    bad += vc.digest_problems(b"".join(by_tag[i][1] for i in range(vc.N)), want_dig, "digests (by tag)")
    assert not bad, (run, bad)


def test_verdict_bits_receiver(bt, oracle):
    """Path 5: k_sha1_resume<true> in its single-message form, one launch per
    commit: 168 chunks through 4 slots, the verdicts taken as slots free up."""
    chunks, want_dig = object_chunks(oracle)
    rx = bt.Receiver(chunk_len=OBJ_CHUNK, nslots=4)
    try:
        for exact in (False, True):
            exp = vc.expectations(want_dig, exact)
            before, got = rx.stats(), []
            for i, c in enumerate(chunks):
                if rx.pending() == 4:  # every slot waits for its verdict
                    got += rx.drain()
                rx.receive(c, exp[i].tobytes(), i)
                got += rx.poll()
            got += rx.drain()
            s = rx.stats()
            # default stride 64 KiB > chunk_len: nothing advanced, one finishing launch per chunk
            assert (s["launches"] - before["launches"], s["advance_launches"] - before["advance_launches"]) == (vc.N, 0)
            check_verdicts(got, want_dig, exact, ("receiver", "exact" if exact else "planted"))
    finally:
        rx.close()


def test_verdict_bits_intake(bt, oracle):
    """Path 6: k_sha1_resume_table<true>: 168 slots committed, then ONE poll
    whose kick finishes them all in a single launch; the expectation reaches
    the kernel through the host's copy into each slot's control block."""
    chunks, want_dig = object_chunks(oracle)
    ix = bt.Intake(chunk_len=OBJ_CHUNK, nslots=vc.N)
    try:
        for exact in (False, True):
            exp = vc.expectations(want_dig, exact)
            for i, c in enumerate(chunks):
                p = ix.slot()
                ctypes.memmove(p, c, OBJ_CHUNK)
                ix.commit(p, exp[i].tobytes(), i)
            before = ix.stats()
            got = ix.poll()
            got += ix.drain()
            s = ix.stats()
            delta = {k: s[k] - before[k] for k in ("launches", "entries", "advanced_bytes", "deferred")}
            run = ("intake", "exact" if exact else "planted")
            assert delta == {"launches": 1, "entries": vc.N, "advanced_bytes": 0, "deferred": 0}, (run, delta)
            assert s["max_entries"] == vc.N, (run, s)
            check_verdicts(got, want_dig, exact, run)
    finally:
        ix.close()


def test_verdict_bits_verifier(bt, oracle):
    """Path 7: 168 submits through batches of 64 (two full, one of 40 flushed
    by drain): `expected` is staged per batch before the fused compare reads it."""
    chunks, want_dig = object_chunks(oracle)
    for exact in (False, True):
        exp = vc.expectations(want_dig, exact)
        v = bt.Verifier(chunk_len=OBJ_CHUNK, batch=64, nstreams=2)
        try:
            for i, c in enumerate(chunks):
                v.submit(c, exp[i].tobytes(), i)
            got = v.drain()
            assert v.pending() == 0
        finally:
            v.close()
        check_verdicts(got, want_dig, exact, ("verifier", "exact" if exact else "planted"))
