"""GPU: verify chunks of any length.

1. bt_sha1_ragged_verify_dev through every form of btsha1_launch_ragged_verify
   (ragged_verify_cases.py: chain, k_sha1_lat_ragged_verify with 2 and 3 slots,
   k_sha1_ragged_verify in 64- and 256-thread workgroups): lengths around every
   padding boundary mixed inside one workgroup, a workgroup of empty messages,
   offsets at every residue mod 16, `expected` / `ok` / digests at odd
   addresses behind canaries, every digest bit as the only difference once,
   true digests in every run, the verdicts unchanged without a digest buffer.
2. verify_dev and chunks_dev keep their answers.  (btsha1_launch_chain's refusal
   of `ok` with offsets or a tail is not reachable from the C ABI: verify_dev
   passes neither, and btsha1_launch_fixed refuses a tail with `ok` first.)
3. The ragged verifier: short chunks, planted mismatches, a released slot, the
   stats; full chunks only take the classic launch; a classic verifier still
   refuses a short commit.
4. verify-stream on a file that ends in a short chunk, in its modes.
"""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import ragged_verify_cases as rv
import test_gpu_launch_forms as lf
import verdict_cases as vc
from conftest import PKG, load_btsha1

pytestmark = pytest.mark.gpu
CHUNK = 512 * 1024


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
# 1. bt_sha1_ragged_verify_dev
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", rv.FORMS)
def test_ragged_verify_every_form(bt, torch, oracle, cus, form):
    before = (bt.set_chain_batch(7), bt.set_latency_batch(9))
    bt.set_chain_batch(before[0]), bt.set_latency_batch(before[1])
    lens, launches = rv.run_form(bt, torch, lf, vc, oracle, form, cus)
    assert launches == 3 and set(lens) >= set(rv.SHORT)
    assert (4097 in lens) == (form != "lanes256")
    assert all(ln == 0 for ln in lens[64:128])  # the workgroup of empty messages
    # the settings are back where they were
    assert (bt.set_chain_batch(before[0]), bt.set_latency_batch(before[1])) == before


def test_ragged_verify_matches_ragged_dev_and_takes_no_messages(bt, torch, oracle):
    """Default settings (300 messages: the chain kernel on a full MI355X):
    ragged_verify_dev's digests are ragged_dev's, and n == 0 touches nothing."""
    n = 300
    blob, offs, lens, want = rv.batch(oracle, n)
    d = lf.upload(torch, blob)
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    d_exp = torch.frombuffer(bytearray(want), dtype=torch.uint8).cuda()
    plain, ok, dig = lf.Guarded(torch, n, 20, 1), lf.Guarded(torch, n, 1), lf.Guarded(torch, n, 20, 1)
    bt.ragged_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, plain.ptr)
    bt.ragged_verify_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, d_exp.data_ptr(), ok.ptr, dig.ptr)
    lf.settle(torch, "default settings", [("ragged_dev", plain, want), ("ok", ok, bytes([1]) * n),
                                          ("digests", dig, want)])
    ok0, dig0 = lf.Guarded(torch, 4, 1), lf.Guarded(torch, 4, 20)
    bt.ragged_verify_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), 0, d_exp.data_ptr(), ok0.ptr, dig0.ptr)
    lf.settle(torch, "n == 0", [("ok", ok0, None), ("digests", dig0, None)])


# ---------------------------------------------------------------------------
# 2. The fixed-layout calls keep their answers
# ---------------------------------------------------------------------------
def test_fixed_layout_calls_keep_their_answers(bt, torch, oracle):
    length, pitch, n = 760, 768, 168
    img, ref = lf.image(oracle, length, pitch, n)
    d = lf.upload(torch, img)
    assert bt.kernel_name(n) == "k_sha1_chain"
    lf.plain(bt, torch, d, n, length, pitch, ref, "chunks_dev")
    for with_digests in (True, False):
        lf.fused_compare(bt, torch, d, n, length, pitch, ref, with_digests, True, ("verify_dev", with_digests))
    # verify_dev still takes whole chunks in the fast layout only
    with pytest.raises(bt.BtSha1Error, match="verify needs a 16-byte aligned layout"):
        bt.verify_dev(d.data_ptr() + 1, 1, length, pitch, d.data_ptr(), d.data_ptr())


# ---------------------------------------------------------------------------
# 3. The ragged verifier
# ---------------------------------------------------------------------------
def _chunk(orc, length, k):
    return bytes(orc.fill_synthetic(length, 100 + k, 0x7A66ED))


def test_ragged_verifier_short_chunks(bt, oracle):
    """max_chunk_len 64 KiB + 8 (slots at a pitch of 64 KiB + 16), one batch of
    8 slots: lengths 1, 63, 64, 65536 and the full length, two planted
    mismatches, one slot released in the middle."""
    full = 65536 + 8
    plan = [(1, True), (63, True), (64, True), ("release", None), (65536, True), (full, True), (full, False), (63, False)]
    v = bt.Verifier(chunk_len=full, batch=8, nstreams=2, ragged=True)
    try:
        slots = [v.slot() for _ in plan]
        assert [b - a for a, b in zip(slots, slots[1:])] == [full + 8] * 7  # the 16-byte pitch
        want = []
        for k, (ln, good) in reversed(list(enumerate(plan))):  # settled in any order
            if ln == "release":
                v.release(slots[k])
                continue
            data = _chunk(oracle, ln, k)
            ctypes.memmove(slots[k], data, ln)
            dg = hashlib.sha1(data).digest()
            exp = dg if good else bytes([dg[0]]) + bytes([dg[1] ^ 0x10]) + dg[2:]
            v.commit(slots[k], exp, k, ln)
            want.append((k, good, dg))
        assert v.stats()["batches"] == 1  # the eighth settled slot launched the batch
        got = v.drain()
        assert sorted(got) == sorted(want), got
        assert v.stats() == {"batches": 1, "ragged_batches": 1, "chunks": 7, "short_chunks": 5, "released": 1}
        for bad_len in (0, full + 1):
            with pytest.raises(bt.BtSha1Error, match=f"chunk of {bad_len} bytes, ragged verifier takes 1 .. {full}"):
                v.submit(b"x" * bad_len, bytes(20), 1)
        # a second round through submit, lengths in another order
        want = []
        for k, ln in enumerate((full, 1, 65536, 63, 64)):
            data = _chunk(oracle, ln, 50 + k)
            v.submit(data, hashlib.sha1(data).digest(), 50 + k)
            want.append((50 + k, True, hashlib.sha1(data).digest()))
        assert v.drain() == want and v.pending() == 0
        assert v.stats() == {"batches": 2, "ragged_batches": 2, "chunks": 12, "short_chunks": 9, "released": 1}
    finally:
        v.close()


def test_ragged_verifier_full_chunks_take_the_classic_launch(bt, oracle):
    full = 65536
    v = bt.Verifier(chunk_len=full, batch=8, nstreams=2, ragged=True)
    try:
        want = []
        for k in range(11):  # a full batch and one of three, flushed by drain
            data = _chunk(oracle, full, k)
            dg = hashlib.sha1(data).digest()
            v.submit(data, dg if k != 4 else bytes(19) + b"\x01", k)
            want.append((k, k != 4, dg))
        assert v.drain() == want
        assert v.stats() == {"batches": 2, "ragged_batches": 0, "chunks": 11, "short_chunks": 0, "released": 0}
        # one short chunk turns its batch, and only it, into a ragged one
        data = _chunk(oracle, full - 1, 99)
        v.submit(data, hashlib.sha1(data).digest(), 99)
        assert v.drain() == [(99, True, hashlib.sha1(data).digest())]
        assert v.stats() == {"batches": 3, "ragged_batches": 1, "chunks": 12, "short_chunks": 1, "released": 0}
    finally:
        v.close()


def test_classic_verifier_still_refuses_a_short_commit(bt, oracle):
    v = bt.Verifier(chunk_len=65536, batch=8, nstreams=2)
    try:
        with pytest.raises(bt.BtSha1Error, match="verifier: chunk of 100 bytes, verifier built for 65536"):
            v.commit(v.slot(), bytes(20), 1, 100)
        with pytest.raises(bt.BtSha1Error, match="verifier: chunk of 100 bytes, verifier built for 65536"):
            v.submit(b"x" * 100, bytes(20), 2)
        s = v.stats()
        assert (s["chunks"], s["ragged_batches"]) == (0, 0)
    finally:
        v.close()


# ---------------------------------------------------------------------------
# 4. verify-stream
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_file(tmp_path_factory):
    """A 3 x 512 KiB + 1000-byte file and the chunks file make-chunks writes for it."""
    d = tmp_path_factory.mktemp("ragged_stream")
    data = os.urandom(3 * CHUNK + 1000)
    p = d / "data.bin"
    p.write_bytes(data)
    out = subprocess.run([os.path.join(PKG, "bin", "make-chunks"), str(p)], capture_output=True, check=True).stdout
    lines = out.decode().splitlines()
    assert len(lines) == 4 and lines[3].split()[1] == hashlib.sha1(data[3 * CHUNK:]).hexdigest()
    ck = d / "data.chunks"
    ck.write_bytes(out)
    return d, data, p, ck


@pytest.mark.parametrize("mode", [[], ["-g", "2", "-t"], ["-z", "-b", "2", "-r", "2"]], ids=["default", "g2t", "zcopy"])
def test_verify_stream_verifies_the_short_last_chunk(tail_file, mode):
    _, _, p, ck = tail_file
    exe = os.path.join(PKG, "bin", "verify-stream")
    r = subprocess.run([exe, *mode, str(p), str(ck)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    per_round = 4
    rounds = 2 if "-r" in mode else 1
    assert f'"chunks": {per_round * rounds}, "ok": {per_round * rounds}, "failed": 0' in r.stdout, r.stdout
    assert "Verification failed" not in r.stdout


def test_verify_stream_fails_only_a_corrupted_tail(tail_file):
    d, data, _, ck = tail_file
    bad = bytearray(data)
    bad[3 * CHUNK + 999] ^= 0x01  # the file's last byte
    q = d / "corrupt.bin"
    q.write_bytes(bad)
    exe = os.path.join(PKG, "bin", "verify-stream")
    r = subprocess.run([exe, str(q), str(ck)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert '"chunks": 4, "ok": 3, "failed": 1' in r.stdout, r.stdout
    assert r.stdout.count("Verification failed!") == 1
    assert f"Hash: {hashlib.sha1(bytes(bad[3 * CHUNK:])).hexdigest()}\n" in r.stdout
