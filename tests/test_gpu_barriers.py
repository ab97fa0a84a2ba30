"""GPU: the barrier-accounting build (`make dbgbar`) on the shapes that stress
the latency kernels' barrier counts.

k_sha1_lat, k_sha1_chain and k_sha1_lat_ragged split each chain between a
loader/schedule wave S and a round wave R that meet at s_barrier from
DIFFERENT call sites; s_barrier counts waves, so the kernels are correct only
while both waves execute exactly the count the invariant in sha1_kernels.hip
("Barrier accounting") predicts -- and that count derives from the padding
block count of sha.c:536-543 (one padding block, or two when the tail holds
r >= 56 bytes).  The -DBT_SHA1_DEBUG_BARRIERS build counts each wave's
barriers and tallies {waves checked, barriers executed, misses}.

The child process loads that build (BT_SHA1_LIB) and runs, each pinned to its
kernel: tails with r >= 56 and r < 56, the chain kernel at 63/64/65 and
128/129 blocks (its 64-block loader batches), the streaming API's midstate
launches, the 2- and 3-slot forms of k_sha1_lat (1 and > 1 workgroups per CU)
incl. the fused verify, an image tail and chunks of one or two blocks in all
(0, 55, 56 and 64 bytes), and ragged batches whose longest message sits in the
LAST lane of its workgroup or whose workgroups hold only messages of one or
two blocks.  For every case it checks
the digests against the oracle, zero misses, and the EXACT wave and barrier
totals computed here from the invariant -- so the tallies prove the counting
build is what ran, and which kernel (S/R pairs per workgroup) ran.
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import PKG, REPO

pytestmark = pytest.mark.gpu
DBG_LIB = os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so")


def nb_total(length):
    """Blocks of one message incl. MD padding (sha.c:536-543)."""
    return (length >> 6) + (2 if (length & 63) >= 56 else 1)


def _child():
    import torch
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, PKG)
    import btsha1 as bt
    import py_oracle as orc

    assert torch.cuda.is_available()
    assert os.path.samefile(bt.LIB_PATH, DBG_LIB), bt.LIB_PATH
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bt.debug_barrier_stats(reset=True)
    results = []

    def pin(chain, lat):
        bt.set_chain_batch(1 << 62 if chain else 0)
        bt.set_latency_batch(1 << 62 if lat else 0)

    def record(name, want, ok):
        got = bt.debug_barrier_stats(reset=True)
        results.append({"case": name, "want": list(want), "got": list(got), "digests_ok": bool(ok)})

    def dev(data):
        t = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
        if data:
            t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        return t

    def fixed(name, n, length, pitch, kernel, seed, verify=False):
        data = bytes(orc.fill_synthetic(n * pitch, seed, 0xBA77))
        d = dev(data)
        out = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
        assert bt.kernel_name(n) == kernel, (name, bt.kernel_name(n))
        want_dig = b"".join(orc.sha1(data[i * pitch:i * pitch + length]) for i in range(n))
        if verify:
            exp = bytearray(want_dig)
            for i in range(0, n, 7):
                exp[20 * i] ^= 1  # every 7th chunk must fail util.c:313's compare
            e = dev(bytes(exp))
            ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
            bt.verify_dev(d.data_ptr(), n, length, pitch, e.data_ptr(), ok.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            good = [int(x) for x in ok.cpu()] == [0 if i % 7 == 0 else 1 for i in range(n)]
        else:
            bt.chunks_dev(d.data_ptr(), n, length, pitch, out.data_ptr())
            torch.cuda.synchronize()
            good = True
        good = good and bytes(out.cpu().numpy().tobytes()) == want_dig
        if kernel == "k_sha1_chain":
            per = 2 * ((nb_total(length) + 63) // 64 + 1)
            want = (2 * n, n * per)
        else:
            grid = (n + 63) // 64
            slots = 3 if grid > cus else 2
            want = (2 * grid, 2 * grid * (nb_total(length) + slots - 1))
        record(name, want, good)

    # ---- k_sha1_chain: one two-wave workgroup per message, 64-block batches
    pin(chain=True, lat=True)
    for k, length in enumerate([62 * 64, 63 * 64, 64 * 64, 61 * 64 + 60, 62 * 64 + 56, 63 * 64 + 57,
                                127 * 64, 127 * 64 + 60, 55, 56, 0]):
        pitch = (length + 15) // 16 * 16 or 16
        fixed(f"chain len={length} nb={nb_total(length)}", 3, length, pitch, "k_sha1_chain", 100 + k)
    fixed("chain verify", 5, 64 * 64, 64 * 64, "k_sha1_chain", 120, verify=True)
    # image with a short last chunk (the make_chunks tail rides in the same launch)
    img = bytes(orc.fill_synthetic(5 * 4096 + 4000, 130, 0xBA77))
    got = bt.chunks_host(img, 4096)
    want_dig = [orc.sha1(img[i:i + 4096]) for i in range(0, len(img), 4096)]
    record("chain image + tail", (2 * 6, 5 * 2 * ((nb_total(4096) + 63) // 64 + 1) + 2 * ((nb_total(4000) + 63) // 64 + 1)),
           got == want_dig)
    # drop-ins: shahash (chain kernel) and the SHA1Update / SHA1Final midstates
    for length in (63 * 64 + 60, 64 * 64 + 56):
        msg = bytes(orc.fill_synthetic(length, 140 + length, 0xBA77))
        ok = bt.shahash(msg) == orc.sha1(msg)
        record(f"shahash len={length}", (2, 2 * ((nb_total(length) + 63) // 64 + 1)), ok)
    for nb in (63, 64, 65, 129):
        msg = bytes(orc.fill_synthetic(64 * nb, 150 + nb, 0xBA77))
        ok = bt.Sha1().update(msg).final() == orc.sha1(msg)
        # update: one midstate launch of nb blocks; final: one padding block
        record(f"SHA1Update {nb} blocks + SHA1Final", (4, 2 * ((nb + 63) // 64 + 1) + 2 * 2), ok)

    # ---- k_sha1_lat: 64 chunks per two-wave workgroup
    pin(chain=False, lat=True)
    fixed("lat 2-slot r=56", 100, 4096 + 56, 4160, "k_sha1_lat", 200)
    fixed("lat 2-slot r=40", 130, 1000, 1008, "k_sha1_lat", 201)
    fixed("lat 2-slot r=0 verify", 100, 4096, 4096, "k_sha1_lat", 202, verify=True)
    fixed("lat 3-slot r=60", 64 * cus + 64, 1024 + 60, 1088, "k_sha1_lat", 203)
    fixed("lat 3-slot odd count r=63", 64 * cus + 1, 64 * 3 + 63, 256, "k_sha1_lat", 204)
    img = bytes(orc.fill_synthetic(100 * 1024 + 1020, 205, 0xBA77))
    got = bt.chunks_host(img, 1024)
    want_dig = [orc.sha1(img[i:i + 1024]) for i in range(0, len(img), 1024)]
    record("lat image + tail r=60", (6, 2 * 2 * (nb_total(1024) + 1) + 2 * (nb_total(1020) + 1)), got == want_dig)
    # one and two blocks in all (nb_total = 1, 1, 2, 2): at 3 slots R's loop takes its b + 1 / b + 2
    # fallbacks on the first trip and S's closing barriers pair with R's opening ones
    fixed("lat 3-slot len=0", 64 * cus + 1, 0, 16, "k_sha1_lat", 206)
    fixed("lat 3-slot len=55", 64 * cus + 1, 55, 64, "k_sha1_lat", 207)
    fixed("lat 3-slot len=56", 64 * cus + 1, 56, 64, "k_sha1_lat", 208)
    fixed("lat 3-slot len=64", 64 * cus + 1, 64, 64, "k_sha1_lat", 209)
    fixed("lat 2-slot len=0", 100, 0, 16, "k_sha1_lat", 210)

    # ---- k_sha1_lat_ragged: the wave runs to its longest message
    pin(chain=False, lat=True)
    import random

    def longest_in_lane_63(rng, n):
        lens = [rng.randrange(0, 1500) for _ in range(n)]
        for g in range(0, n, 64):
            last = min(g + 63, n - 1)
            lens[last] = 1600 + 60 if (g // 64) % 2 else 1600 + 20  # longest, r >= 56 on every other group
        return lens

    def short_workgroups(rng, n):
        """Workgroups of messages under 56 bytes (nbmax == 1) alternating with
        workgroups under 120 bytes that hold one of 56 or more (nbmax == 2)."""
        lens = []
        for g in range(0, n, 64):
            m = min(64, n - g)
            if (g // 64) % 2:
                part = [rng.randrange(0, 120) for _ in range(m)]
                part[rng.randrange(m)] = rng.randrange(56, 120)
            else:
                part = [rng.randrange(0, 56) for _ in range(m)]
            lens += part
        return lens

    for name, n, seed, recipe in (("lat_ragged 2-slot", 600, 300, longest_in_lane_63),
                                  ("lat_ragged 3-slot", 64 * cus + 100, 301, longest_in_lane_63),
                                  ("lat_ragged 3-slot nbmax 1 and 2", 64 * cus + 100, 302, short_workgroups),
                                  ("lat_ragged 2-slot nbmax 1 and 2", 600, 303, short_workgroups)):
        rng = random.Random(seed)
        lens = recipe(rng, n)
        blob, offs = bytearray(), []
        for i, ln in enumerate(lens):
            blob += bytes(i % 5)  # odd alignments
            offs.append(len(blob))
            blob += bytes(orc.fill_synthetic(ln, 1000 * i, seed))
        d = dev(bytes(blob))
        o = torch.tensor(offs, dtype=torch.int64, device="cuda")
        ln_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
        out = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
        bt.ragged_dev(d.data_ptr(), o.data_ptr(), ln_t.data_ptr(), n, out.data_ptr())
        torch.cuda.synchronize()
        good = bytes(out.cpu().numpy().tobytes()) == b"".join(
            orc.sha1(bytes(blob[offs[i]:offs[i] + lens[i]])) for i in range(n))
        grid = (n + 63) // 64
        slots = 3 if grid > cus else 2
        bars = 0
        for g in range(grid):
            idx = [min(g * 64 + j, n - 1) for j in range(64)]  # lanes past n re-hash message n-1
            bars += 2 * (max(nb_total(lens[i]) for i in idx) + slots - 1)
        record(name, (2 * grid, bars), good)
    print("BARRIER_RESULTS " + json.dumps(results), flush=True)


def test_barrier_accounting_build_matches_invariant():
    assert os.path.exists(DBG_LIB), "build_variants/dbgbar/libbtsha1.so missing: run `make dbgbar` first"
    env = dict(os.environ, BT_SHA1_LIB=DBG_LIB, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "child"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BARRIER_RESULTS ")]
    assert len(line) == 1, r.stdout[-2000:]
    results = json.loads(line[0].split(" ", 1)[1])
    assert len(results) == 34
    bad = [c for c in results if not c["digests_ok"] or c["got"][2] != 0 or c["got"][:2] != c["want"]]
    assert not bad, bad


def _child_columns():
    import ctypes

    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, PKG)
    import btsha1 as bt
    import column_cases as cc
    import py_oracle as orc

    assert torch.cuda.is_available()
    assert os.path.samefile(bt.LIB_PATH, DBG_LIB), bt.LIB_PATH
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bt.debug_barrier_stats(reset=True)
    results = []

    def record(name, want, problems):
        got = bt.debug_barrier_stats(reset=True)
        results.append({"case": name, "want": list(want), "got": list(got), "digests_ok": not problems,
                        "problems": problems})

    # ---- one launch at a time: the small shapes first, so a miscount shows at 6 MiB, not at 1 GiB
    for case in cc.cases(cus):
        cc.run_case(bt, torch, orc, case,
                    lambda label, n, width, part, bad: record(label, cc.barrier_want(n, width, part, cus), bad))

    # ---- whole split batches through the public verifier
    def verifier(name, chunk_len, batch):
        parts, width = 8, chunk_len // 8
        assert chunk_len % (64 * parts) == 0
        img = bytearray(batch * chunk_len)
        view = np.frombuffer(img, dtype=np.uint64)
        view[:] = np.arange(view.size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(chunk_len)
        ref = orc.hash_chunks(img, chunk_len, nthreads=8)
        v = bt.Verifier(chunk_len=chunk_len, batch=batch, nstreams=2)
        want = []
        for k in range(batch):
            p = v.slot()
            if k % 211 == 5:  # an aborted download: hashed with the batch, no verdict
                v.release(p)
                continue
            ctypes.memmove(p, (ctypes.c_uint8 * chunk_len).from_buffer(img, k * chunk_len), chunk_len)
            v.commit(p, ref[k] if k % 97 else bytes(20), tag=k)
            want.append((k, k % 97 != 0, ref[k]))
        got = v.drain()
        v.close()
        problems = [] if got == want else [f"{len(got)} verdicts for {len(want)} chunks, "
                                           f"{sum(a != b for a, b in zip(got, want))} differ"]
        grid = (batch + 63) // 64  # released slots are rows of the batch like any other
        slots = 3 if grid > cus else 2
        nbs = [width // 64] * (parts - 1) + [width // 64 + 1]
        record(name, (2 * grid * parts, sum(2 * grid * (nb + slots - 1) for nb in nbs)), problems)

    verifier("verifier 3-slot: 64 KiB x (64 CUs + 64)", 64 << 10, 64 * cus + 64)
    verifier("verifier 16 MiB x 4", 16 << 20, 4)
    verifier("verifier (4 MiB + 512) x 6, nblocks % 4 == 1", (4 << 20) + 512, 6)
    print("BARRIER_RESULTS " + json.dumps(results), flush=True)


def _run_child(mode, env, timeout):
    assert os.path.exists(DBG_LIB), "build_variants/dbgbar/libbtsha1.so missing: run `make dbgbar` first"
    env = dict(os.environ, BT_SHA1_LIB=DBG_LIB, HSA_ENABLE_IPC_MODE_LEGACY="0", **env)
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), mode], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BARRIER_RESULTS ")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0].split(" ", 1)[1])


def test_column_forms_match_the_barrier_invariant():
    results = _run_child("child-columns", {"BT_SHA1_COLUMN_MIN_MB": "0"}, 300)
    for c in results:
        print(c["case"], "want", c["want"], "got", c["got"], c["problems"])
    # cases a to d: 4 + 4 + 5 + 5 + 4 launches; three verifier batches
    assert len(results) == 22 + 3
    assert any("3-slot" in c["case"] and "MIDDLE" in c["case"] for c in results)
    bad = [c for c in results if not c["digests_ok"] or c["got"][2] != 0 or c["got"][:2] != c["want"]]
    assert not bad, bad


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
if __name__ == "__main__" and sys.argv[1:] == ["child-columns"]:
    _child_columns()
