"""GPU: the barrier-accounting build (`make dbgbar`) on k_sha1_gather_lat.  Its
loader wave S steps through segment lists and its round wave R runs to the
longest message of their 64; only S reads the descriptors and publishes the
block counts, so the kernel is correct only while both waves execute exactly
nbmax + SLOTS - 1 barriers.

A child process loads that build (BT_SHA1_LIB), turns the knob on and runs
  two slots    130 messages: the walk's cases in turn (the empty message,
               r < 56 and r >= 56, lengths mixed inside a workgroup), two
               that share a segment, the longest (77 blocks) in the last lane
               of a partly filled workgroup, digests and fused verdicts;
  three slots  64 x CUs + 1 messages of 100 .. 300 bytes with empty messages
               (seg_count 0) and one-segment messages of 1 .. 299 bytes
               swapped in, the last workgroup one empty message (nbmax 1)
and checks exact digests, zero misses and the EXACT totals: 2 waves per
workgroup and the sum over workgroups of 2 * (nbmax + SLOTS - 1) barriers,
computed here from the lengths -- which also proves which kernel ran."""
import json
import os
import subprocess
import sys

import pytest

from conftest import PKG, REPO

pytestmark = pytest.mark.gpu
DBG_LIB = os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so")


def _child():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, PKG)
    import btsha1 as bt
    import gather_lat_cases as glc

    assert torch.cuda.is_available()
    assert os.path.samefile(bt.LIB_PATH, DBG_LIB), bt.LIB_PATH
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()

    prev = bt.set_seglist_latency_batch(2**64 - 1)
    results = []
    try:
        bt.debug_barrier_stats(reset=True)
        mixed, small = glc.mixed_batch(), glc.small_batch()
        for case, slots, batch, (first, count, want, lens) in (
                ("two slots", 2, mixed, glc.longest_last(mixed, 130)),
                ("three slots", 3, small, glc.tiled_with_seams(small, 64 * cus + 1))):
            n, problems = len(lens), []
            if bt.seglist_kernel_name(n) != "k_sha1_gather_lat<%d>" % slots:
                problems.append(bt.seglist_kernel_name(n))
            blob, segs, d_first, d_count = dev(batch["blob"]), dev(batch["segs"]), dev(first), dev(count)
            dig = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
            ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
            exp = dev(np.frombuffer(want, dtype=np.uint8))
            bt.gather_dev(blob.data_ptr(), segs.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), n, dig.data_ptr())
            torch.cuda.synchronize()
            if bytes(dig.cpu().numpy()) != want:
                problems.append("digests differ")
            bt.gather_verify_dev(blob.data_ptr(), segs.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), n,
                                 exp.data_ptr(), ok.data_ptr(), None)
            torch.cuda.synchronize()
            if bytes(ok.cpu().numpy()) != bytes([1]) * n:
                problems.append("verdicts differ")
            got = bt.debug_barrier_stats(reset=True)
            waves, bars = glc.barrier_want(lens, slots)
            results.append({"case": case, "workgroups": (n + 63) // 64, "want": [2 * waves, 2 * bars],
                            "got": list(got), "problems": problems})
    finally:
        bt.set_seglist_latency_batch(prev)
    print("BARRIER_RESULTS " + json.dumps(results), flush=True)


def test_gather_latency_kernel_matches_the_barrier_invariant():
    assert os.path.exists(DBG_LIB), "build_variants/dbgbar/libbtsha1.so missing: run `make dbgbar` first"
    env = dict(os.environ, BT_SHA1_LIB=DBG_LIB, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "child"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BARRIER_RESULTS ")]
    assert len(line) == 1, r.stdout[-2000:]
    results = json.loads(line[0].split(" ", 1)[1])
    for c in results:
        print(c["case"], c["workgroups"], "workgroups, want", c["want"], "got", c["got"], c["problems"])
    assert [c["case"] for c in results] == ["two slots", "three slots"]
    # two launches each: 2 waves per workgroup; the two-slot case's last workgroup runs to 77 blocks
    assert all(c["want"][0] == 2 * 2 * c["workgroups"] and c["want"][1] > c["want"][0] for c in results)
    assert results[0]["want"][1] == 2 * 2 * ((4 + 1) + (4 + 1) + (77 + 1))
    bad = [c for c in results if c["problems"] or c["got"][2] != 0 or c["got"][:2] != c["want"]]
    assert not bad, bad


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
