"""GPU: the barrier-accounting build (`make dbgbar`) on k_sha1_gather_chain.
Wave 0 builds each window and decides the piece, both waves meet at one
barrier per window and then run gather_resume_body, whose loader and round
waves meet nbatch + 1 times; the kernel is correct only while both waves
execute, per message,
    T + sum over body calls of (nbatch + 1)
barriers (T windows; the empty message builds one and calls nothing).

A child process loads that build (BT_SHA1_LIB) and runs, through
bt_sha1_segchain_dev,
  padding   segchain_cases.padding_batch: both empty messages, every tail
            length, the 354-datagram chunk (129 batches in one call);
  windows   one message of 2049 segments of 1 .. 3 bytes: three windows or more;
  pieces    piece_bytes = 64 on 10 KiB in 37 segments: 160 body calls
and checks exact digests and verdicts, zero misses and the EXACT totals, which
segchain_cases.plan / barriers derive from the segment lengths alone."""
import json
import os
import subprocess
import sys

import pytest

from conftest import PKG, REPO

pytestmark = pytest.mark.gpu
DBG_LIB = os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so")
CASES = ["padding", "windows", "pieces"]


def _child():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, PKG)
    import btsha1 as bt
    import py_oracle
    import segchain_cases as sc

    assert torch.cuda.is_available()
    assert os.path.samefile(bt.LIB_PATH, DBG_LIB), bt.LIB_PATH

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()

    window = sc.window_batch()
    one = dict(window, first=window["first"][4:5], count=window["count"][4:5], want=window["want"][80:100],
               seg_list=window["seg_list"], n=1)
    lens4 = sc.lengths(window, 4)
    results = []
    bt.debug_barrier_stats(reset=True)
    for case, batch, lens_of, piece in (("padding", sc.padding_batch(py_oracle), None, 0),
                                        ("windows", one, [lens4], 0),
                                        ("pieces", sc.piece_batch(), None, 64)):
        n = 1 if case != "padding" else batch["n"]
        lens = lens_of or [sc.lengths(batch, i) for i in range(n)]
        want, problems = batch["want"][:20 * n], []
        tables = [dev(batch[k]) for k in ("blob", "segs", "first", "count")]
        dig = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
        ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        exp = dev(np.frombuffer(want, dtype=np.uint8))
        bt.segchain_dev(*(t.data_ptr() for t in tables), n, exp.data_ptr(), ok.data_ptr(), dig.data_ptr(), piece)
        torch.cuda.synchronize()
        if bytes(dig.cpu().numpy()) != want:
            problems.append("digests differ")
        if bytes(ok.cpu().numpy()) != bytes([1]) * n:
            problems.append("verdicts differ")
        got = bt.debug_barrier_stats(reset=True)
        per = [sc.barriers(l, piece or sc.PIECE) for l in lens]
        results.append({"case": case, "messages": n, "windows": [len(sc.plan(l, piece or sc.PIECE)) for l in lens],
                        "want": [2 * sum(c for c, _ in per), 2 * sum(b for _, b in per)], "got": list(got),
                        "problems": problems})
    print("BARRIER_RESULTS " + json.dumps(results), flush=True)


def test_segchain_kernel_matches_the_barrier_invariant():
    assert os.path.exists(DBG_LIB), "build_variants/dbgbar/libbtsha1.so missing: run `make dbgbar` first"
    env = dict(os.environ, BT_SHA1_LIB=DBG_LIB, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "child"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BARRIER_RESULTS ")]
    assert len(line) == 1, r.stdout[-2000:]
    results = json.loads(line[0].split(" ", 1)[1])
    for c in results:
        print(c["case"], c["messages"], "messages, windows", c["windows"], "want", c["want"], "got", c["got"],
              c["problems"])
    assert [c["case"] for c in results] == CASES
    pad, win, pie = results
    # every padding message is one window; the chunk's one call is 8193 blocks in 129 batches
    assert pad["messages"] == 16 and set(pad["windows"]) == {1}
    assert pad["want"][0] == 2 * (16 + 14)  # the two empty messages call nothing
    assert pad["want"][1] == 2 * (16 + 13 * 2 + 130)
    assert win["windows"][0] >= 3 and win["want"] == [2 * (1 + win["windows"][0]), 2 * 3 * win["windows"][0]]
    assert pie["windows"] == [160] and pie["want"] == [2 * 161, 2 * 160 * 3]  # per piece: a window, one batch + 1
    bad = [c for c in results if c["problems"] or c["got"][2] != 0 or c["got"][:2] != c["want"]]
    assert not bad, bad


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
