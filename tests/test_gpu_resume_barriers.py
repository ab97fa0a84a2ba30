"""GPU: the barrier-accounting build (`make dbgbar`) on the resumable chain
kernel.  k_sha1_resume's loader wave S and round wave R meet at s_barrier from
different call sites, and whether a message advances or finishes is decided at
run time, so the kernel is correct only while both waves execute nbatch + 1
barriers, nbatch = ceil(nb / 64), nb = lens >> 6 for an advance and
(lens >> 6) + (r >= 56 ? 2 : 1) for a finish (sha1_kernels.hip).

A child process loads that build (BT_SHA1_LIB) and runs the advance / finish
shapes of resume_cases.py and a receiver run; for each it checks oracle-exact
results, zero misses, and the EXACT totals: 2 waves per message and
2 * (nbatch + 1) barriers per message.
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import PKG, REPO

pytestmark = pytest.mark.gpu
DBG_LIB = os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so")


def _child():
    import torch
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, PKG)
    import btsha1 as bt
    import py_oracle as orc
    import resume_cases as rc

    assert torch.cuda.is_available()
    assert os.path.samefile(bt.LIB_PATH, DBG_LIB), bt.LIB_PATH
    bt.debug_barrier_stats(reset=True)
    results = []

    def report(name, launches, problems):
        got = bt.debug_barrier_stats(reset=True)
        results.append({"case": name, "want": list(rc.barrier_want(launches)), "got": list(got),
                        "problems": problems})

    rc.run_advances(bt, torch, orc, report)
    rc.run_finishes(bt, torch, orc, report, compare_chunks_dev=False)  # bt_sha1_chunks_dev would add k_sha1_chain's waves
    rc.run_mixed(bt, torch, orc, report)
    rc.run_read_bound(bt, torch, orc, report)
    rc.run_pinned(bt, torch, orc, report)

    # a receiver run: the single-message launches of the host object
    for chunk_len, stride in ((12 * 1024 + 192, 4096), (4160, 64), (64 * 130 + 57, rc.NEVER)):
        data = bytes(orc.fill_synthetic(chunk_len, chunk_len, 0x4EC))
        want = orc.sha1(data)
        rx = bt.Receiver(chunk_len=chunk_len, nslots=2, stride=stride)
        rx.receive(data, want, 7)
        got = rx.drain()
        rx.close()
        launches, _, _ = rc.stride_rule(chunk_len, stride)
        report(f"receiver {chunk_len} bytes, stride {stride}", launches,
               [] if got == [(7, True, want)] else [f"verdict {got}"])
    print("BARRIER_RESULTS " + json.dumps(results), flush=True)


def test_resume_kernel_matches_the_barrier_invariant():
    assert os.path.exists(DBG_LIB), "build_variants/dbgbar/libbtsha1.so missing: run `make dbgbar` first"
    env = dict(os.environ, BT_SHA1_LIB=DBG_LIB, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "child"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BARRIER_RESULTS ")]
    assert len(line) == 1, r.stdout[-2000:]
    results = json.loads(line[0].split(" ", 1)[1])
    for c in results:
        print(c["case"], "want", c["want"], "got", c["got"], c["problems"])
    # 7 single advances + 8 chained; 3 finish launches; mixed; read bound; pinned; 3 receiver runs
    assert len(results) == 15 + 3 + 1 + 1 + 1 + 3
    assert any(c["want"][0] > 2 for c in results) and all(c["want"][1] > 0 for c in results)
    bad = [c for c in results if c["problems"] or c["got"][2] != 0 or c["got"][:2] != c["want"]]
    assert not bad, bad


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
