"""GPU: the barrier-accounting build (`make dbgbar`) on the chain-form gather
kernels.  In k_sha1_gather_resume and k_sha1_gather_resume_table the loader
wave S and the round wave R of every workgroup meet at s_barrier from different
call sites, and whether an entry advances or finishes is read at run time, so
the kernels are correct only while both waves of every entry execute
nbatch + 1 barriers (nbatch as in k_sha1_resume: resume_cases.nbatch).

A child process loads that build (BT_SHA1_LIB) and runs the seam cases of
gather_resume_cases.py in both forms -- the array form with a mixed advance /
finish launch, the table form through a gather intake with a mixed table; for
each launch it checks oracle-exact results, zero misses, and the EXACT totals:
2 waves per entry and 2 * (nbatch + 1) barriers per entry.
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
    import gather_resume_cases as grc
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

    grc.run_seams(bt, torch, orc, report, mixed=True)
    grc.run_intake_seams(bt, orc, report)
    print("BARRIER_RESULTS " + json.dumps(results), flush=True)


def test_gather_resume_kernels_match_the_barrier_invariant():
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
    # array form: advance, mixed launch, finishes; table form: advance, mixed table, finishes
    assert len(results) == 3 + 3
    assert all(c["want"][0] >= 6 and c["want"][1] > c["want"][0] for c in results)
    bad = [c for c in results if c["problems"] or c["got"][2] != 0 or c["got"][:2] != c["want"]]
    assert not bad, bad


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
