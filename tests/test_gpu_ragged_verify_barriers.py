"""GPU: the barrier-accounting build (`make dbgbar`) on the ragged latency
kernel's verify form.  k_sha1_lat_ragged_verify's loader wave S and round wave
R meet at s_barrier from different call sites and run to the longest message
of their 64, so the kernel is correct only while both waves execute nbmax +
SLOTS - 1 barriers; the fused compare sits in R's epilogue, after the check,
and must add none.

A child process loads that build (BT_SHA1_LIB) and runs the lat2 and lat3
launches of ragged_verify_cases.py -- lengths mixed inside a workgroup, a
workgroup of empty messages, a partly filled last workgroup -- and for each
checks exact verdicts and digests, zero misses, and the EXACT totals: 2 waves
per workgroup and the sum over workgroups of 2 * (nbmax + SLOTS - 1) barriers,
computed here from the lengths.
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
    import ragged_verify_cases as rv
    import test_gpu_launch_forms as lf
    import verdict_cases as vc

    assert torch.cuda.is_available()
    assert os.path.samefile(bt.LIB_PATH, DBG_LIB), bt.LIB_PATH
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bt.debug_barrier_stats(reset=True)
    results = []
    for form, slots in (("lat2", 2), ("lat3", 3)):
        problems = []
        try:
            lens, launches = rv.run_form(bt, torch, lf, vc, orc, form, cus)
        except AssertionError as e:
            problems.append(str(e)[:500])
            lens, launches = rv.lengths(rv.n_for(form, cus)), 3
        got = bt.debug_barrier_stats(reset=True)
        results.append({"case": form, "workgroups": (len(lens) + 63) // 64,
                        "want": list(rv.barrier_want(lens, slots, launches)), "got": list(got), "problems": problems})
    print("BARRIER_RESULTS " + json.dumps(results), flush=True)


def test_ragged_verify_kernel_matches_the_barrier_invariant():
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
    assert [c["case"] for c in results] == ["lat2", "lat3"]
    # three launches each: 2 waves per workgroup; workgroup 0 alone runs to 66 blocks
    assert all(c["want"][0] == 3 * 2 * c["workgroups"] and c["want"][1] > c["want"][0] for c in results)
    bad = [c for c in results if c["problems"] or c["got"][2] != 0 or c["got"][:2] != c["want"]]
    assert not bad, bad


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
